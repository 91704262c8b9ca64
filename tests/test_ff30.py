"""Signed radix-2^30 Montgomery arithmetic (csrc/ff30.hpp, the 13-limb BLS12-381 Fq prototype)
checked on the host against Python integers: congruences mod p, the magnitude bounds the header
states, the limb states (exact / near), canonicalisation and the 32-bit Montgomery round trip
including max-limb stress operands (a column overflow shows as a wrong residue); and its mixed
add (ec30.hpp) word for word against the radix-2^29 one (ec29.hpp) on chains of random inputs."""
import json
import os
import subprocess

import pytest

from limb_bounds import check30

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ff30") / "ff30_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "ff30_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    return [json.loads(ln) for ln in out.splitlines()]


def test_ff30_field_ops(lines):
    seen = set()
    for d in lines:
        seen.add(d["op"])
        check30(d)
    assert {"mul", "mul2", "add", "sub", "canon", "mont"} <= seen


def test_ff30_madd_matches_radix29(lines):
    res = [d for d in lines if d["op"] == "madd"][0]
    assert res["checked"] == 2560 and res["bad"] == 0
    chains = [d for d in lines if d["op"] == "madd_chain"]
    assert [c["inf"] for c in chains[38:]] == [1, 1]


def test_ff30_add_dbl_and_tables_match_radix29(lines):
    """general adds (with equal / opposite operands), doublings, and pack_aff -> load -> store"""
    res = [d for d in lines if d["op"] == "add" and "checked" in d][0]
    assert res["checked"] == 24 * 36 and res["bad"] == 0 and res["table_bad"] == 0

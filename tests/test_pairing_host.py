"""The BN254 pairing tower of csrc/pairing.hpp on the host (tests/cpp/pairing_check.cpp, built
with g++ and the address / undefined-behaviour sanitizers and run directly): Fq2 / Fq6 / Fq12
products against schoolbook, squares against products, inverses, Frobenius against a^p and
Frobenius^12 == identity, e(G, H) != 1, e(G, H)^r == 1, e(aG, bH) == e(G, H)^(ab) for 8 seeded
pairs, the sparse line product, and the precomputed-line Miller loop against the on-the-fly one."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_constants_are_the_generators(tmp_path):
    """csrc/pairing_consts.hpp is what tools/gen_pairing.py derives (Frobenius constants, twist,
    digits; the generator asserts the curve facts and the hard part's exponent with integers)"""
    import sys
    pkg = os.path.join(os.path.dirname(HERE), "verkle-kzg_amd")
    out = tmp_path / "pairing_consts.hpp"
    subprocess.check_call([sys.executable, os.path.join(pkg, "tools", "gen_pairing.py"), str(out)])
    assert out.read_bytes() == open(os.path.join(pkg, "csrc", "pairing_consts.hpp"), "rb").read()


def test_pairing_tower_and_bilinearity(tmp_path):
    exe = tmp_path / "pairing_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "pairing_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True, timeout=300)
    d = json.loads(out.splitlines()[-1])
    assert d["checks"] >= 300
    assert d["mismatches"] == 0, d

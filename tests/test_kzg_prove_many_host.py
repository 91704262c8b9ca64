"""KZG batch proving (vc_kzg_prove_many) without a GPU.

* the expected-proof shortcut of tests/kzg_prove_cases.py (one scalar multiplication of g by
  sum_j c_j q_j) against protocol.KZG.prove_point itself, N = 16;
* the per-lane arithmetic of csrc/kzg_many.hpp on the host (tests/cpp/kzg_many_check.cpp, built with
  g++ and the address / undefined-behaviour sanitizers and run directly), a wave emulated as 64 lanes
  in a loop: the point's class, z^N - 1, y and the whole quotient row against the oracle's,
  N = 2, 16, 64, 256;
* both kernels are in the cross-built gfx950 code object, within the register budget DESIGN.md 4.9
  records, without spills."""
import json
import os
import random
import subprocess
import sys

import pytest

import kzg_prove_cases as cases
from pyoracle import protocol

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
R = cases.R


def test_expected_proof_is_prove_points():
    N = 16
    kzg = protocol.KZG(N, secret=cases.SECRET)
    assert tuple(kzg.lagrange_scalars) == cases.scalars(N)
    assert kzg.pre.omega == cases.omega(N) == cases.oracle(N).pre.omega
    full, short = cases.row(N, N, 1), cases.row(N, N - 3, 2)
    for evals, point in ((full, 0), (full, N - 1), (short, N - 2), (full, N + 1), (short, R - 2),
                         (short, random.Random(5).randrange(R))):
        want = kzg.prove_point(None, point, protocol.LagrangeBasis(list(evals), N))
        assert want["proof"] is not None
        assert cases.expected(N, evals, point) == want, point
    assert cases.expected(N, (7,) * N, 3) == {"proof": None, "y": 7}        # a constant: q = 0
    with pytest.raises(IndexError):
        cases.quotient(N, full, N)


def _points(N, width, rng):
    w = cases.omega(N)
    pts = [0, N - 1, width if width < N else N - 1, N, N + 1, R - 1, R - 2, rng.randrange(N + 2, R)]
    if N >= 16:
        pts.append(pow(w, 3, R))
    return pts


def _class_of(N, evals, point):
    """0 in the domain, 1 outside, 2 where the reference panics -- from the oracle alone"""
    try:
        cases.quotient(N, evals, point)
    except (IndexError, ZeroDivisionError, ValueError):
        return 2
    return 0 if point < N else 1


def test_lane_arithmetic_under_the_sanitizers(tmp_path):
    rng = random.Random(2024)
    lines, want = [], {0: 0, 1: 0, 2: 0}
    for N in (2, 16, 64, 256):
        width = N - 3 if N > 4 else 1
        evals = cases.row(N, width, 3)
        for point in _points(N, width, rng):
            cls = _class_of(N, evals, point)
            want[cls] += 1
            lines.append("%d %d %d" % (N, width, cls))
            lines.append("%x" % point)
            lines += ["%x" % v for v in evals]
            lines.append("%x" % ((pow(point, N, R) - 1) % R))
            if cls != 2:
                q, y = cases.quotient(N, evals, point)
                lines.append("%x" % y)
                lines += ["%x" % v for v in q]
    ncases = sum(want.values())
    # the reference panics at N, at w^3 and at r - 1 = w^(N / 2), a domain element of every even N
    assert want[2] == 4 + 3 + 4 and want[0] >= 11 and want[1] >= 11
    flat = tmp_path / "cases.txt"
    flat.write_text("%d\n" % ncases + "\n".join(lines) + "\n")
    exe = tmp_path / "kzg_many_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "kzg_many_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe), str(flat)], text=True, timeout=600)
    d = json.loads(out.splitlines()[-1])
    print(d)
    assert d["cases"] == ncases
    assert d["wrong"] == 0, d
    assert (d["in_domain"], d["outside"], d["domain_error"]) == (want[0], want[1], want[2])
    assert d["rows"] == want[0] + want[1]


def test_kernels_in_the_code_object_within_their_register_budget():
    """both kernels within 128 VGPRs + AGPRs (256-lane blocks at four waves per SIMD),
    neither spilling, on both scalar fields"""
    sys.path.insert(0, os.path.join(ROOT, "verkle-kzg_amd", "tools"))
    import vkzg
    from kernel_regs import kernel_regs
    rows = kernel_regs(vkzg.LIB_PATH, "k_kzg_many_")
    for kern in ("k_kzg_many_lane", "k_kzg_many_wave"):
        hit = [r for r in rows if kern in r[0]]
        assert len(hit) == 2, (kern, rows)              # BN254 Fr and BLS12-381 Fr
        for name, vgpr, agpr, spills in hit:
            print(name, vgpr, agpr, spills)
            assert spills == 0, (name, spills)
            assert vgpr + agpr <= 128, (name, vgpr, agpr)

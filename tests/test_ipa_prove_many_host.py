"""IPA batch proving (vc_ipa_prove_many) without a GPU.

* the shared text of csrc/ipa_many.hpp on the host (tests/cpp/ipa_many_check.cpp, built with g++ and
  the address / undefined-behaviour sanitizers and run directly): openings at N = 2, 4 and 32 -- in
  the domain and outside, an all-zero row under the identity commitment among them -- run as the
  kernels run them, given the recorded L_k, R_k of the oracle's proof; the barycentric row, y, w and
  every x, every round's two scalar rows, every fold the device keeps and the tip equal the oracle's
  field side (tests/ipa_prove_cases.py); the two N = 256 openings of tests/golden/ipa_256.json give
  the file's y and tip;
* the new kernels are in the cross-built gfx950 code object within the register budget DESIGN.md
  4.14 records, without spills;
* the statuses decided before a context is looked at: a NULL context with good or bad arguments is
  VC_E_INVALID and writes nothing."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

import ipa_prove_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
R = cases.R


def _pt(P):
    return "1 0 0" if P is None else "0 %x %x" % P


def _opening(N, evals, point, com, proof, full):
    K = len(proof["l"])
    lines = ["%d %d %d" % (N, K, int(full)), _pt(com), "%x" % point] + ["%x" % v for v in evals]
    lines += ["%x" % proof["y"], "%x" % proof["tip"]]
    tr = cases.field_trace(N, evals, point, com, proof["l"], proof["r"]) if full else None
    if full:
        assert tr["y"] == proof["y"] and tr["tip"] == proof["tip"]      # the trace restates the oracle's prover
        lines += ["%x" % tr["w"]] + ["%x" % v for v in tr["b"]]
    for k in range(K):
        lines += [_pt(proof["l"][k]), _pt(proof["r"][k])]
        if full:
            rd = tr["rounds"][k]
            lines.append("%x" % rd["x"])
            for key in ("sl", "sr", "a", "b", "coeff"):
                lines += ["%x" % v for v in rd[key]]
    return lines


def test_shared_text_under_the_sanitizers(tmp_path):
    lines, count, rows, folds = [], 0, 0, 0
    for N in (2, 4, 32):
        evals = cases.row(N, 1)
        com = cases.commitment(N, evals)
        K = N.bit_length() - 1
        for p in cases.standard_points(N):
            lines += _opening(N, evals, p, com, cases.expected(N, evals, p), True)
            count += 1
            rows += 2 * (N + 1) * K
            folds += sum(2 * (N >> r) + N for r in range(1, K))
    zero = (0,) * 4                                                  # the identity's transcript encoding
    for p in (1, 9):
        pr = cases.expected(4, zero, p, None)
        assert pr["l"] == pr["r"] == [None, None] and pr["tip"] == pr["y"] == 0
        lines += _opening(4, zero, p, None, pr, True)
        count += 1
        rows += 2 * 5 * 2
        folds += 2 * 2 + 4
    data, com, proofs = cases.golden256()
    for pr in proofs:
        lines += _opening(256, data, pr["point"], com, pr, False)
        count += 1
    flat = tmp_path / "openings.txt"
    flat.write_text("\n".join([str(count)] + lines) + "\n")
    exe = tmp_path / "ipa_many_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "ipa_many_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe), str(flat)], text=True, timeout=600)
    d = json.loads(out.splitlines()[-1])
    print(d)
    assert d["openings"] == count == 22 and d["widths"] == 2 | 4 | 32 | 256
    assert d["inside"] == 3 * 3 + 1 + 1 and d["outside"] == 3 * 3 + 1 + 1
    assert d["ys"] == d["tips"] == count and d["ys_bad"] == 0 and d["tips_bad"] == 0, d
    assert d["weights"] == 6 * (2 + 4 + 32) + 2 * 4 and d["weights_bad"] == 0, d
    assert d["challenges"] == 6 * (2 + 3 + 6) + 2 * 3 and d["challenges_bad"] == 0, d     # w and every x
    assert d["rows"] == rows and d["rows_bad"] == 0, d
    assert d["folds"] == folds > 0 and d["folds_bad"] == 0, d


def test_kernels_in_the_code_object_within_their_register_budget():
    """a wave per opening, one wave per block; init and round within 256 VGPRs + AGPRs
    (two waves per SIMD), finish within 128, none spilling"""
    sys.path.insert(0, os.path.join(ROOT, "verkle-kzg_amd", "tools"))
    import vkzg
    from kernel_regs import kernel_regs
    found = {name: (v, a, s) for name, v, a, s in kernel_regs(vkzg.LIB_PATH, "k_ipa_many_")}
    budget = {"k_ipa_many_init": 256, "k_ipa_many_round": 256, "k_ipa_many_finish": 128}
    for kern, limit in budget.items():
        hit = [r for name, r in found.items() if kern in name]
        assert len(hit) == 1, (kern, sorted(found))
        vgpr, agpr, spills = hit[0]
        print(kern, vgpr, agpr, spills)
        assert vgpr + agpr <= limit, (kern, vgpr, agpr)
        assert spills == 0, (kern, spills)


def test_a_null_context_is_invalid_and_writes_nothing():
    from vkzg._lib import lib
    N, K, n = 4, 2, 3
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
    data = np.ones((n * N, 4), dtype=np.uint64)
    com, cinf = np.ones((n, 8), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    pts = np.array([[1, 0, 0, 0], [9, 0, 0, 0], [2**64 - 1] * 4], dtype=np.uint64)      # (the last one >= r)
    row = np.array([0, 7, 1], dtype=np.uint32)                                          # (one >= rows)
    for fn in ("vc_ipa_prove_many", "vc_ipa_prove_many_device"):
        for Nv, nv, r_, d_ in ((N, n, None, data), (N, n, row, data), (3, n, None, data), (512, n, None, data),
                               (N, n, None, None), (N, 0, None, None)):
            outs = [np.full((n * K, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(n * K, 0xA5, dtype=np.uint8),
                    np.full((n * K, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(n * K, 0xA5, dtype=np.uint8),
                    np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)]
            st = getattr(lib(), fn)(None, 0, Nv, n, P(d_), P(r_), P(com), P(cinf), P(pts), nv, *[P(o) for o in outs])
            assert st == -1, (fn, Nv, nv)
            assert all((o == (0xA5 if o.dtype == np.uint8 else 0xA5A5A5A5A5A5A5A5)).all() for o in outs)

"""KZG subvector proofs without a GPU.

* the helper tests/kzg_sub_cases.py (trapdoor proof, long-division quotient row) against
  protocol.KZG itself at N = 16: the proof is sum c_i prove_point(i), the row sum c_i quotient(i);
* the per-lane arithmetic of csrc/kzg_sub.hpp on the host (tests/cpp/kzg_sub_check.cpp, built with
  g++ and the address / undefined-behaviour sanitizers and run directly), a wave emulated as 64 lanes
  in a loop: the weights and the whole quotient row against the helper's, N = 2, 16, 64, 128, 256;
* vc_kzg_subvector_weights, vc_kzg_powers_from_secret, the key and vc_kzg_verify_subvector on both
  curves: proofs made with the trapdoor, verdicts exact;
* the kernel is in the cross-built gfx950 code object within the register figure DESIGN.md 4.12
  records, without spills."""
import json
import os
import random
import subprocess
import sys

import pytest

import bls12_381_g2
import bn254_g2
import kzg_sub_cases as cases
from pyoracle import protocol
from pyoracle.curves import BLS12_381, BLS_P, BN254, BN254_P, BN254_R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
R = BN254_R
VC_E_INVALID, VC_E_RANGE = -1, -5


def _status(fn):
    from vkzg._lib import VCError
    with pytest.raises(VCError) as ei:
        fn()
    return ei.value.status


# ---------------------------------------------------------------- the helper against the oracle
def test_helper_is_the_weighted_sum_of_prove_points():
    N = 16
    kzg = protocol.KZG(N, secret=cases.SECRET)
    assert tuple(kzg.lagrange_scalars) == cases.scalars(N)
    for evals in (cases.row(N, N, 1), cases.row(N, N - 3, 2)):
        data = protocol.LagrangeBasis(list(evals), N)
        for S in ([5], [0, 15], [3, 14, 7, 0, 13], list(range(15)), [15, 14, 13]):
            c = cases.weights(N, S)
            singles = [kzg.prove_point(None, i, data) for i in S]
            want = BN254.msm([p["proof"] for p in singles], c)
            got = cases.expected(N, evals, S)
            assert got["proof"] == want and want is not None, S
            assert got["ys"] == [p["y"] for p in singles]
            rows = [kzg.quotient(i, data)[0] for i in S]
            assert cases.quotient_row(N, evals, S) == [sum(ci * q[j] for ci, q in zip(c, rows)) % R for j in range(N)]
        full = list(range(N))
        random.Random(3).shuffle(full)
        assert cases.expected(N, evals, full)["proof"] is None       # k = N: q = 0
        assert cases.quotient_row(N, evals, full) == [0] * N
    # the order of a set changes nothing but the order of the ys
    a, b = cases.expected(N, evals, [3, 9, 12]), cases.expected(N, evals, [12, 3, 9])
    assert a["proof"] == b["proof"] and a["ys"] == [b["ys"][1], b["ys"][2], b["ys"][0]]


# ---------------------------------------------------------------- the lane text under the sanitizers
def test_lane_arithmetic_under_the_sanitizers(tmp_path):
    lines, ncases, ks = [], 0, set()
    for N in (2, 16, 64, 128, 256):
        width = N - 3 if N > 4 else 1
        for wd, seed in ((width, 3), (N, 4)):
            evals = cases.row(N, wd, seed)
            sets = cases.standard_sets(N, wd) if wd == width else [cases.standard_sets(N, wd)[-1], [0, N - 1]]
            for S in sets:
                ncases += 1
                ks.add((N, len(S)))
                lines.append("%d %d %d" % (N, wd, len(S)))
                lines.append(" ".join(str(i) for i in S))
                lines += ["%x" % v for v in evals]
                lines += ["%x" % v for v in cases.weights(N, S)]
                lines += ["%x" % v for v in cases.quotient_row(N, evals, S)]
    for N, k in ((2, 1), (2, 2), (16, 15), (64, 63), (64, 64), (128, 65), (128, 127), (256, 63), (256, 64), (256, 65),
                 (256, 255), (256, 256)):
        assert (N, k) in ks, (N, k)
    sets256 = cases.standard_sets(256, 253)
    assert any(0 in S and 255 in S for S in sets256) and [253, 254, 255] in sets256
    assert any(S != sorted(S) for S in sets256)
    flat = tmp_path / "cases.txt"
    flat.write_text("%d\n" % ncases + "\n".join(lines) + "\n")
    exe = tmp_path / "kzg_sub_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "kzg_sub_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe), str(flat)], text=True, timeout=600)
    d = json.loads(out.splitlines()[-1])
    print(d)
    assert d["cases"] == ncases and ncases >= 50
    assert d["wrong"] == 0, d
    assert d["entries"] > 5000 and d["weights"] > 1000


# ---------------------------------------------------------------- weights
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_weights_are_the_helpers(curve):
    from vkzg import scheme
    for N, S in ((2, [1]), (2, [1, 0]), (16, [3, 14, 7, 0, 13]), (256, list(range(255, 190, -1))), (1024, [0, 1023, 512])):
        assert scheme.kzg_subvector_weights(N, S, curve) == cases.weights(N, S, curve), (N, S)


def test_weights_refuse_a_bad_set():
    from vkzg import scheme
    for N, S in ((16, [3, 3]), (16, [16]), (16, []), (12, [1]), (1, [0]), (16, [1, 5, 9, 1])):
        assert _status(lambda: scheme.kzg_subvector_weights(N, S)) == VC_E_INVALID, (N, S)
    with pytest.raises(ValueError):
        scheme.kzg_subvector_weights(16, [1], "bandersnatch")


# ---------------------------------------------------------------- powers
@pytest.mark.parametrize("secret", [cases.SECRET, R - 2])
def test_powers_from_secret_are_the_integer_arithmetic(secret):
    from vkzg import scheme
    g1, g2 = scheme.kzg_powers_from_secret(secret, 4)
    assert g1 == [BN254.mul(BN254.g, pow(secret, t, R)) for t in range(4)]
    assert g2 == [bn254_g2.mul(bn254_g2.H, pow(secret, t, R)) for t in range(5)]
    assert g1[0] == BN254.g and g2[0] == bn254_g2.H
    assert _status(lambda: scheme.kzg_powers_from_secret(0, 4)) == VC_E_INVALID


# ---------------------------------------------------------------- the verifier, BN254
KS = {16: 16, 256: 20}       # the keys' K per domain


@pytest.fixture(scope="module")
def keys():
    from vkzg import scheme
    made = {}

    def get(N):
        if N not in made:
            made[N] = scheme.KZGSubvectorKey(*scheme.kzg_powers_from_secret(cases.SECRET, KS[N]), N)
        return made[N]
    return get


def _commitment(N, evals, curve="bn254"):
    C = cases.curve_of(curve)
    return C.mul(C.g, sum(c * v for c, v in zip(cases.scalars(N, curve), evals)) % C.r)


def _statement(N, k, seed=7):
    evals = cases.row(N, N - 3, seed)
    rng = random.Random(100 * N + k)
    if k == 1:
        S = [rng.randrange(N)]
    else:                                                   # 0 and N - 1 among them, in no order
        S = [0, N - 1] + rng.sample(range(1, N - 1), k - 2)
        rng.shuffle(S)
    return evals, S, _commitment(N, evals), cases.expected(N, evals, S)


@pytest.mark.parametrize("N,k", [(16, 1), (16, 2), (16, 16), (256, 1), (256, 2), (256, 16), (256, 20)])
def test_verdicts(keys, N, k):
    key = keys(N)
    assert k <= key.K == KS[N]
    evals, S, C, ex = _statement(N, k)
    ys, pi = ex["ys"], ex["proof"]
    assert (pi is None) == (k == N)
    assert key.verify(C, S, ys, pi) is True
    perm = list(range(k))
    random.Random(k).shuffle(perm)
    assert key.verify(C, [S[p] for p in perm], [ys[p] for p in perm], pi) is True
    # each single tamper
    t = k // 2
    bad_y = list(ys)
    bad_y[t] = (ys[t] + 1) % R
    assert key.verify(C, S, bad_y, pi) is False
    other = cases.expected(N, evals, [(S[0] + 1) % N] if k == 1 else S[:-1])["proof"] if k < N else BN254.g
    assert other != pi
    assert key.verify(C, S, ys, other) is False
    assert key.verify(_commitment(N, cases.row(N, N - 3, 8)), S, ys, pi) is False
    if k < N:
        out = next(i for i in range(N) if i not in S)
        swapped = list(S)
        swapped[t] = out
        assert key.verify(C, swapped, ys, pi) is False
    if k >= 2:
        a, b = S.index(0), S.index(N - 1)                  # y = f_0 and y = 0 (N - 1 is beyond the row)
        assert ys[a] != ys[b]
        swapped_y = list(ys)
        swapped_y[a], swapped_y[b] = ys[b], ys[a]
        assert key.verify(C, S, swapped_y, pi) is False


def test_malformed_content_gives_verdict_zero(keys):
    N, k = 16, 5
    key = keys(N)
    evals, S, C, ex = _statement(N, k)
    ys, pi = ex["ys"], ex["proof"]
    assert key.verify(C, S, ys, pi) is True
    P = BN254_P
    off = (pi[0], (pi[1] + 1) % P)
    assert not BN254.is_on_curve(off)
    assert key.verify(C, S, ys, (pi[0] + P, pi[1])) is False         # a coordinate >= p
    assert key.verify(C, S, ys, (pi[0], pi[1] + P)) is False
    assert key.verify((C[0] + P, C[1]), S, ys, pi) is False
    assert key.verify(C, S, ys, off) is False                        # off the curve
    assert key.verify((C[0], (C[1] + 1) % P), S, ys, pi) is False
    assert key.verify(C, S, [ys[0] + R] + ys[1:], pi) is False       # y >= r
    assert key.verify(C, S, ys[:-1] + [R], pi) is False


def test_statuses(keys):
    from vkzg import scheme
    N = 256
    key = keys(N)
    K = key.K
    evals = cases.row(N, N - 3, 7)
    C = _commitment(N, evals)
    S = list(range(3, 3 + K + 1))
    ex = cases.expected(N, evals, S)
    assert _status(lambda: key.verify(C, S, ex["ys"], ex["proof"])) == VC_E_RANGE          # k = K + 1
    S = S[:K]
    ex = cases.expected(N, evals, S)
    assert key.verify(C, S, ex["ys"], ex["proof"]) is True
    assert _status(lambda: key.verify(C, [3, 4, 3], ex["ys"][:3], ex["proof"])) == VC_E_INVALID    # a duplicate
    assert _status(lambda: key.verify(C, [3, N], ex["ys"][:2], ex["proof"])) == VC_E_INVALID       # an index >= N
    assert _status(lambda: key.verify(C, [], [], ex["proof"])) == VC_E_INVALID
    # keys
    g1, g2 = scheme.kzg_powers_from_secret(cases.SECRET, 4)
    scheme.KZGSubvectorKey(g1, g2, 16)
    outside = bn254_g2.outside_subgroup()
    assert bn254_g2.on_twist(outside)
    off1 = (g1[2][0], (g1[2][1] + 1) % BN254_P)
    bad_keys = [(g1, [g2[1]] + g2[1:]),                     # g2[0] != H
                ([g1[1]] + g1[1:], g2),                     # g1[0] != G
                (g1, g2[:3] + [outside] + g2[4:]),          # outside the subgroup
                (g1[:2] + [off1] + g1[3:], g2),             # off the curve
                (g1, g2[:2] + [((g2[2][0][0] + BN254_P, g2[2][0][1]), g2[2][1])] + g2[3:])]    # a coordinate >= p
    for b1, b2 in bad_keys:
        assert _status(lambda: scheme.KZGSubvectorKey(b1, b2, 16)) == VC_E_INVALID
    assert _status(lambda: scheme.KZGSubvectorKey(g1, g2, 12)) == VC_E_INVALID             # not a power of two
    assert _status(lambda: scheme.KZGSubvectorKey(g1, g2, 2)) == VC_E_INVALID              # K > size
    with pytest.raises(ValueError):
        scheme.KZGSubvectorKey(g1, g2[:-1], 16)


def test_the_identity_commitment_accepts_the_identity_proof(keys):
    key = keys(16)
    S = [0, 7, 15]
    assert cases.expected(16, (0,) * 16, S) == {"proof": None, "ys": [0, 0, 0]}
    assert key.verify(None, S, [0, 0, 0], None) is True
    assert key.verify(None, S, [0, 1, 0], None) is False
    assert key.verify(None, S, [0, 0, 0], BN254.g) is False
    # a constant row: C = c G, I = c, the proof is the identity
    c = 12345
    assert cases.expected(16, (c,) * 16, S)["proof"] is None
    assert key.verify(BN254.mul(BN254.g, c), S, [c] * 3, None) is True


# ---------------------------------------------------------------- the verifier, BLS12-381
def test_bls12_381_verdicts():
    import kzg_batch_bls_cases as bls
    from vkzg import scheme
    curve, N, K = "bls12_381", 16, 6
    g1, g2 = scheme.kzg_powers_from_secret(cases.SECRET, K, curve)
    r = BLS12_381.r
    assert g1 == [BLS12_381.mul(BLS12_381.g, pow(cases.SECRET, t, r)) for t in range(K)]
    assert g2[:3] == [bls12_381_g2.mul(bls12_381_g2.H, pow(cases.SECRET, t, r)) for t in range(3)]
    key = scheme.KZGSubvectorKey(g1, g2, N, curve)
    evals = cases.row(N, N - 3, 5, curve)
    S = [14, 0, 15, 6, 9]
    C = _commitment(N, evals, curve)
    ex = cases.expected(N, evals, S, curve)
    assert ex["ys"][0] == 0 and ex["proof"] is not None
    assert key.verify(C, S, ex["ys"], ex["proof"]) is True
    assert key.verify(C, S, ex["ys"][:3] + [(ex["ys"][3] + 1) % r] + ex["ys"][4:], ex["proof"]) is False
    T = bls.fixture()["T"]
    assert T is not None and BLS12_381.is_on_curve(T) and not bls.in_subgroup(T)
    assert key.verify(C, S, ex["ys"], BLS12_381.add(ex["proof"], T)) is False      # outside the subgroup
    assert key.verify(BLS12_381.add(C, T), S, ex["ys"], ex["proof"]) is False
    assert key.verify(C, S, ex["ys"], (ex["proof"][0] + BLS_P, ex["proof"][1])) is False
    assert _status(lambda: scheme.KZGSubvectorKey(g1[:2] + [T] + g1[3:], g2, N, curve)) == VC_E_INVALID
    assert _status(lambda: scheme.KZGSubvectorKey(g1, g2[:2] + [bls12_381_g2.outside_subgroup()] + g2[3:], N,
                                                  curve)) == VC_E_INVALID


# ---------------------------------------------------------------- the kernel's registers
def test_kernel_in_the_code_object_within_its_register_figure():
    """k_kzg_sub_wave at 98 VGPRs, no AGPRs, no spills on both scalar fields (the
    target: 128, four waves per SIMD at 256-lane blocks)"""
    sys.path.insert(0, os.path.join(ROOT, "verkle-kzg_amd", "tools"))
    import vkzg
    from kernel_regs import kernel_regs
    hit = kernel_regs(vkzg.LIB_PATH, "k_kzg_sub_wave")
    assert len(hit) == 2, hit                           # BN254 Fr and BLS12-381 Fr
    for name, vgpr, agpr, spills in hit:
        print(name, vgpr, agpr, spills)
        assert spills == 0, (name, spills)
        assert vgpr + agpr <= 98, (name, vgpr, agpr)

"""KZG subvector batch verification without a GPU: the host path (ctx == NULL) of
vc_kzg_subvector_batch_fold / vc_kzg_verify_subvector_batch, the shared text under the sanitizers, the
kernel's register figures. Every expected value comes from Python integers (tests/kzg_subv_cases.py
over tests/kzg_sub_cases.py and pyoracle.curves): with pi_j = q_j G the expected P_t is
(sum_j rho^j z_{j,t} q_j) G, and the expected verdict is the trapdoor identity of every entry.

* the fold equals the integer fold on both curves (ragged k, a valid and an invalid batch), k = N;
* verdicts: three seeds, one changed y / proof / commitment located, cancelling errors, identities;
* every status, with the outputs untouched; malformed content is verdict 0 with VC_OK; n = 0;
* csrc/kzg_subv.hpp as the kernel runs it (64 lanes in a loop) and as the host path runs it, and
  miller_loop_tabn against miller_loop_tab2 and the general product (tests/cpp/kzg_subv_check.cpp,
  built with g++ and the address / undefined-behaviour sanitizers and run directly);
* k_kzg_subv_fold in the cross-built gfx950 code object within the register figures DESIGN.md 4.13
  records, without spills."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kzg_sub_cases as cases
import kzg_subv_cases as sv
from pyoracle.curves import BLS12_381, BLS_P, BN254, BN254_P, BN254_R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
R = BN254_R
VC_OK, VC_E_INVALID, VC_E_RANGE = 0, -1, -5
SEEDS = [bytes([7]) * 32, bytes(range(32)), bytes([255 - i for i in range(32)])]


def _status(fn):
    from vkzg._lib import VCError
    with pytest.raises(VCError) as ei:
        fn()
    return ei.value.status


@pytest.fixture(scope="module")
def keys():
    from vkzg import scheme
    made = {}

    def get(N, K, curve="bn254"):
        if (N, K, curve) not in made:
            made[N, K, curve] = scheme.KZGSubvectorKey(*scheme.kzg_powers_from_secret(cases.SECRET, K, curve), N, curve)
        return made[N, K, curve]
    return get


@pytest.fixture(scope="module")
def ragged():
    """N = 8, K = 4, n = 5 with k = (1, 2, 3, 4, 1), per curve"""
    return {curve: sv.batch(8, (1, 2, 3, 4, 1), seed=11, curve=curve) for curve in ("bn254", "bls12_381")}


# ---------------------------------------------------------------- the challenge
def test_challenge_is_hash_to_field_with_its_own_tag():
    from pyoracle import arkser
    from vkzg import scheme
    for seed in SEEDS:
        assert scheme.kzg_subvector_batch_challenge(seed) == arkser.hash_to_field(seed, b"vkzg-kzg-subv-batch", R)
        assert scheme.kzg_subvector_batch_challenge(seed) != scheme.kzg_batch_challenge(seed)
        assert scheme.kzg_subvector_batch_challenge(seed, "bls12_381") == arkser.hash_to_field(
            seed, b"vkzg-kzg-subv-batch", BLS12_381.r)


# ---------------------------------------------------------------- the fold
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_fold_equals_the_integer_fold(keys, ragged, curve):
    from vkzg import scheme
    N, K = 8, 4
    key = keys(N, K, curve)
    r = cases.curve_of(curve).r
    good = ragged[curve]
    assert [len(e["S"]) for e in good] == [1, 2, 3, 4, 1] and all(sv.is_valid(N, e, curve) for e in good)
    bad = list(good)
    bad[2] = sv.tampered(good[2], "y", r)
    assert not sv.is_valid(N, bad[2], curve)
    for entries in (good, bad):
        for rho in (1, 2, scheme.kzg_subvector_batch_challenge(SEEDS[0], curve), r - 1):
            got = key.batch_fold(None, *sv.args(entries, curve), rho)
            assert got == sv.fold_points(N, entries, rho, curve), rho
            assert len(got) == 5
    # a batch of smaller sets folds into fewer points
    assert len(key.batch_fold(None, *sv.args(good[:2], curve), 3)) == 3


def test_full_domain_set_has_the_identity_proof(keys):
    N = K = 4
    key = keys(N, K)
    e = sv.entry(N, [2, 0, 3, 1], 5)
    assert e["q"] == 0 and cases.z_coeffs(N, e["S"]) == [R - 1, 0, 0, 0, 1]       # Z_S = X^4 - 1
    com, sets, ys, proofs = sv.args([e])
    assert proofs == [None]
    for rho in (1, 12345):
        assert key.batch_fold(None, com, sets, ys, proofs, rho) == sv.fold_points(N, [e], rho)
    assert key.verify_batch(None, com, sets, ys, proofs, seed=SEEDS[0]) is True
    two = [e, sv.entry(N, [1, 3], 6)]
    assert key.batch_fold(None, *sv.args(two), 77) == sv.fold_points(N, two, 77)
    assert key.verify_batch(None, *sv.args(two), seed=SEEDS[1]) is True
    assert key.verify_batch(None, *sv.args([sv.tampered(e, "y", R)]), seed=SEEDS[0]) is False


# ---------------------------------------------------------------- verdicts
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_valid_batch_accepts_and_each_tamper_is_located(keys, ragged, curve):
    N, K = 8, 4
    key = keys(N, K, curve)
    r = cases.curve_of(curve).r
    good = ragged[curve]
    for seed in SEEDS:
        assert key.verify_batch(None, *sv.args(good, curve), seed=seed) is True
    assert key.verify_batch(None, *sv.args(good, curve), seed=SEEDS[0], locate=True) == (True, [True] * 5)
    assert key.verify_batch(None, *sv.args(good, curve)) is True                   # OS entropy
    for pos, what in ((0, "y"), (3, "proof"), (4, "commitment")):
        bad = list(good)
        bad[pos] = sv.tampered(good[pos], what, r)
        want = [sv.is_valid(N, e, curve) for e in bad]
        assert want == [j != pos for j in range(5)]
        assert key.verify_batch(None, *sv.args(bad, curve), seed=SEEDS[1]) is False
        assert key.verify_batch(None, *sv.args(bad, curve), seed=SEEDS[2], locate=True) == (False, want)


def test_cancelling_errors_pass_at_rho_one_and_are_rejected(keys):
    from vkzg import scheme
    N, K = 8, 4
    key = keys(N, K)
    S = [6, 1, 4]
    a, b = sv.entry(N, S, 21), sv.entry(N, S, 22)
    t = 424242
    a2, b2 = dict(a, q=(a["q"] + t) % R), dict(b, q=(b["q"] - t) % R)
    assert not sv.is_valid(N, a2) and not sv.is_valid(N, b2)
    entries = [a2, b2]
    fold = key.batch_fold(None, *sv.args(entries), 1)              # all weights 1: the errors cancel
    assert fold == sv.fold_points(N, [a, b], 1) == sv.fold_points(N, entries, 1)
    _, g2 = scheme.kzg_powers_from_secret(cases.SECRET, K)
    assert scheme.pairing_check([(P, g2[t]) for t, P in enumerate(fold)]) is True
    seeded = key.batch_fold(None, *sv.args(entries), scheme.kzg_subvector_batch_challenge(SEEDS[0]))
    assert scheme.pairing_check([(P, g2[t]) for t, P in enumerate(seeded)]) is False
    assert key.verify_batch(None, *sv.args(entries), seed=SEEDS[0], locate=True) == (False, [False, False])
    assert key.verify_batch(None, *sv.args([a, b]), seed=SEEDS[0]) is True


def test_identity_commitments_with_identity_proofs_accept(keys):
    key = keys(8, 4)
    zero = [{"c": 0, "S": [0, 7, 3], "ys": [0, 0, 0], "q": 0}, {"c": 0, "S": [5], "ys": [0], "q": 0}]
    com, sets, ys, proofs = sv.args(zero)
    assert com == [None, None] and proofs == [None, None]
    assert key.verify_batch(None, com, sets, ys, proofs, seed=SEEDS[0], locate=True) == (True, [True, True])
    assert key.batch_fold(None, com, sets, ys, proofs, 5) == [None] * 4
    const = {"c": 12345, "S": [1, 2], "ys": [12345, 12345], "q": 0}               # a constant row
    assert sv.is_valid(8, const)
    assert key.verify_batch(None, *sv.args(zero + [const]), seed=SEEDS[1]) is True
    off = dict(zero[1], ys=[1])
    assert key.verify_batch(None, *sv.args([zero[0], off]), seed=SEEDS[1], locate=True) == (False, [True, False])


def test_n_zero_accepts(keys):
    key = keys(8, 4)
    assert key.verify_batch(None, [], [], [], [], seed=SEEDS[0]) is True
    assert key.verify_batch(None, [], [], [], [], locate=True) == (True, [])
    assert key.batch_fold(None, [], [], [], [], 3) == [None]


# ---------------------------------------------------------------- statuses, outputs untouched
def _raw(key, entries, curve="bn254"):
    from vkzg.scheme import _p
    arrs = list(key._subv_arrays(*sv.args(entries, curve)))
    return arrs, _p


def _call_both(key, arrs, n=None, rho=3, drop=None, ctx=None):
    """both calls on raw arrays -> (statuses, outputs untouched?)"""
    from vkzg import lib
    from vkzg.scheme import _fr_raw, _p
    n = len(arrs[1]) if n is None else n
    ptr = [_p(x) for x in arrs]
    if drop is not None:
        ptr[drop] = None
    kmax = ctypes.c_size_t(0xABCD)
    bad = ctypes.c_int(0xABCD)
    out = np.full((key.K + 1, 2 * key.nl), 0x5A5A, dtype=np.uint64)
    inf = np.full(key.K + 1, 0x5A, dtype=np.uint8)
    rho_arr = np.array([(int(rho) >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
    st_fold = lib().vc_kzg_subvector_batch_fold(ctx, key.h, n, *ptr, _p(rho_arr), ctypes.byref(kmax), _p(out), _p(inf),
                                                ctypes.byref(bad))
    res = ctypes.c_int(0xABCD)
    results = np.full(max(n, 1), 0x5A, dtype=np.uint8)
    seed = np.frombuffer(SEEDS[0], dtype=np.uint8).copy()
    st_ver = lib().vc_kzg_verify_subvector_batch(ctx, key.h, n, *ptr, _p(seed), ctypes.byref(res), _p(results))
    untouched = (kmax.value == 0xABCD and bad.value == 0xABCD and (out == 0x5A5A).all() and (inf == 0x5A).all()
                 and res.value == 0xABCD and (results == 0x5A).all())
    return (st_fold, st_ver), untouched


def test_every_status_leaves_the_outputs_untouched(keys, ragged):
    from vkzg import lib
    from vkzg.scheme import _p
    N, K = 8, 4
    key = keys(N, K)
    good = ragged["bn254"]
    arrs, _ = _raw(key, good)
    assert _call_both(key, arrs)[0] == (VC_OK, VC_OK)
    INV, RNG = ((VC_E_INVALID,) * 2, True), ((VC_E_RANGE,) * 2, True)

    def with_sets(sets, ys=None):
        e = [dict(g, S=S, ys=(ys[j] if ys else [0] * len(S))) for j, (g, S) in enumerate(zip(good, sets))]
        return _raw(key, e)[0]
    sets = [e["S"] for e in good]
    assert _call_both(key, with_sets(sets[:3] + [[1, 8]] + sets[4:])) == INV                   # an index >= size
    assert _call_both(key, with_sets(sets[:3] + [[1, 5, 1]] + sets[4:])) == INV                # a repeated index
    assert _call_both(key, with_sets([[0, 1, 2, 3, 4]] + sets[1:])) == RNG                     # k = K + 1
    big = keys(8, 8)
    assert _call_both(big, _raw(big, [dict(good[0], S=list(range(8)) + [0], ys=[0] * 9)])[0]) == INV   # k > size
    empty = [a.copy() for a in arrs]
    empty[2][2] = empty[2][1]                                                                  # an empty set
    assert _call_both(key, empty) == INV
    down = [a.copy() for a in arrs]
    down[2][2] = down[2][1] - 1                                                                # not monotone
    assert _call_both(key, down) == INV
    for drop in range(7):                                                                      # a null argument
        assert _call_both(key, arrs, drop=drop) == INV, drop
    # rho >= r: the fold alone takes a rho
    (st_fold, st_ver), _ = _call_both(key, arrs, rho=R)
    assert (st_fold, st_ver) == (VC_E_INVALID, VC_OK)
    assert _call_both(key, arrs, rho=R - 1)[0] == (VC_OK, VC_OK)
    # null outputs / key
    ptr = [_p(x) for x in arrs]
    res = ctypes.c_int()
    assert lib().vc_kzg_verify_subvector_batch(None, key.h, 5, *ptr, None, None, None) == VC_E_INVALID
    assert lib().vc_kzg_verify_subvector_batch(None, None, 5, *ptr, None, ctypes.byref(res), None) == VC_E_INVALID
    assert lib().vc_kzg_subvector_batch_challenge(0, None, None) == VC_E_INVALID
    out = np.zeros(4, dtype=np.uint64)
    seed = np.frombuffer(SEEDS[0], dtype=np.uint8).copy()
    assert lib().vc_kzg_subvector_batch_challenge(7, _p(seed), _p(out)) == VC_E_INVALID
    # the Python layer's own checks
    with pytest.raises(ValueError):
        key.verify_batch(None, *sv.args(good), seed=b"short")
    with pytest.raises(ValueError):
        key.verify_batch(None, [None], [[1, 2]], [[0]], [None])


# ---------------------------------------------------------------- malformed content
def test_malformed_content_is_verdict_zero_with_ok(keys, ragged):
    N, K = 8, 4
    key = keys(N, K)
    good = ragged["bn254"]
    com, sets, ys, proofs = sv.args(good)
    P = BN254_P
    pi, C = proofs[3], com[1]
    assert pi is not None and C is not None

    def swap(lst, pos, v):
        return lst[:pos] + [v] + lst[pos + 1:]
    variants = [
        (com, ys, swap(proofs, 3, (pi[0] + P, pi[1]))),                    # a coordinate >= p
        (com, ys, swap(proofs, 3, (pi[0], pi[1] + P))),
        (swap(com, 1, (C[0] + P, C[1])), ys, proofs),
        (com, ys, swap(proofs, 3, (pi[0], (pi[1] + 1) % P))),              # off the curve
        (swap(com, 1, (C[0], (C[1] + 1) % P)), ys, proofs),
        (com, swap(ys, 0, [ys[0][0] + R]), proofs),                        # y >= r, first and last entry
        (com, swap(ys, 4, [R]), proofs),
        (com, swap(ys, 3, ys[3][:3] + [2**256 - 1]), proofs),
    ]
    for c, y, p in variants:
        assert key.batch_fold(None, c, sets, y, p, 3) is None
        ok, which = key.verify_batch(None, c, sets, y, p, seed=SEEDS[0], locate=True)
        assert ok is False and which.count(False) == 1


def test_bls12_381_point_outside_the_subgroup_is_malformed(keys, ragged):
    import kzg_batch_bls_cases as bls
    curve = "bls12_381"
    key = keys(8, 4, curve)
    com, sets, ys, proofs = sv.args(ragged[curve], curve)
    T = bls.fixture()["T"]
    assert BLS12_381.is_on_curve(T) and not bls.in_subgroup(T)
    moved = proofs[:2] + [BLS12_381.add(proofs[2], T)] + proofs[3:]
    assert key.batch_fold(None, com, sets, ys, moved, 3) is None
    assert key.verify_batch(None, com, sets, ys, moved, seed=SEEDS[0], locate=True) == (False, [True, True, False, True, True])
    movedc = [BLS12_381.add(com[0], T)] + com[1:]
    assert key.batch_fold(None, movedc, sets, ys, proofs, 3) is None
    assert key.verify_batch(None, com, sets, ys, proofs[:4] + [(proofs[4][0] + BLS_P, proofs[4][1])], seed=SEEDS[0]) is False


# ---------------------------------------------------------------- the shared text under the sanitizers
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("subv") / "kzg_subv_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "kzg_subv_check.cpp"), "-o", str(exe)])
    return exe


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_shared_text_and_miller_loop_tabn_under_the_sanitizers(tmp_path, check_exe, curve):
    r = cases.curve_of(curve).r
    shapes = [(2, 1), (2, 2), (4, 4), (8, 3), (16, 15), (64, 63), (64, 64), (128, 65), (256, 64), (256, 129)]
    if curve != "bn254":
        shapes = [(2, 2), (16, 5), (128, 65)]
    lines = []
    for n_case, (N, k) in enumerate(shapes):
        S = sv.set_of(N, k, 3)
        ys = [(v * 0x9E3779B97F4A7C15 + n_case) % r for v in range(1, k + 1)]
        ys[0] = 0
        wgt = pow(12345678901234567, n_case + 1, r)
        lines.append("%d %d" % (N, k))
        lines.append(" ".join(str(i) for i in S))
        lines += ["%x" % v for v in ys] + ["%x" % wgt]
        lines += ["%x" % v for v in cases.z_coeffs(N, S, curve)]
        lines += ["%x" % (wgt * v % r) for v in cases.i_coeffs(N, S, ys, curve)]
    flat = tmp_path / "cases.txt"
    flat.write_text("%d\n" % len(shapes) + "\n".join(lines) + "\n")
    out = subprocess.check_output([str(check_exe), str(flat), curve], text=True, timeout=600)
    d = json.loads(out.splitlines()[-1])
    print(d)
    assert d["cases"] == len(shapes) and d["wrong"] == 0, d
    assert d["coeffs"] == sum(k + 3 for _, k in shapes) and d["sums"] == sum(k for _, k in shapes)
    assert d["pairing_checks"] == 16 and d["pairing_wrong"] == 0, d


# ---------------------------------------------------------------- the kernel's registers
def test_kernel_in_the_code_object_within_its_register_figures():
    """k_kzg_subv_fold, one wave per block, at 113 VGPRs on BN254 and 176 + 8 AGPRs on
    BLS12-381 (its 12-limb subgroup test), no spills; the figures of this build are the bounds."""
    sys.path.insert(0, os.path.join(ROOT, "verkle-kzg_amd", "tools"))
    import vkzg
    from kernel_regs import kernel_regs
    hit = kernel_regs(vkzg.LIB_PATH, "k_kzg_subv_fold")
    assert len(hit) == 2, hit
    bound = {"BN254Kzg": 113, "BLS381Kzg": 184}
    for name, vgpr, agpr, spills in hit:
        print(name, vgpr, agpr, spills)
        assert spills == 0, (name, spills)
        curve = next(c for c in bound if c in name)
        assert vgpr + agpr <= bound[curve], (name, vgpr, agpr)
    for name, vgpr, agpr, spills in kernel_regs(vkzg.LIB_PATH, "k_kzg_subv_sum"):
        assert spills == 0 and vgpr + agpr <= 64, (name, vgpr, agpr)

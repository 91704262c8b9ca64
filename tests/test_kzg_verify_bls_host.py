"""KZG verification on BLS12-381 through the library, without a context: no GPU. Expected values
are the oracle's (tests/kzg_batch_bls_cases.py: verdicts from protocol.KZG.verify_point with the
trapdoor, False for anything malformed, the fold in pyoracle.curves.BLS12_381 arithmetic, the
challenge from arkser.hash_to_field; [s]_2 from tests/bls12_381_g2.py). Comparisons are exact."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import bls12_381_g2 as g2
import kzg_batch_bls_cases as cases
from pyoracle import arkser
from pyoracle.curves import BLS12_381, BLS_P, BLS_R

VC_E_INVALID = -1
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def vk():
    from vkzg import scheme
    f = cases.fixture()
    return scheme.KZGVerifyingKey(f["g2"], f["size"], cases.CURVE)


@pytest.fixture(scope="module")
def rhos():
    return [arkser.hash_to_field(s, b"vkzg-kzg-batch", BLS_R) for s in cases.SEEDS]


def _invalid(fn):
    from vkzg._lib import VCError
    with pytest.raises(VCError) as ei:
        fn()
    assert ei.value.status == VC_E_INVALID


@pytest.mark.parametrize("secret", [1, 2, 100, BLS_R - 1, (1 << 200) + 12345])
def test_g2_from_secret_is_the_integer_arithmetic(secret):
    from vkzg import scheme
    assert scheme.kzg_g2_from_secret(secret, cases.CURVE) == g2.mul(g2.H, secret)
    assert cases.fixture()["g2"] == g2.mul(g2.H, cases.fixture()["secret"])


def test_key_refuses_a_malformed_g2_point():
    from vkzg import scheme
    s2 = cases.fixture()["g2"]
    scheme.KZGVerifyingKey(s2, 16, cases.CURVE)
    off = (s2[0], ((s2[1][0] + 1) % BLS_P, s2[1][1]))
    assert not g2.on_twist(off)
    outside = g2.outside_subgroup()
    assert g2.on_twist(outside) and g2.mul(outside, BLS_R) is not None
    over = ((s2[0][0] + BLS_P, s2[0][1]), s2[1])
    for bad in (off, outside, None, over):
        _invalid(lambda: scheme.KZGVerifyingKey(bad, 16, cases.CURVE))
    _invalid(lambda: scheme.KZGVerifyingKey(s2, 12, cases.CURVE))    # not a power of two
    with pytest.raises(ValueError):
        scheme.KZGVerifyingKey(s2, 16, "bandersnatch")


def test_verify_equals_the_oracle_on_every_fixture_entry(vk):
    f = cases.fixture()
    assert sum(e["valid"] for e in f["entries"]) == 18 and len(f["entries"]) > 30
    for e in f["entries"]:
        assert e["valid"] == cases.oracle_verdict(e), e["name"]
        assert vk.verify_point(e["commitment"], e["point"], e["proof"]) == e["valid"], e["name"]
    for e in cases.valid_pool():
        assert vk.verify_point(e["commitment"], e["point"], e["proof"]) is True, e["name"]


def test_malformed_and_subgroup_entries_give_verdict_zero(vk):
    names = [n for n, _ in cases.malformed_cases()]
    assert names[-3:] == ["subgroup_proof_plus_T", "subgroup_commitment_plus_T", "subgroup_R_as_proof"]
    for name, e in cases.malformed_cases():
        assert cases.oracle_verdict(e) is False
        assert vk.verify_point(e["commitment"], e["point"], e["proof"]) is False, name


def test_the_cofactor_entry_differs_from_a_valid_one_by_a_small_order_point(vk):
    """pi + T with C valid: the entry without T is accepted, so only the subgroup test stands
    between pi + T and acceptance (tests/cpp/pairing_bls_check.cpp shows it accepted without)"""
    C = BLS12_381
    T = cases.fixture()["T"]
    e = dict(cases.subgroup_cases())["subgroup_proof_plus_T"]
    pi = C.add(e["proof"]["proof"], C.neg(T))
    assert T is not None and C.is_on_curve(T) and not cases.in_subgroup(T)
    assert vk.verify_point(e["commitment"], e["point"], {"proof": pi, "y": e["proof"]["y"]}) is True
    assert vk.verify_point(e["commitment"], e["point"], e["proof"]) is False


def test_pairing_check_on_bilinear_pairs():
    from vkzg import scheme
    C = BLS12_381
    a, b = 0x1234567890abcdef1234567, BLS_R - 987654321
    aG, bH = C.mul(C.g, a), g2.mul(g2.H, b)
    assert scheme.pairing_check([(aG, bH), (C.neg(C.mul(C.g, a * b % BLS_R)), g2.H)], cases.CURVE) is True
    assert scheme.pairing_check([(aG, bH), (C.neg(C.mul(C.g, (a * b + 1) % BLS_R)), g2.H)], cases.CURVE) is False
    assert scheme.pairing_check([(aG, g2.H), (C.neg(C.g), g2.mul(g2.H, a))], cases.CURVE) is True
    assert scheme.pairing_check([(C.g, g2.H)], cases.CURVE) is False
    assert scheme.pairing_check([(None, g2.H), (C.g, None)], cases.CURVE) is True
    assert scheme.pairing_check([], cases.CURVE) is True
    T = cases.fixture()["T"]
    for bad in ([(T, g2.H)], [((C.g[0], (C.g[1] + 1) % BLS_P), g2.H)], [(C.g, g2.outside_subgroup())]):
        _invalid(lambda: scheme.pairing_check(bad, cases.CURVE))


def test_challenge_is_hash_to_field_of_the_seed(rhos):
    from vkzg import scheme
    for seed, rho in zip(cases.SEEDS, rhos):
        assert scheme.kzg_batch_challenge(seed, cases.CURVE) == rho
        assert scheme.kzg_batch_challenge(seed, "bn254") == scheme.kzg_batch_challenge(seed)


@pytest.mark.parametrize("n", [1, 2, 17, 33])
def test_host_fold_is_the_oracle_fold(vk, rhos, n):
    batch = cases.valid_batch(n)
    want = cases.oracle_fold(batch, rhos[1])
    assert cases.trapdoor_accepts(*want)
    assert vk.batch_fold(None, *cases.arrays(batch), rhos[1]) == want
    assert vk.verify_batch(None, *cases.arrays(batch), seed=cases.SEEDS[1]) is True
    other = cases.other_valid_batch(n)
    assert vk.batch_fold(None, *cases.arrays(other), rhos[2]) == cases.oracle_fold(other, rhos[2])


def test_host_batch_rejects_tampered_and_reports_malformed(vk, rhos):
    for k, e in enumerate(cases.tampered_pool()[:4]):
        batch = cases.valid_batch(9)
        batch[(2 * k + 1) % 9] = e
        got = vk.batch_fold(None, *cases.arrays(batch), rhos[0])
        assert got == cases.oracle_fold(batch, rhos[0]) and not cases.trapdoor_accepts(*got)
        assert vk.verify_batch(None, *cases.arrays(batch), seed=cases.SEEDS[0]) is False
    for name, e in cases.malformed_cases():
        batch = cases.valid_batch(5)
        batch[3] = e
        assert vk.batch_fold(None, *cases.arrays(batch), rhos[0]) is None, name
        assert vk.verify_batch(None, *cases.arrays(batch), seed=cases.SEEDS[0]) is False, name
    assert vk.verify_batch(None, [], [], []) is True
    _invalid(lambda: vk.batch_fold(None, *cases.arrays(cases.valid_batch(2)), BLS_R))


def test_fold_and_pairing_entry_under_the_sanitizers(tmp_path, rhos):
    """csrc/kzg_batch.hpp for BLS12-381 and the final pairing entry as a stand-alone program
    (tests/cpp/kzg_batch_check.cpp with the curve as its second argument, built with g++ and the
    address / undefined-behaviour sanitizers, run directly): valid batches of 1, 2 and 17, a batch
    of 5 with a tampered entry, a batch of 5 with pi + T; expected points from the oracle's fold"""
    from test_kzg_verify_batch_host import _dump
    batches = []
    for n, rho in ((1, rhos[0]), (2, rhos[1]), (17, rhos[2])):
        batch = cases.valid_batch(n)
        batches.append((batch, rho, False, True, cases.oracle_fold(batch, rho)))
    batch = cases.valid_batch(5)
    batch[3] = cases.tampered_pool()[0]
    batches.append((batch, rhos[0], False, False, cases.oracle_fold(batch, rhos[0])))
    batch = cases.valid_batch(5)
    batch[2] = dict(cases.subgroup_cases())["subgroup_proof_plus_T"]
    batches.append((batch, rhos[1], True, False, (None, None)))
    flat = tmp_path / "batches.txt"
    _dump(flat, cases.fixture(), batches)
    exe = tmp_path / "kzg_batch_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "kzg_batch_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe), str(flat), cases.CURVE], text=True, timeout=600)
    d = json.loads(out.splitlines()[-1])
    print(d)
    assert d == {"batches": 5, "wrong": 0, "accepted": 3, "rejected": 1, "malformed": 1, "pow_checks": 30}


def test_a_bn254_key_is_still_bn254_whatever_the_array_sizes():
    """the old entry points mean BN254: a key made by vc_kzg_vk_new reads 8 u64 per G1 point even
    out of arrays sized for BLS12-381 (12 u64), and takes a 16-word G2 point"""
    import kzg_batch_cases as bn
    from vkzg import scheme
    from vkzg._lib import lib
    f = bn.fixture()
    assert scheme.kzg_g2_from_secret(f["secret"]) == f["g2"] == scheme.kzg_g2_from_secret(f["secret"], "bn254")
    vk_bn = scheme.KZGVerifyingKey(f["g2"], f["size"])
    assert vk_bn.curve == "bn254" and vk_bn.nl == 4
    e = bn.valid_pool()[0]
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for words in (8, 12):
        cxy, pxy = np.zeros(words, dtype=np.uint64), np.zeros(words, dtype=np.uint64)
        cxy[:8], _ = scheme._pt_arrays([e["commitment"]])
        pxy[:8], _ = scheme._pt_arrays([e["proof"]["proof"]])
        cxy[8:] = pxy[8:] = 2**64 - 1          # (never read)
        res = ctypes.c_int(-1)
        st = lib().vc_kzg_verify(vk_bn.h, P(cxy), 0, P(scheme._fr_raw(e["point"])), P(pxy), 0,
                                 P(scheme._fr_raw(e["proof"]["y"])), ctypes.byref(res))
        assert (st, res.value) == (0, 1)
    # the raw old constructor and a BLS12-381 point: not a BN254 G2 point
    h = ctypes.c_void_p()
    xy, inf = scheme._g2_array(cases.fixture()["g2"], 6)
    assert lib().vc_kzg_vk_new(P(xy), inf, 16, ctypes.byref(h)) == VC_E_INVALID
    # each key verifies its own curve's entries only
    eb = cases.valid_pool()[0]
    assert vk_bn.verify_point(eb["commitment"], eb["point"], eb["proof"]) is False

"""IPA batch verification on the GPU (vc_ipa_verify_batch, csrc/ipa_batch.hip): one combined verdict
for n openings. Expected values are the oracle's (tests/ipa_batch_cases.py): the challenges and
verdicts recorded in tests/golden/ipa_verify_many.json, the fold S = sum_j rho^j sigma_j E_j in
pyoracle.curves.BN254 arithmetic; never the code under test's. Everything compared is an integer, a
point or a boolean: no tolerance anywhere."""
import ctypes
import random

import numpy as np
import pytest

import ipa_batch_cases as cases

pytestmark = pytest.mark.gpu
CHUNK_ENV = "VKZG_IPA_BATCH_CHUNK"  # proofs per chunk, read per call: the one knob of the batch fold
SEED = cases.SEEDS[1]


@pytest.fixture(scope="module")
def eng():
    import vkzg
    e = vkzg.Engine("bn254")
    yield e
    e.close()


@pytest.fixture(scope="module")
def ipas(eng):
    from vkzg import scheme
    return {N: scheme.IPA(eng, N, cases.crs()[:N + 1]) for N in (4, 32, 256)}


@pytest.fixture(scope="module")
def rho():
    return cases.oracle_rho(SEED)


def arrays(batch):
    from vkzg import scheme
    return ([e["commitment"] for e in batch], [e["point"] for e in batch],
            [scheme.IPAProof(list(e["l"]), list(e["r"]), e["tip"], e["y"]) for e in batch])


def prior(prefix):
    from vkzg import scheme
    if prefix is None:
        return None
    tr = scheme.TranscriptHasher("multiproof")
    for v in prefix:
        tr.append_fr(v, "t")
    return tr


# ---------------------------------------------------------------- challenges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_device_challenges_match_host_and_fixture(ipas, n):
    """a lane per proof, 64 lanes per block: the wave and block edges; tampered entries (the
    identity's encoding among them) included"""
    batch = cases.tampered_batch(n) if n > 1 else cases.tampered_pool()[3:4]
    assert n > 1 or batch[0]["name"] == "tamper_l0_identity"
    dev = ipas[32].challenges_many(*arrays(batch))
    host = ipas[32].challenges_many(*arrays(batch), device=False)
    assert dev == [(e["w"], e["x"]) for e in batch]
    assert host == dev


@pytest.mark.parametrize("N", [4, 256])
def test_device_challenges_other_sizes(ipas, N):
    batch = cases.fresh(N)
    assert ipas[N].challenges_many(*arrays(batch)) == [(e["w"], e["x"]) for e in batch]


# ---------------------------------------------------------------- fold
def _fold_matches(ipas, rho, n):
    batch = cases.tampered_batch(n)
    want = cases.oracle_fold(batch, rho)
    assert want is not None
    assert ipas[32].batch_fold(*arrays(batch), rho) == want


@pytest.mark.parametrize("n", [2, 65, 130])
def test_fold_matches_the_oracle(ipas, rho, n):
    """tampered entries at positions 0, 63, 64, n - 1: S is not the identity, so every weight counts"""
    _fold_matches(ipas, rho, n)


def test_fold_weights_continue_across_chunks(ipas, rho, monkeypatch):
    """chunks of 48: 130 proofs are 48 + 48 + 34; chunks of 1"""
    monkeypatch.setenv(CHUNK_ENV, "48")
    _fold_matches(ipas, rho, 130)
    monkeypatch.setenv(CHUNK_ENV, "1")
    _fold_matches(ipas, rho, 3)
    monkeypatch.delenv(CHUNK_ENV)


def test_fold_of_a_valid_batch_is_the_identity_and_deterministic(ipas, rho):
    batch = cases.valid_batch(7)
    assert ipas[32].batch_fold(*arrays(batch), rho) is None
    bad = cases.tampered_batch(7)
    a, b = ipas[32].batch_fold(*arrays(bad), rho), ipas[32].batch_fold(*arrays(bad), rho)
    assert a == b == cases.oracle_fold(bad, rho)


# ---------------------------------------------------------------- verdicts
@pytest.mark.parametrize("n", [1, 2, 64, 130])
def test_valid_batch_accepted(ipas, n):
    batch = cases.valid_batch(n)
    assert all(e["valid"] for e in batch)
    assert ipas[32].verify_batch(*arrays(batch), seed=SEED) is True
    assert ipas[32].verify_batch(*arrays(batch)) is True  # seed=None: OS entropy
    assert ipas[32].verify_batch(*arrays(batch), seed=SEED, locate=True) == (True, [True] * n)


@pytest.mark.parametrize("N", [256, 4])
def test_other_sizes(ipas, N):
    ents = cases.fresh(N)
    good = [e for e in ents if e["valid"]]
    assert len(good) == (2 if N == 256 else 1)
    assert ipas[N].verify_batch(*arrays(good), seed=SEED) is True
    assert ipas[N].verify_batch(*arrays(ents), seed=SEED, locate=True) == (False, [e["valid"] for e in ents])
    rho = cases.oracle_rho(SEED)
    assert ipas[N].batch_fold(*arrays(ents), rho) == cases.oracle_fold(ents, rho)


@pytest.mark.parametrize("kind", range(7))
def test_each_tamper_kind_rejected_and_located(ipas, kind):
    bad = cases.tampered_pool()[kind]
    batch = cases.valid_batch(5)
    batch[kind % 5] = bad
    assert ipas[32].verify_batch(*arrays(batch), seed=SEED) is False
    assert ipas[32].verify_batch(*arrays(batch), seed=SEED, locate=True) == (False, [e["valid"] for e in batch])


def test_same_seed_same_fold(ipas):
    from vkzg import scheme
    batch = cases.tampered_batch(5)
    rho = scheme.ipa_batch_challenge(cases.SEEDS[2])
    assert rho == cases.oracle_rho(cases.SEEDS[2])
    first = ipas[32].batch_fold(*arrays(batch), rho)
    assert first == ipas[32].batch_fold(*arrays(batch), rho) == cases.oracle_fold(batch, rho)


# ---------------------------------------------------------------- malformed entries, domain points
def test_malformed_entries(ipas, rho):
    good = cases.valid_pool()
    for i, bad in enumerate(cases.malformed_variants(good[4])):
        batch = [good[i], bad, good[i + 7]]
        assert ipas[32].batch_fold(*arrays(batch), rho) is False  # malformed
        assert ipas[32].verify_batch(*arrays(batch), seed=SEED) is False  # VC_OK with *result = 0
        assert ipas[32].verify_batch(*arrays(batch), seed=SEED, locate=True) == (False, [True, False, True])


def test_domain_elements_as_points(eng, ipas):
    """omega^3 is a domain element that is not below N: VC_E_DOMAIN for the whole call, nothing
    written; 1 = omega^0 is below N: the one-hot branch"""
    import vkzg
    from pyoracle import protocol
    from vkzg import scheme
    ipa = ipas[32]
    good = cases.valid_pool()[:3]
    com, pts, proofs = arrays(good)
    pts[1] = pow(protocol.group_gen(32), 3, scheme.R_BN254)
    with pytest.raises(vkzg.VCError) as err:
        ipa.verify_batch(com, pts, proofs, seed=SEED)
    assert err.value.status == -8
    arrs, ok = ipa._verify_many_arrays(com, pts, proofs)
    assert all(ok)
    out = np.full(3, 0xAA, dtype=np.uint8)
    res = ctypes.c_int(0x55)
    st = vkzg.lib().vc_ipa_verify_batch(eng.h, ipa.table, 32, 3, *[a.ctypes.data_as(ctypes.c_void_p) for a in arrs],
                                        None, None, ctypes.byref(res), out.ctypes.data_as(ctypes.c_void_p))
    assert st == -8 and out.tolist() == [0xAA] * 3 and res.value == 0x55
    data = scheme.LagrangeBasis([pow(11, i + 2, scheme.R_BN254) for i in range(32)])
    c = ipa.commit(data)
    pr = ipa.prove_point(c, 1, data)
    assert pr.y == data[1]
    assert ipa.verify_batch([c, c], [1, 1], [pr, pr], seed=SEED) is True
    assert ipa.verify_batch([c, c], [1, 2], [pr, pr], seed=SEED, locate=True) == (False, [True, False])


# ---------------------------------------------------------------- prior transcripts
def test_prior_transcripts(ipas):
    pre = [e for e in cases.entries() if e["prefix"] is not None]
    assert [e["valid"] for e in pre] == [True, False]
    plain = cases.valid_pool()
    ok = [plain[0], pre[0], plain[7], plain[1]]
    assert ipas[32].verify_batch(*arrays(ok), seed=SEED, transcripts=[prior(e["prefix"]) for e in ok]) is True
    mixed = [plain[0], pre[0], plain[7], pre[1], plain[1]]
    got = ipas[32].verify_batch(*arrays(mixed), seed=SEED, locate=True, transcripts=[prior(e["prefix"]) for e in mixed])
    assert got == (False, [e["valid"] for e in mixed])
    # the same openings without their prefix: a different transcript, rejected
    assert ipas[32].verify_batch(*arrays(pre[:1]), seed=SEED) is False
    assert ipas[32].verify_batch(*arrays(pre), seed=SEED, locate=True, transcripts=[None, None]) == (False, [False, False])


# ---------------------------------------------------------------- other cases
def test_round_trip_with_the_engines_prover(ipas):
    from vkzg import scheme
    ipa = ipas[32]
    rng = random.Random(5)
    datas = [scheme.LagrangeBasis([rng.randrange(scheme.R_BN254) for _ in range(32)]) for _ in range(5)]
    coms = ipa.commit_batch(datas)
    pts = [3, 40, 31, 0, 12345]
    proofs = ipa.prove_batch_points(coms, pts, datas)
    assert ipa.verify_batch(coms, pts, proofs, seed=SEED) is True
    assert ipa.verify_batch(coms[1:] + coms[:1], pts, proofs, seed=SEED) is False
    assert ipa.verify_batch([], [], []) is True  # n = 0
    assert ipa.verify_batch([], [], [], locate=True) == (True, [])


def test_other_curve_is_invalid(ipas):
    import vkzg
    e = vkzg.Engine("bls12_381")
    try:
        tid = e.random_bases(33, seed=3)
        arrs, _ = ipas[32]._verify_many_arrays(*arrays(cases.valid_batch(1)))
        res = ctypes.c_int(7)
        st = vkzg.lib().vc_ipa_verify_batch(e.h, tid, 32, 1, *[a.ctypes.data_as(ctypes.c_void_p) for a in arrs], None,
                                            None, ctypes.byref(res), None)
        assert st == -1 and res.value == 7
        out = np.zeros((1, 6, 4), dtype=np.uint64)
        a = arrs
        st = vkzg.lib().vc_ipa_challenges_many(e.h, 32, 1, *[x.ctypes.data_as(ctypes.c_void_p) for x in
                                                              (a[0], a[1], a[2], a[8], a[3], a[4], a[5], a[6])],
                                               out.ctypes.data_as(ctypes.c_void_p))
        assert st == -1
    finally:
        e.close()

"""KZG verification on BLS12-381 on the GPU: one verdict per opening (vc_kzg_verify_many ->
k_kzg_verify_bls, csrc/pairing_bls.hip) and one combined verdict (vc_kzg_verify_batch ->
csrc/kzg_batch_bls.hip) with a BLS12-381 key. Expected values are the oracle's
(tests/kzg_batch_bls_cases.py: verdicts from protocol.KZG.verify_point with the trapdoor, False for
anything malformed -- a point of E(Fq) outside the subgroup of order r included -- and the fold in
pyoracle.curves.BLS12_381 arithmetic); the host path of the fold (oracle-checked at small n in
tests/test_kzg_verify_bls_host.py) must agree point for point and is the yardstick at the sizes
where the MSM changes route. All results are points and booleans: no tolerance anywhere."""
import pytest

import kzg_batch_bls_cases as cases
from pyoracle import arkser
from pyoracle.curves import BLS_R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import vkzg
    e = vkzg.Engine("bls12_381")
    yield e
    e.close()


@pytest.fixture(scope="module")
def vk():
    from vkzg import scheme
    f = cases.fixture()
    return scheme.KZGVerifyingKey(f["g2"], f["size"], cases.CURVE)


@pytest.fixture(scope="module")
def rho():
    return arkser.hash_to_field(cases.SEEDS[1], b"vkzg-kzg-batch", BLS_R)


def _bad_pool():
    """wrong entries, malformed entries and the subgroup cases, interleaved"""
    t, m = cases.tampered_pool(), [e for _, e in cases.malformed_cases()]
    return [x for pair in zip(m, t) for x in pair]


def _bad_batch(n, shift=0):
    """the valid batch with bad entries at 0, 63, 64 and n - 1 (the ends of the first wave, the
    first lane of the second, the last lane)"""
    pool = _bad_pool()
    out = cases.valid_batch(n)
    for k, pos in enumerate(sorted({0, 63, 64, n - 1})):
        if pos < n:
            out[pos] = pool[(3 * k + n + shift) % len(pool)]
    return out


# ---------------------------------------------------------------- 4. one verdict per opening
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_verify_many_equals_the_oracle(eng, vk, n):
    for batch in (cases.valid_batch(n), _bad_batch(n)):
        want = [cases.oracle_verdict(e) for e in batch]
        assert vk.verify_many(eng, *cases.arrays(batch)) == want
    assert want[0] is False and want[-1] is False
    # the three subgroup cases (on the curve, outside G1) and one wrong entry at the same lanes
    sub = [e for _, e in cases.subgroup_cases()] + cases.tampered_pool()[:1]
    batch = cases.valid_batch(n)
    for k, pos in enumerate(sorted({0, 63, 64, n - 1})):
        if pos < n:
            batch[pos] = sub[(k + n) % 4]
    want = [i not in (0, 63, 64, n - 1) for i in range(n)]
    assert [cases.oracle_verdict(e) for e in batch] == want
    assert vk.verify_many(eng, *cases.arrays(batch)) == want


def test_verify_many_on_every_bad_entry(eng, vk):
    """every tampered, malformed and subgroup entry once, among valid ones"""
    bad = cases.tampered_pool() + [e for _, e in cases.malformed_cases()]
    batch = [x for e in bad for x in (e, cases.valid_pool()[len(e["name"]) % 21])]
    want = [cases.oracle_verdict(e) for e in batch]
    assert want == [False, True] * len(bad)
    assert vk.verify_many(eng, *cases.arrays(batch)) == want


# ---------------------------------------------------------------- 5. the fold
@pytest.mark.parametrize("n", [1, 32, 33, 63, 64, 65, 130, 257])
def test_device_fold_is_the_host_fold_is_the_oracle_fold(eng, vk, rho, n):
    batch = cases.valid_batch(n)
    want = cases.oracle_fold(batch, rho)
    assert cases.trapdoor_accepts(*want)
    assert vk.batch_fold(None, *cases.arrays(batch), rho) == want
    assert vk.batch_fold(eng, *cases.arrays(batch), rho) == want


def test_weights_continue_across_chunks(eng, vk, rho, monkeypatch):
    batch = cases.valid_batch(257)
    want = cases.oracle_fold(batch, rho)
    monkeypatch.setenv("VKZG_KZG_BATCH_CHUNK", "100")
    assert vk.batch_fold(eng, *cases.arrays(batch), rho) == want
    bad = _bad_batch(257)
    bad[0], bad[63], bad[64] = batch[0], batch[63], batch[64]     # the bad entry in the last chunk only
    assert vk.verify_batch(eng, *cases.arrays(bad), seed=cases.SEEDS[0]) is False
    assert vk.verify_batch(eng, *cases.arrays(batch), seed=cases.SEEDS[0]) is True


# ---------------------------------------------------------------- 6. the GLV crossing
@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_fold_across_the_glv_threshold_and_a_refill(vk, rho, n):
    """the 2n-point MSM takes the GLV route from n = 2048, the n-point MSM from n = 4097: the
    device fold equals the host fold and the trapdoor accepts it; then a second, different batch of
    the same n through the same context must equal its host fold -- it does not if the copies
    derived from the first batch's table outlive the refill. A context of its own, so that the
    first run is the first use of its scratch table."""
    import vkzg
    e = vkzg.Engine("bls12_381")
    try:
        for batch in (cases.valid_batch(n), cases.other_valid_batch(n)):
            a = cases.arrays(batch)
            want = vk.batch_fold(None, *a, rho)
            assert want is not None and cases.trapdoor_accepts(*want)
            assert vk.batch_fold(e, *a, rho) == want
    finally:
        e.close()


# ---------------------------------------------------------------- 7. one verdict for the batch
@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_verify_batch(eng, vk, n):
    good = cases.valid_batch(n)
    for seed in (cases.SEEDS[0], cases.SEEDS[2], None):
        assert vk.verify_batch(eng, *cases.arrays(good), seed=seed) is True
    assert vk.verify_batch(eng, *cases.arrays(good), seed=cases.SEEDS[1], locate=True) == (True, [True] * n)
    for pos in sorted({0, 63, 64, n - 1}):
        if pos >= n:
            continue
        bad = list(good)
        bad[pos] = _bad_pool()[(pos + n) % len(_bad_pool())]
        assert vk.verify_batch(eng, *cases.arrays(bad), seed=cases.SEEDS[1]) is False
    bad = _bad_batch(n)
    want = [cases.oracle_verdict(e) for e in bad]
    got = vk.verify_batch(eng, *cases.arrays(bad), seed=cases.SEEDS[1], locate=True)
    assert got == (False, want) and got[1] == vk.verify_many(eng, *cases.arrays(bad))


def test_cancelling_errors_are_rejected_under_weights(eng, vk, rho):
    for make in (cases.cancelling_y, cases.cancelling_proofs):
        batch, (a, b) = make()
        # the errors cancel in the unweighted sums ...
        assert cases.trapdoor_accepts(*cases.oracle_fold(batch, rho, unweighted=True))
        # ... and not under the weights
        got = vk.batch_fold(eng, *cases.arrays(batch), rho)
        assert got == cases.oracle_fold(batch, rho) and not cases.trapdoor_accepts(*got)
        ok, per = vk.verify_batch(eng, *cases.arrays(batch), seed=cases.SEEDS[1], locate=True)
        assert ok is False and per == [i not in (a, b) for i in range(len(batch))]


def test_subgroup_entries_make_the_fold_report_malformed(eng, vk, rho):
    for name, e in cases.malformed_cases():
        for n, pos in ((5, 3), (65, 64)):
            batch = cases.valid_batch(n)
            batch[pos] = e
            assert vk.batch_fold(eng, *cases.arrays(batch), rho) is None, name
            assert vk.verify_batch(eng, *cases.arrays(batch), seed=cases.SEEDS[0]) is False, name


def test_empty_batch_and_wrong_context(eng, vk):
    import vkzg
    from vkzg._lib import VCError
    assert vk.verify_batch(eng, [], [], []) is True
    assert vk.verify_many(eng, [], [], []) == []
    e = vkzg.Engine("bn254")
    try:
        a = cases.arrays(cases.valid_batch(2))
        for call in (lambda: vk.verify_many(e, *a), lambda: vk.verify_batch(e, *a, seed=cases.SEEDS[0]),
                     lambda: vk.batch_fold(e, *a, 5)):
            with pytest.raises(VCError) as ei:
                call()
            assert ei.value.status == -1
    finally:
        e.close()


# ---------------------------------------------------------------- 8. end to end
def test_prove_batch_points_then_verify_batch_on_a_bls12_381_engine(eng):
    from vkzg import scheme
    kz = scheme.KZG(eng, 16, secret=0x5ec2e7)
    assert kz.size == 16 and kz.verifying_key().curve == cases.CURVE
    data = scheme.LagrangeBasis([pow(5, 3 * i + 1, BLS_R) for i in range(16)], r=BLS_R)
    com = kz.commit(data)
    points = [i % 16 for i in range(40)] + [17 + 1000003 * i for i in range(24)] + [BLS_R - 2]
    assert len(points) == 65
    proofs = kz.prove_batch_points([com], points, [data], rows=[0] * 65)
    assert [pr["y"] for pr in proofs[:16]] == list(data.evals)
    coms = [com] * 65
    assert kz.verify_batch(coms, points, proofs, seed=cases.SEEDS[1]) is True
    assert kz.verify_batch(coms, points, proofs) is True
    assert kz.verify(com, 3, proofs[3]) is True
    bad = list(proofs)
    bad[41] = {"proof": proofs[41]["proof"], "y": (proofs[41]["y"] + 1) % BLS_R}
    assert kz.verify_batch(coms, points, bad, seed=cases.SEEDS[1]) is False
    assert kz.verify_batch(coms, points, bad, seed=cases.SEEDS[1], locate=True) == (False, [i != 41 for i in range(65)])
    assert kz.verify_many(coms, points, bad) == [i != 41 for i in range(65)]

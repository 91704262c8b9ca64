"""KZG batch verification on the GPU (vc_kzg_verify_batch, csrc/kzg_batch.hip): one combined
verdict for n openings. Expected values are the oracle's (tests/kzg_batch_cases.py: the fold in
pyoracle.curves.BN254 arithmetic, verdicts from protocol.KZG.verify_point); the host path of the
fold (itself oracle-checked in tests/test_kzg_verify_batch_host.py) must agree point for point.
All results are points and booleans: no tolerance anywhere."""
import pytest

import kzg_batch_cases as cases
from pyoracle import arkser
from pyoracle.curves import BN254_R

pytestmark = pytest.mark.gpu
# the wave edges (63 / 64 / 65), more than one wave per block (130), the block edge (256 / 257)
SIZES = [1, 32, 33, 63, 64, 65, 130, 257]


@pytest.fixture(scope="module")
def eng():
    import vkzg
    e = vkzg.Engine("bn254")
    yield e
    e.close()


@pytest.fixture(scope="module")
def vk():
    from vkzg import scheme
    f = cases.fixture()
    return scheme.KZGVerifyingKey(f["g2"], f["size"])


@pytest.fixture(scope="module")
def rho():
    return arkser.hash_to_field(cases.SEEDS[1], b"vkzg-kzg-batch", BN254_R)


def _tampered_batch(n):
    """the valid batch with tampered fixture entries at 0, 63, 64 and n - 1 (the ends of the first
    wave, the first lane of the second, the last lane)"""
    tampered = cases.tampered_pool()
    out = cases.valid_batch(n)
    for k, pos in enumerate(sorted({0, 63, 64, n - 1})):
        if pos < n:
            out[pos] = tampered[(3 * k + n) % len(tampered)]
    return out


@pytest.mark.parametrize("n", SIZES)
def test_device_fold_is_the_host_fold_is_the_oracle_fold(eng, vk, rho, n):
    batch = cases.valid_batch(n)
    want = cases.oracle_fold(batch, rho)
    assert cases.trapdoor_accepts(*want)
    assert vk.batch_fold(None, *cases.arrays(batch), rho) == want
    assert vk.batch_fold(eng, *cases.arrays(batch), rho) == want


@pytest.mark.parametrize("n", [1, 64, 65, 130, 257])
def test_verdicts(eng, vk, n):
    good, bad = cases.valid_batch(n), _tampered_batch(n)
    want = [cases.oracle_verdict(e) for e in bad]
    assert not want[0] and not want[n - 1] and (n == 1 or any(want))
    for seed in cases.SEEDS[:2]:
        assert vk.verify_batch(eng, *cases.arrays(good), seed=seed) is True
        assert vk.verify_batch(eng, *cases.arrays(bad), seed=seed) is False
    assert vk.verify_batch(eng, *cases.arrays(good)) is True        # a seed of the call's own
    ok, v = vk.verify_batch(eng, *cases.arrays(bad), seed=cases.SEEDS[2], locate=True)
    assert ok is False and v == want
    assert v == vk.verify_many(eng, *cases.arrays(bad))
    assert vk.verify_batch(eng, *cases.arrays(good), seed=cases.SEEDS[2], locate=True) == (True, [True] * n)


@pytest.mark.parametrize("make", [cases.cancelling_y, cases.cancelling_proofs])
def test_cancelling_pairs_across_the_wave_edge(eng, vk, rho, make):
    batch, touched = make(130, 63, 64)
    assert touched == (63, 64)
    for i in touched:
        assert cases.oracle_verdict(batch[i]) is False
    assert cases.trapdoor_accepts(*cases.oracle_fold(batch, 1, unweighted=True))
    want = cases.oracle_fold(batch, rho)
    assert not cases.trapdoor_accepts(*want)
    assert vk.batch_fold(eng, *cases.arrays(batch), rho) == want
    assert vk.verify_batch(eng, *cases.arrays(batch), seed=cases.SEEDS[1]) is False
    ok, v = vk.verify_batch(eng, *cases.arrays(batch), seed=cases.SEEDS[1], locate=True)
    assert ok is False and v == [i not in touched for i in range(130)]


def test_chunks_give_the_same_fold(eng, vk, rho, monkeypatch):
    batch = cases.valid_batch(130)
    whole = vk.batch_fold(eng, *cases.arrays(batch), rho)
    assert whole == cases.oracle_fold(batch, rho)
    monkeypatch.setenv("VKZG_KZG_BATCH_CHUNK", "64")       # 64 + 64 + 2
    assert vk.batch_fold(eng, *cases.arrays(batch), rho) == whole
    assert vk.verify_batch(eng, *cases.arrays(batch), seed=cases.SEEDS[0]) is True
    assert vk.verify_batch(eng, *cases.arrays(_tampered_batch(130)), seed=cases.SEEDS[0]) is False


def test_malformed_entries_then_a_clean_batch(eng, vk, rho):
    good = cases.valid_batch(65)
    for k, (name, e) in enumerate(cases.malformed_cases()):
        bad = list(good)
        bad[(0, 63, 64, 31, 64)[k]] = e
        want = [cases.oracle_verdict(x) for x in bad]
        assert want.count(False) == 1
        assert vk.verify_batch(eng, *cases.arrays(bad), seed=cases.SEEDS[1]) is False, name
        assert vk.batch_fold(eng, *cases.arrays(bad), rho) is None, name
        ok, v = vk.verify_batch(eng, *cases.arrays(bad), seed=cases.SEEDS[1], locate=True)
        assert ok is False and v == want, name
        assert vk.verify_batch(eng, *cases.arrays(good), seed=cases.SEEDS[1]) is True


def test_two_keys_alternate_on_one_context(eng):
    """s = 100 and s = 101 on one context: each key accepts its own 4 openings and rejects the other's"""
    from pyoracle import protocol
    from vkzg import scheme
    fx = cases.fixture()
    k100, k101 = scheme.KZG(eng, 16, secret=100), scheme.KZG(eng, 16, secret=101)
    data = scheme.LagrangeBasis(fx["data"], 16)
    pts = [0, 5, 11, 17]
    sets = {}
    for k in (k100, k101):
        com = k.commit(data)
        sets[k.secret] = (com, [k.prove_point(com, p, data) for p in pts])
    oracles = {s: protocol.KZG(16, secret=s) for s in (100, 101)}
    for _ in range(2):
        for k in (k100, k101):
            for s, (com, proofs) in sets.items():
                want = all(oracles[k.secret].verify_point(com, p, pr) for p, pr in zip(pts, proofs))
                assert want is (s == k.secret)
                assert k.verify_batch([com] * len(pts), pts, proofs, seed=cases.SEEDS[1]) is want


def test_fk_openings_of_size_256(eng):
    """every FK opening of a 256-point polynomial in one batch; with the y of entries 0, 100 and
    255 changed the batch is rejected and locate marks exactly those three"""
    from vkzg import scheme
    kzg = scheme.KZG(eng, 256)
    data = scheme.LagrangeBasis([pow(7, 3 * i + 1, scheme.R_BN254) for i in range(256)])
    com = kzg.commit(data)
    proofs = kzg.prove_all_points(data, mode=1)
    assert len(proofs) == 256 and [p["y"] for p in proofs] == list(data.evals)
    assert kzg.verify_batch([com] * 256, list(range(256)), proofs) is True
    assert kzg.verify_batch([com] * 256, list(range(256)), proofs, seed=cases.SEEDS[2], locate=True) == (True, [True] * 256)
    bad = {0, 100, 255}
    tampered = [{"proof": p["proof"], "y": (p["y"] + 1) % scheme.R_BN254} if i in bad else p
                for i, p in enumerate(proofs)]
    assert kzg.verify_batch([com] * 256, list(range(256)), tampered) is False
    assert kzg.verify_batch([com] * 256, list(range(256)), tampered, locate=True) == (False, [i not in bad for i in range(256)])

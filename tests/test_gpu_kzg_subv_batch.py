"""KZG subvector batch verification on the GPU (vc_kzg_verify_subvector_batch, csrc/kzg_subv.hip): the
device fold against the host fold of the same library point for point (the host fold is pinned to
Python integers in tests/test_kzg_subv_batch_host.py; the small shapes are compared with the integer
fold here too), verdicts against the trapdoor identity (tests/kzg_subv_cases.py). All results are
points and verdicts: no tolerance anywhere. A wave takes a run of 4 proofs at these sizes, so n = 7, 8, 9
lie around two whole runs. The chunk test forces chunks of 3 through VKZG_KZG_SUBV_CHUNK."""
import pytest

import kzg_sub_cases as cases
import kzg_subv_cases as sv
from pyoracle.curves import BLS12_381, BN254_P, BN254_R

pytestmark = pytest.mark.gpu
R = BN254_R
VC_E_INVALID, VC_E_RANGE = -1, -5
SEEDS = [bytes([7]) * 32, bytes(range(32))]


@pytest.fixture(scope="module")
def eng():
    import vkzg
    e = vkzg.Engine("bn254")
    yield e
    e.close()


@pytest.fixture(scope="module")
def keys():
    from vkzg import scheme
    made = {}

    def get(N, K, curve="bn254"):
        if (N, K, curve) not in made:
            made[N, K, curve] = scheme.KZGSubvectorKey(*scheme.kzg_powers_from_secret(cases.SECRET, K, curve), N, curve)
        return made[N, K, curve]
    return get


def _status(fn):
    from vkzg._lib import VCError
    with pytest.raises(VCError) as ei:
        fn()
    return ei.value.status


SHAPES = {
    "one": (8, 4, (3,)),
    "ragged": (8, 4, (1, 2, 3, 4, 1)),
    "lane_edges": (128, 65, (63, 64, 65)),              # the coefficient passes' lane edges
    "runs_minus_one": (16, 4, (2, 1, 4, 3, 1, 2, 4)),   # 7 = two runs of 4 less one
    "runs_exact": (16, 4, (2, 1, 4, 3, 1, 2, 4, 3)),
    "runs_plus_one": (16, 4, (2, 1, 4, 3, 1, 2, 4, 3, 2)),
    "many_partials": (16, 3, (1, 2, 3) * 23 + (1,)),    # 70 proofs, 18 waves' partials per t
    "largest_domain": (1024, 66, (2, 66)),
}


@pytest.fixture(scope="module")
def batches():
    made = {}

    def get(name):
        if name not in made:
            N, _, ks = SHAPES[name]
            made[name] = sv.batch(N, ks, seed=40 + len(ks))
        return made[name]
    return get


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_fold_equals_host_fold(eng, keys, batches, name):
    from vkzg import scheme
    N, K, ks = SHAPES[name]
    key = keys(N, K)
    entries = batches(name)
    a = sv.args(entries)
    for rho in (1, scheme.kzg_subvector_batch_challenge(SEEDS[0])):
        dev = key.batch_fold(eng, *a, rho)
        assert dev is not None and len(dev) == max(ks) + 1
        assert dev == key.batch_fold(None, *a, rho)
        if N <= 16:
            assert dev == sv.fold_points(N, entries, rho)
    assert key.verify_batch(eng, *a, seed=SEEDS[0]) is True
    # one changed y, in the last entry: the fold differs in P_H alone, the verdict is located
    bad = entries[:-1] + [sv.tampered(entries[-1], "y", R)]
    b = sv.args(bad)
    dev = key.batch_fold(eng, *b, 5)
    assert dev == key.batch_fold(None, *b, 5)
    assert dev[1:] == key.batch_fold(eng, *a, 5)[1:] and dev[0] != key.batch_fold(eng, *a, 5)[0]
    assert key.verify_batch(eng, *b, seed=SEEDS[1], locate=True) == (False, [True] * (len(ks) - 1) + [False])


def test_chunks_of_three_give_the_same_outputs(eng, keys, batches, monkeypatch):
    N, K, _ = SHAPES["runs_minus_one"]
    key = keys(N, K)
    entries = batches("runs_minus_one")
    a = sv.args(entries)
    rho = 0xC0FFEE
    whole = key.batch_fold(eng, *a, rho)
    monkeypatch.setenv("VKZG_KZG_SUBV_CHUNK", "3")          # 3 + 3 + 1
    assert key.batch_fold(eng, *a, rho) == whole == sv.fold_points(N, entries, rho)
    assert key.verify_batch(eng, *a, seed=SEEDS[0]) is True
    bad = entries[:6] + [sv.tampered(entries[6], "proof", R)]
    assert key.verify_batch(eng, *sv.args(bad), seed=SEEDS[0], locate=True) == (False, [True] * 6 + [False])
    # a malformed entry at the first and at the last position of the second chunk
    com, sets, ys, proofs = a
    for pos in (3, 5):
        off = proofs[:pos] + [(proofs[pos][0], (proofs[pos][1] + 1) % BN254_P)] + proofs[pos + 1:]
        assert key.batch_fold(eng, com, sets, ys, off, rho) is None
        assert key.verify_batch(eng, com, sets, ys, off, seed=SEEDS[0]) is False
        big_y = ys[:pos] + [[ys[pos][0] + R] + ys[pos][1:]] + ys[pos + 1:]
        assert key.batch_fold(eng, com, sets, big_y, proofs, rho) is None
    monkeypatch.delenv("VKZG_KZG_SUBV_CHUNK")
    assert key.batch_fold(eng, com, sets, ys, off, rho) is None
    assert key.batch_fold(eng, *a, rho) == whole


def test_proofs_of_the_gpu_prover_verify(eng):
    from vkzg import scheme
    N, K = 64, 8
    kz = scheme.KZG(eng, N, secret=cases.SECRET)
    key = kz.subvector_key(K)
    rows = [cases.row(N, N - 3, s) for s in (31, 32, 33)]
    datas = [scheme.LagrangeBasis(list(r), N) for r in rows]
    sets = [sv.set_of(N, 1 + j % K, j) for j in range(13)]
    row = [j % 3 for j in range(13)]
    com = [kz.commit(d) for d in datas]
    got = kz.prove_subvectors(row, sets, datas)
    coms = [com[r] for r in row]
    ys = [g["ys"] for g in got]
    proofs = [g["proof"] for g in got]
    assert key.verify_batch(eng, coms, sets, ys, proofs) is True                       # OS entropy
    assert key.verify_batch(eng, coms, sets, ys, proofs, seed=SEEDS[0], locate=True) == (True, [True] * 13)
    bad_ys = [list(v) for v in ys]
    bad_ys[8][0] = (bad_ys[8][0] + 1) % R
    assert key.verify_batch(eng, coms, sets, bad_ys, proofs, seed=SEEDS[0], locate=True) == (
        False, [j != 8 for j in range(13)])
    # a second call, the key's tables existing: the same verdicts
    assert key.verify_batch(eng, coms, sets, ys, proofs, seed=SEEDS[0]) is True
    assert key.verify_batch(eng, coms, sets, bad_ys, proofs, seed=SEEDS[0]) is False


def test_bls12_381(keys):
    import kzg_batch_bls_cases as bls
    import vkzg
    curve, N, K = "bls12_381", 16, 5
    key = keys(N, K, curve)
    entries = sv.batch(N, (5, 1, 3, 2, 4, 5), seed=60, curve=curve)
    assert all(sv.is_valid(N, e, curve) for e in entries)
    a = sv.args(entries, curve)
    e = vkzg.Engine(curve)
    try:
        rho = 0xABCDEF
        assert key.batch_fold(e, *a, rho) == key.batch_fold(None, *a, rho) == sv.fold_points(N, entries, rho, curve)
        assert key.verify_batch(e, *a, seed=SEEDS[0]) is True
        bad = entries[:2] + [sv.tampered(entries[2], "y", BLS12_381.r)] + entries[3:]
        assert key.verify_batch(e, *sv.args(bad, curve), seed=SEEDS[0], locate=True) == (
            False, [j != 2 for j in range(6)])
        T = bls.fixture()["T"]
        assert BLS12_381.is_on_curve(T) and not bls.in_subgroup(T)
        com, sets, ys, proofs = a
        moved = proofs[:4] + [BLS12_381.add(proofs[4], T)] + proofs[5:]
        assert key.batch_fold(e, com, sets, ys, moved, rho) is None
        assert key.verify_batch(e, com, sets, ys, moved, seed=SEEDS[0]) is False
        assert key.batch_fold(e, [BLS12_381.add(com[0], T)] + com[1:], sets, ys, proofs, rho) is None
    finally:
        e.close()


def test_two_keys_on_one_context(eng, keys, batches):
    k8, k16 = keys(8, 4), keys(16, 4)
    e8, e16 = batches("ragged"), batches("runs_exact")
    for _ in range(2):
        assert k8.batch_fold(eng, *sv.args(e8), 9) == sv.fold_points(8, e8, 9)
        assert k16.batch_fold(eng, *sv.args(e16), 9) == sv.fold_points(16, e16, 9)
        assert k8.verify_batch(eng, *sv.args(e8), seed=SEEDS[0]) is True
        assert k16.verify_batch(eng, *sv.args(e16), seed=SEEDS[0]) is True
    # a key of the other domain over the same statements: every index set is still good, no proof is
    assert k16.verify_batch(eng, *sv.args(e8), seed=SEEDS[0]) is False


def test_device_statuses(eng, keys, batches):
    import vkzg
    from vkzg import scheme
    key = keys(8, 4)
    a = sv.args(batches("ragged"))
    big = scheme.KZGSubvectorKey(*scheme.kzg_powers_from_secret(cases.SECRET, 2), 2048)
    one = sv.args([{"c": 0, "S": [5, 2000], "ys": [0, 0], "q": 0}])
    assert _status(lambda: big.verify_batch(eng, *one, seed=SEEDS[0])) == VC_E_RANGE       # the device's domains
    assert big.verify_batch(None, *one, seed=SEEDS[0]) is True                              # the host takes it
    com, sets, ys, proofs = a
    assert _status(lambda: key.verify_batch(eng, com, [[0, 0]] + sets[1:], [[1, 1]] + ys[1:], proofs)) == VC_E_INVALID
    assert _status(lambda: key.batch_fold(eng, *a, R)) == VC_E_INVALID
    other = vkzg.Engine("bls12_381")
    try:
        assert _status(lambda: key.verify_batch(other, *a, seed=SEEDS[0])) == VC_E_INVALID  # not the key's curve
    finally:
        other.close()
    assert key.verify_batch(eng, [], [], [], [], locate=True) == (True, [])

"""GPU parity of the accumulate's bucket bounds: the thread-start records the fine sort writes
(msm_accumulate.hpp AccStart, msm_sort.hpp k_sort_fine), the next bucket's end loaded one bucket ahead inside the loop, the entry
index loaded two entries ahead and the chain lengths taken from the records -- against the C
oracle's group law, bit-exact, as tests/test_gpu_msm.py does.

VKZG_MSM_M (sorted entries per accumulate thread, read on every call) is set to 4 and 16, so a few
hundred terms cross hundreds of thread boundaries: thread starts inside a bucket, at a bucket's
first entry, after runs of empty buckets, across the boundary of two bucket sets (offsets[]
concatenates them), an entry count that is no multiple of M, one bucket spanning every thread (the
long-chain host path) and a set whose only used bucket is its last one.

The engine takes the shared-window path (all windows into one bucket set) only for a whole
BLS12-381 table of >= 4096 points (the GLV split); below that a BLS12-381 MSM runs per-window
bucket sets. Every slice_enqueue caller gets the records, so the small cases below run the new
code on per-window sets, and the n = 4099 cases run it on the shared-window set (the plan is
asserted). The 5 x 2^15-bucket radix geometry (>= 2^18 points, lane-per-owner fix-up) is covered
at its own size by tests/test_gpu_fullsize.py."""
import numpy as np
import pytest

from test_gpu_msm import _oracle, engines  # noqa: F401  (engines: module-scoped fixture)

pytestmark = pytest.mark.gpu

MS = [4, 16]


def _device(sc):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(sc).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return d


def _check(e, oracle_c, curve, tid, xy, inf, sc, offset=0):
    n = len(sc)
    d = _device(sc)
    got = e.msm_device(tid, d.data_ptr(), n, offset=offset)
    want = _oracle(oracle_c, curve, xy[offset:offset + n], inf[offset:offset + n], sc)
    assert got[1] == want[1]
    assert want[1] or np.array_equal(got[0], want[0])


def _with_identities(e, tid, every):
    xy, inf = e.download_bases(tid)
    inf = inf.copy()
    inf[::every] = 1
    return e.upload_bases(xy, inf), xy, inf


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("case", ["n1", "n2_equal", "n300_random", "n300_all_equal", "n300_top_bucket",
                                  "n257_identity_zero"])
def test_bounds_bls12_381_small(engines, oracle_c, monkeypatch, case, M):
    import vkzg
    curve = "bls12_381"
    e = engines[curve]
    r = vkzg.SCALAR_R[curve]
    n = {"n1": 1, "n2_equal": 2, "n257_identity_zero": 257}.get(case, 300)
    rng = np.random.default_rng(7000 + n)
    tid = e.random_bases(n, seed=700 + n)
    xy, inf = e.download_bases(tid)
    sc = vkzg.random_scalars(curve, n, rng)
    if case in ("n2_equal", "n300_all_equal"):
        sc = np.repeat(sc[:1], n, axis=0)
    elif case == "n257_identity_zero":
        tid, xy, inf = _with_identities(e, tid, 3)
        sc = sc.copy()
        sc[::5] = 0
    monkeypatch.setenv("VKZG_MSM_M", str(M))
    if case == "n300_top_bucket":
        # the plan's window size c: the digit 2^(c-1) stays positive in the signed recoding (raw >
        # half goes negative), i.e. bucket 2^(c-1) - 1, the last of its window's set
        e.msm_device(tid, _device(sc).data_ptr(), n)
        plan = e.msm_last_plan()
        c = plan["window_bits"]
        assert plan["radix_mul"] == 1 and not plan["shared_windows"]
        s = sum(1 << (c - 1 + c * w) for w in range(250 // c))
        assert s < r
        sc = vkzg.ints_to_limbs([s] * n)
    _check(e, oracle_c, curve, tid, xy, inf, sc)
    assert not e.msm_last_plan()["shared_windows"]


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("case", ["random", "all_equal", "identity_zero"])
def test_bounds_bls12_381_shared_windows(engines, oracle_c, monkeypatch, case, M):
    """a whole table of 4099 points: the GLV split's 8198 terms, every window into one bucket set
    through the window copies (entry count no multiple of M, most thread starts inside a bucket;
    all_equal: one bucket per window holds a whole window's entries, chains far beyond the walk)"""
    import vkzg
    curve = "bls12_381"
    e = engines[curve]
    n = 4099
    rng = np.random.default_rng(8000 + M)
    tid = e.random_bases(n, seed=811)
    xy, inf = e.download_bases(tid)
    sc = vkzg.random_scalars(curve, n, rng)
    if case == "all_equal":
        sc = np.repeat(sc[:1], n, axis=0)
    elif case == "identity_zero":
        tid, xy, inf = _with_identities(e, tid, 3)
        sc = sc.copy()
        sc[::5] = 0
    monkeypatch.setenv("VKZG_MSM_M", str(M))
    _check(e, oracle_c, curve, tid, xy, inf, sc)
    assert e.msm_last_plan()["shared_windows"]


@pytest.mark.parametrize("M", MS)
def test_bounds_point_range(engines, oracle_c, monkeypatch, M):
    """[off, off + n) with off > 0 of a 300-point table, n = 200"""
    import vkzg
    curve = "bls12_381"
    e = engines[curve]
    tid = e.random_bases(300, seed=912)
    xy, inf = e.download_bases(tid)
    sc = vkzg.random_scalars(curve, 200, np.random.default_rng(913))
    monkeypatch.setenv("VKZG_MSM_M", str(M))
    _check(e, oracle_c, curve, tid, xy, inf, sc, offset=37)


@pytest.mark.parametrize("M", MS)
def test_bounds_two_sets(engines, oracle_c, monkeypatch, M):
    """vc_msm_device_many, K = 2, n = 200: each set against the oracle"""
    import vkzg
    curve = "bls12_381"
    e = engines[curve]
    n = 200
    tid = e.random_bases(n, seed=921)
    xy, inf = e.download_bases(tid)
    rng = np.random.default_rng(922)
    sets = [vkzg.random_scalars(curve, n, rng) for _ in range(2)]
    d = [_device(s) for s in sets]
    monkeypatch.setenv("VKZG_MSM_M", str(M))
    got = e.msm_device_many(tid, [x.data_ptr() for x in d], n)
    for k in range(2):
        want = _oracle(oracle_c, curve, xy, inf, sets[k])
        assert got[k][1] == want[1] and np.array_equal(got[k][0], want[0]), k


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("curve", ["bn254", "bandersnatch"])
def test_bounds_per_window_curves(engines, oracle_c, monkeypatch, curve, M):
    import vkzg
    e = engines[curve]
    n = 500
    tid = e.random_bases(n, seed=931)
    xy, inf = e.download_bases(tid)
    sc = vkzg.random_scalars(curve, n, np.random.default_rng(932))
    monkeypatch.setenv("VKZG_MSM_M", str(M))
    _check(e, oracle_c, curve, tid, xy, inf, sc)

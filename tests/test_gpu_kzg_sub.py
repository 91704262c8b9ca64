"""KZG subvector proofs on the GPU (vc_kzg_prove_subvector_many, csrc/kzg_sub.hip): n index sets in
one call, one constant-size proof each. Expected values are the helper's (tests/kzg_sub_cases.py: the
trapdoor proof ((f(s) - I(s)) / Z_S(s)) G in Python integers and the oracle's curves, pinned against
protocol.KZG in tests/test_kzg_sub_host.py), the single call's (vc_kzg_prove) and the weighted sum of
vc_kzg_prove_many's proofs. All results are points and field elements: no tolerance anywhere.
The chunk test forces small chunks through VKZG_KZG_PROVE_CHUNK, the hook vc_kzg_prove_many has."""
import ctypes
import random

import numpy as np
import pytest

import kzg_sub_cases as cases
from pyoracle.curves import BLS12_381, BN254, BN254_R

pytestmark = pytest.mark.gpu
R = BN254_R
VC_E_INVALID, VC_E_TABLE, VC_E_RANGE = -1, -4, -5
POISON = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def eng():
    import vkzg
    e = vkzg.Engine("bn254")
    yield e
    e.close()


@pytest.fixture(scope="module")
def kzgs(eng):
    """N -> scheme.KZG with 8-bit fixed-base window tables, made on demand; N = 2 keeps none, so its
    calls build the table on first use, as vc_msm_batch does"""
    from vkzg import scheme
    made = {}

    def get(N):
        if N not in made:
            made[N] = scheme.KZG(eng, N, secret=cases.SECRET)
            if N != 2:
                eng.fixed_base_precompute(made[N].table, 8)
        return made[N]
    return get


def _lb(evals, N, r=R):
    from vkzg import scheme
    return scheme.LagrangeBasis(list(evals), N, r=r)


def _limbs(vals):
    import vkzg
    return np.ascontiguousarray(vkzg.ints_to_limbs([int(v) for v in vals], 4))


def _flat(sets):
    off = np.zeros(len(sets) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(s) for s in sets])
    idx = np.array([i for s in sets for i in s] or [0], dtype=np.uint32)
    return off, idx


def _raw(eng, table, N, rows, width, data, row, off, idx, n, fn="vc_kzg_prove_subvector_many", nl=8, data_ptr=None,
         drop=(), total=None):
    """the C call with poisoned outputs -> (status, proof_xy, proof_inf, y); drop: arguments passed as NULL"""
    from vkzg._lib import lib
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
    total = len(idx) if total is None else total
    pxy = np.full((max(n, 1), nl), POISON, dtype=np.uint64)
    pinf = np.full(max(n, 1), 0xA5, dtype=np.uint8)
    y = np.full((max(total, 1), 4), POISON, dtype=np.uint64)
    st = getattr(lib(), fn)(eng.h, table, N, rows, width, ctypes.c_void_p(data_ptr) if data_ptr else P(data), P(row),
                            None if "idx_off" in drop else P(off), None if "idx" in drop else P(idx), n,
                            None if "proof_xy" in drop else P(pxy), None if "proof_inf" in drop else P(pinf),
                            None if "y" in drop else P(y))
    return st, pxy, pinf, y


def _untouched(out):
    _, pxy, pinf, y = out
    return bool((pxy == POISON).all() and (pinf == 0xA5).all() and (y == POISON).all())


def _mixed(N, width):
    """three rows and the standard sets over them, two passes: several sets share a row, and the
    rows change from wave to wave"""
    rows = [cases.row(N, width, s) for s in (21, 22, 23)]
    sets = cases.standard_sets(N, width)
    sets = sets + [list(reversed(s)) for s in sets[:3]]
    row = [(3 * t + t // 2) % 3 for t in range(len(sets))]
    return rows, sets, row


# ---------------------------------------------------------------- 1. the helper, by width
@pytest.mark.parametrize("N", [2, 16, 64, 128, 256])
def test_widths_against_the_helper(kzgs, N):
    kz = kzgs(N)
    width = N - 3 if N > 4 else 1
    rows, sets, row = _mixed(N, width)
    ks = {len(s) for s in sets}
    assert {1, N - 1, N} <= ks and (N < 128 or {2, 3, 63, 64, 65} <= ks)
    assert any(0 in s and N - 1 in s for s in sets) and list(range(width, N)) in sets
    assert len(set(row)) == 3 and len(row) > 3
    got = kz.prove_subvectors(row, sets, [_lb(r, N) for r in rows])
    want = [cases.expected(N, rows[r], s) for r, s in zip(row, sets)]
    assert got == want
    for g, s in zip(got, sets):
        assert (g["proof"] is None) == (len(s) == N)
    assert all(y == 0 for y in got[sets.index(list(range(width, N)))]["ys"])


def test_width_1024(kzgs):
    N, width = 1024, 1021
    kz = kzgs(N)
    evals = cases.row(N, width, 5)
    rng = random.Random(1024)
    sets = [[1023], rng.sample(range(N), 65), [0, 1023] + rng.sample(range(1, 1023), 298)]
    got = kz.prove_subvectors([0, 0, 0], sets, [_lb(evals, N)])
    assert got == [cases.expected(N, evals, s) for s in sets]


# ---------------------------------------------------------------- 2. the identities
def test_one_index_is_the_single_call_and_all_indices_give_the_identity(eng, kzgs):
    N, width = 64, 61
    kz = kzgs(N)
    evals = cases.row(N, width, 6)
    data = _lb(evals, N)
    singles = [0, 5, 60, 61, 63]
    full = list(range(N))
    random.Random(6).shuffle(full)
    sets = [[i] for i in singles] + [list(range(N)), full]
    got = kz.prove_subvectors([0] * len(sets), sets, [data])
    for i, g in zip(singles, got):
        one = kz.prove_point(None, i, data)
        assert g == {"proof": one["proof"], "ys": [one["y"]]} and one["proof"] is not None
    off, idx = _flat(sets)
    st, pxy, pinf, y = _raw(eng, kz.table, N, 1, width, _limbs(evals), np.zeros(len(sets), dtype=np.uint32), off, idx,
                            len(sets))
    assert st == 0 and pinf.tolist() == [0] * 5 + [1, 1]
    assert got[5] == {"proof": None, "ys": [cases.value(evals, i) for i in range(N)]}
    assert got[6] == {"proof": None, "ys": [cases.value(evals, i) for i in full]}


def test_a_permuted_subset_gives_the_same_proof_and_permuted_ys(kzgs):
    N = 256
    kz = kzgs(N)
    evals = cases.row(N, 253, 7)
    S = random.Random(9).sample(range(N), 70)
    perm = list(range(70))
    random.Random(10).shuffle(perm)
    a, b, c = kz.prove_subvectors([0, 0, 0], [S, [S[p] for p in perm], sorted(S)], [_lb(evals, N)])
    assert a == cases.expected(N, evals, S)
    assert b["proof"] == a["proof"] == c["proof"]
    assert b["ys"] == [a["ys"][p] for p in perm] and c["ys"] == [cases.value(evals, i) for i in sorted(S)]


@pytest.mark.parametrize("k", [5, 64])
def test_aggregation_of_single_proofs(kzgs, k):
    """pi_S = sum c_i pi_i: the weights from vc_kzg_subvector_weights, the single proofs from
    vc_kzg_prove_many, the sum in the oracle's curve arithmetic"""
    from vkzg import scheme
    N = 64
    kz = kzgs(N)
    evals = cases.row(N, 61, 8)
    data = _lb(evals, N)
    S = random.Random(k).sample(range(N), k)
    singles = kz.prove_batch_points(None, S, [data], rows=[0] * k)
    c = scheme.kzg_subvector_weights(N, S)
    assert c == cases.weights(N, S)
    got = kz.prove_subvector(None, S, data)
    assert got["ys"] == [p["y"] for p in singles]
    assert got["proof"] == BN254.msm([p["proof"] for p in singles], c)
    assert (got["proof"] is None) == (k == N)


# ---------------------------------------------------------------- 3. chunks, the device form, row == NULL
def _seven(N=256, width=253):
    rows = [cases.row(N, width, s) for s in (31, 32)]
    rng = random.Random(7)
    sets = [rng.sample(range(N), k) for k in (1, 4, 65, 2, 256, 17, 3)]
    return rows, sets, [0, 1, 1, 0, 1, 0, 0]


def test_chunks_give_the_same_outputs(eng, kzgs, monkeypatch):
    kz = kzgs(256)
    rows, sets, row = _seven()
    ev = _limbs([v for r in rows for v in r])
    off, idx = _flat(sets)
    args = (eng, kz.table, 256, 2, 253, ev, np.array(row, dtype=np.uint32), off, idx, 7)
    whole = _raw(*args)
    assert whole[0] == 0
    monkeypatch.setenv("VKZG_KZG_PROVE_CHUNK", "3")        # 3 + 3 + 1
    parts = _raw(*args)
    assert parts[0] == 0
    for a, b in zip(whole[1:], parts[1:]):
        assert np.array_equal(a, b)
    got = kz.prove_subvectors(row, sets, [_lb(r, 256) for r in rows])
    assert got == [cases.expected(256, rows[r], s) for r, s in zip(row, sets)]
    # row == NULL under chunks: chunk c starts at row 3 c
    per_set = [_lb(rows[r], 256) for r in row]
    assert kz.prove_subvectors(None, sets, per_set) == got


def test_device_rows_equal_host_rows_and_row_null(eng, kzgs):
    import torch
    kz = kzgs(256)
    rows, sets, row = _seven()
    ev = _limbs([v for r in rows for v in r])
    off, idx = _flat(sets)
    rowa = np.array(row, dtype=np.uint32)
    host = _raw(eng, kz.table, 256, 2, 253, ev, rowa, off, idx, 7)
    d_ev = torch.from_numpy(ev.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    dev = _raw(eng, kz.table, 256, 2, 253, None, rowa, off, idx, 7, fn="vc_kzg_prove_subvector_many_device",
               data_ptr=d_ev.data_ptr())
    assert host[0] == 0 and dev[0] == 0
    for a, b in zip(host[1:], dev[1:]):
        assert np.array_equal(a, b)
    assert np.array_equal(d_ev.cpu().numpy().view(np.uint64), ev)       # the caller's rows are not written
    ev7 = _limbs([v for r in row for v in rows[r]])                     # one row per set
    null = _raw(eng, kz.table, 256, 7, 253, ev7, None, off, idx, 7)
    assert null[0] == 0
    for a, b in zip(host[1:], null[1:]):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 4. BLS12-381
@pytest.mark.parametrize("N", [16, 256])
def test_bls12_381_against_the_helper(N):
    import vkzg
    from vkzg import scheme
    curve = "bls12_381"
    e = vkzg.Engine(curve)
    try:
        kz = scheme.KZG(e, N, secret=cases.SECRET)
        e.fixed_base_precompute(kz.table, 8)
        width = N - 3
        evals = cases.row(N, width, 9, curve)
        rng = random.Random(381 + N)
        sets = [[N - 1], [0, N - 1] + rng.sample(range(1, N - 1), 3), rng.sample(range(N), min(64, N))]
        got = kz.prove_subvectors([0, 0, 0], sets, [_lb(evals, N, BLS12_381.r)])
        want = [cases.expected(N, evals, s, curve) for s in sets]
        assert got == want
        assert all((g["proof"] is None) == (len(s) == N) for g, s in zip(got, sets))
        assert got[0]["ys"] == [0]
    finally:
        e.close()


# ---------------------------------------------------------------- 5. arguments
def test_each_bad_status_leaves_the_outputs_untouched(eng, kzgs):
    kz = kzgs(256)
    N, width = 256, 253
    rows = [cases.row(N, width, 41), cases.row(N, width, 42)]
    ev = _limbs(rows[0] + rows[1])
    sets = [[3, 200, 255], [7], [9, 8]]
    off, idx = _flat(sets)
    row = np.array([0, 1, 1], dtype=np.uint32)

    def call(**kw):
        a = dict(table=kz.table, N=N, rows=2, width=width, data=ev, row=row, off=off, idx=idx, n=3)
        a.update(kw)
        return _raw(eng, a["table"], a["N"], a["rows"], a["width"], a["data"], a["row"], a["off"], a["idx"], a["n"],
                    drop=a.get("drop", ()), total=6)

    from vkzg.scheme import _pt
    from vkzg.engine import limbs_to_int
    st, pxy, pinf, y = call()
    assert st == 0
    want = [cases.expected(N, rows[r], s) for r, s in zip(row, sets)]
    assert [_pt(pxy[i], pinf[i]) for i in range(3)] == [w["proof"] for w in want]
    assert [limbs_to_int(y[p]) for p in range(6)] == [v for w in want for v in w["ys"]]
    u32 = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    invalid = [dict(N=255), dict(N=1), dict(N=0), dict(N=2048), dict(width=257), dict(data=None),
               dict(drop=("idx_off",)), dict(drop=("idx",)), dict(drop=("proof_xy",)), dict(drop=("proof_inf",)),
               dict(drop=("y",)),
               dict(row=None),                              # rows (2) != n (3)
               dict(row=u32(0, 2, 1)),                      # a row index >= rows
               dict(idx=u32(3, 200, 256, 7, 9, 8)),         # an index >= N
               dict(idx=u32(3, 200, 3, 7, 9, 8)),           # a repeated index inside one subset
               dict(off=u32(0, 3, 3, 6)),                   # an empty subset
               dict(off=u32(0, 4, 3, 6)),                   # idx_off not monotone
               dict(idx=u32(*range(300)), off=u32(0, 257, 258, 260))]    # more than N indices
    for kw in invalid:
        out = call(**kw)
        assert out[0] == VC_E_INVALID and _untouched(out), list(kw.items())[0][0]
    out = call(idx=u32(3, 200, 255, 7, 9, 7), off=u32(0, 3, 4, 6))       # the same index in two subsets is fine
    assert out[0] == 0
    out = call(table=kzgs(16).table)                        # the table has 16 points
    assert out[0] == VC_E_RANGE and _untouched(out)
    out = call(table=9999)
    assert out[0] == VC_E_TABLE and _untouched(out)
    out = call(n=0)
    assert out[0] == 0 and _untouched(out)
    out = call(n=0, data=None, row=None, drop=("idx_off", "idx"))
    assert out[0] == 0 and _untouched(out)
    assert kz.prove_subvectors(None, [], []) == []
    assert call()[0] == 0                                   # and the context still proves


# ---------------------------------------------------------------- 6. the key from the SRS, end to end
def test_g1_powers_are_the_powers_of_the_secret(kzgs):
    kz = kzgs(16)
    assert kz.g1_powers(16) == [BN254.mul(BN254.g, pow(cases.SECRET, t, R)) for t in range(16)]
    from vkzg._lib import VCError
    with pytest.raises(VCError) as err:
        kz.g1_powers(17)
    assert err.value.status == VC_E_RANGE


def test_gpu_proofs_verify_and_a_changed_y_is_rejected(kzgs):
    N, K = 256, 16
    kz = kzgs(N)
    key = kz.subvector_key(K)
    assert key.K == K and key.size == N
    rows = [cases.row(N, 253, s) for s in (51, 52)]
    datas = [_lb(r, N) for r in rows]
    coms = [kz.commit(d) for d in datas]
    rng = random.Random(51)
    sets = [[255], [0, 255, 100, 254, 7], rng.sample(range(N), 16), rng.sample(range(N), 16)]
    row = [0, 1, 1, 0]
    proofs = kz.prove_subvectors(row, sets, datas)
    for r, s, pr in zip(row, sets, proofs):
        assert key.verify(coms[r], s, pr["ys"], pr["proof"]) is True
        assert key.verify(coms[1 - r], s, pr["ys"], pr["proof"]) is False
        bad = list(pr["ys"])
        bad[len(s) // 2] = (bad[len(s) // 2] + 1) % R
        assert key.verify(coms[r], s, bad, pr["proof"]) is False

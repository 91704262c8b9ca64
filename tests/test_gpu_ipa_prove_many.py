"""IPA batch proving on the GPU (vc_ipa_prove_many, csrc/ipa_many.hip): n openings in one call, the
whole proof made on the device. Expected values are the golden file's, the oracle's
(tests/ipa_prove_cases.py: pyoracle.protocol.IPA.prove_point, N <= 32) and the single call's
(vc_ipa_prove). All results are points and field elements: no tolerance anywhere.

r - 1 is -1 = w^(N / 2), an element of every domain of even size, where the reference divides by
zero, so it belongs to the points that make the whole call fail with VC_E_DOMAIN; r - 2 stands
beside it as the large point that opens."""
import ctypes
import random

import numpy as np
import pytest

import ipa_prove_cases as cases

pytestmark = pytest.mark.gpu
R = cases.R
VC_E_INVALID, VC_E_TABLE, VC_E_DOMAIN = -1, -4, -8
POISON = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def eng():
    import vkzg
    e = vkzg.Engine("bn254")
    yield e
    e.close()


@pytest.fixture(scope="module")
def ipas(eng):
    """N -> scheme.IPA over the fixture's CRS with 8-bit fixed-base window tables, made on demand;
    N = 2 keeps none, so its calls build the table on first use, as vc_msm_batch does"""
    from vkzg import scheme
    made = {}

    def get(N):
        if N not in made:
            made[N] = scheme.IPA(eng, N, cases.crs()[:N + 1])
            if N != 2:
                eng.fixed_base_precompute(made[N].table, 8)
        return made[N]
    return get


def _lb(evals):
    from vkzg import scheme
    return scheme.LagrangeBasis(list(evals))


def _limbs(vals):
    import vkzg
    return np.ascontiguousarray(vkzg.ints_to_limbs([int(v) for v in vals], 4))


def _P(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _raw(eng, table, N, rows, data, row, com, cinf, points, n, fn="vc_ipa_prove_many", data_ptr=None, drop=()):
    """the C call with poisoned outputs -> (status, l_xy, l_inf, r_xy, r_inf, tip, y); drop: outputs
    passed as NULL"""
    from vkzg._lib import lib
    K = max(N, 2).bit_length() - 1
    m = max(n, 1)
    outs = {"l_xy": np.full((m * K, 8), POISON, dtype=np.uint64), "l_inf": np.full(m * K, 0xA5, dtype=np.uint8),
            "r_xy": np.full((m * K, 8), POISON, dtype=np.uint64), "r_inf": np.full(m * K, 0xA5, dtype=np.uint8),
            "tip": np.full((m, 4), POISON, dtype=np.uint64), "y": np.full((m, 4), POISON, dtype=np.uint64)}
    st = getattr(lib(), fn)(eng.h, table, N, rows, ctypes.c_void_p(data_ptr) if data_ptr else _P(data), _P(row), _P(com),
                            _P(cinf), _P(points), n, *[None if k in drop else _P(a) for k, a in outs.items()])
    return (st,) + tuple(outs.values())


def _untouched(out):
    return all(bool((a == (0xA5 if a.dtype == np.uint8 else POISON)).all()) for a in out[1:])


def _dicts(proofs):
    return [p.as_dict() for p in proofs]


# ---------------------------------------------------------------- 1. the golden
def test_golden_openings_as_one_batch(ipas):
    data, com, want = cases.golden256()
    got = ipas(256).prove_many([com], [w["point"] for w in want], [_lb(data)], rows=[0, 0])
    assert [w["point"] for w in want] == [77, 1000]              # in the domain, outside it
    for g, w in zip(got, want):
        assert g.l == w["l"] and g.r == w["r"] and g.tip == w["tip"] and g.y == w["y"]


# ---------------------------------------------------------------- 2. the oracle, by width
@pytest.mark.parametrize("N", [2, 4, 32])     # K = 1: only the 'w' label precedes; K = 2: the first 'x' label
def test_widths_against_the_oracle_and_the_single_call(ipas, N):
    ipa = ipas(N)
    evals = cases.row(N, 1)
    data, com = _lb(evals), cases.commitment(N, evals)
    points = cases.standard_points(N)
    assert points[:5] == [0, N - 1, N // 2 if N > 2 else 1, N + 1, R - 2] and len(points) == 6
    want = [cases.expected(N, evals, p) for p in points]
    got = ipa.prove_many([com], points, [data], rows=[0] * 6)
    assert _dicts(got) == want
    assert _dicts(got) == [ipa.prove_point(com, p, data).as_dict() for p in points]
    assert ipa.commit(data) == com
    # one row per opening (row == NULL), the same rows
    assert _dicts(ipa.prove_many([com] * 6, points, [data] * 6)) == want


# ---------------------------------------------------------------- 3. single-call parity at N = 256
@pytest.fixture(scope="module")
def pool256(ipas):
    """3 data rows with their commitments; 20 (row, point) pairs in the domain, 20 outside"""
    N = 256
    rows = [cases.row(N, s) for s in (11, 12, 13)]
    datas = [_lb(r) for r in rows]
    coms = ipas(N).commit_batch(datas)
    rng = random.Random(256)
    inside = [0, 1, 63, 64, 65, 127, 128, 191, 192, 253, 254, 255] + rng.sample(range(2, 250), 8)
    outside = [N, N + 1, N + 7, R - 2, 1 << 64, (1 << 64) + 5] + [rng.randrange(N + 8, R) for _ in range(14)]
    return datas, coms, [(k % 3, p) for k, p in enumerate(inside)], [(k % 3, p) for k, p in enumerate(outside)]


def _batch256(pool, kind, n):
    datas, coms, pin, pout = pool
    if kind == "inside":
        pairs = [pin[(i + i // 20) % 20] for i in range(n)]
    elif kind == "outside":
        pairs = [pout[(i + i // 20) % 20] for i in range(n)]
    else:  # alternating: the branch changes from wave to wave
        pairs = [(pin if i % 2 == 0 else pout)[(i // 2 + i // 40) % 20] for i in range(n)]
    return pairs


@pytest.mark.parametrize("kind", ["inside", "outside", "alternating"])
@pytest.mark.parametrize("n", [1, 3, 64, 65, 257])
def test_single_call_parity(eng, ipas, pool256, kind, n):
    ipa = ipas(256)
    datas, coms, _, _ = pool256
    pairs = _batch256(pool256, kind, n)
    points, rows = [p for _, p in pairs], [r for r, _ in pairs]
    want = ipa.prove_batch_points([coms[r] for r in rows], points, [datas[r] for r in rows])
    eng.enable_timing(True)
    try:
        eng.reset_timing()
        got = ipa.prove_many(coms, points, datas, rows=rows)
        counts = [eng.kernel_time(k)[1] for k in ("ipa_many_init", "ipa_many_round", "ipa_many_finish")]
    finally:
        eng.enable_timing(False)
    assert _dicts(got) == _dicts(want)
    assert counts == [1, 8, 1]                                   # K = 8 rounds, no launch per opening


# ---------------------------------------------------------------- 4. degenerate rows
def test_degenerate_rows(ipas):
    N = 32
    ipa = ipas(N)
    m = N - 1
    zero, const = (0,) * N, (12345,) * N
    single = tuple(777 if i == m else 0 for i in range(N))
    rows3 = (zero, const, single)
    datas = [_lb(r) for r in rows3]
    coms = [None, cases.commitment(N, const), cases.commitment(N, single)]
    assert cases.commitment(N, zero) is None
    points = [0, N + 5, 1, N + 9, m, N + 3]
    rows = [0, 0, 1, 1, 2, 2]
    got = _dicts(ipa.prove_many(coms, points, datas, rows=rows))
    # the all-zero row: every L_k, R_k is the identity (its transcript encoding), tip = y = 0
    for g in got[:2]:
        assert g == {"l": [None] * 5, "r": [None] * 5, "tip": 0, "y": 0}
    assert got == [cases.expected(N, rows3[r], p, coms[r]) for p, r in zip(points, rows)]
    assert got == [ipa.prove_point(coms[r], p, datas[r]).as_dict() for p, r in zip(points, rows)]
    assert got[2]["y"] == 12345 and got[4]["y"] == 777


# ---------------------------------------------------------------- 5. chunks
def test_chunks_give_the_same_proofs(ipas, pool256, monkeypatch):
    ipa = ipas(256)
    datas, coms, _, _ = pool256
    pairs = _batch256(pool256, "alternating", 130)
    points, rows = [p for _, p in pairs], [r for r, _ in pairs]
    whole = _dicts(ipa.prove_many(coms, points, datas, rows=rows))
    assert whole[:5] == _dicts(ipa.prove_batch_points([coms[r] for r in rows[:5]], points[:5], [datas[r] for r in rows[:5]]))
    monkeypatch.setenv("VKZG_IPA_PROVE_CHUNK", "64")            # 64 + 64 + 2
    assert _dicts(ipa.prove_many(coms, points, datas, rows=rows)) == whole
    # row == NULL: chunk k starts at row 64 k
    assert _dicts(ipa.prove_many([coms[r] for r in rows], points, [datas[r] for r in rows])) == whole


# ---------------------------------------------------------------- 6. closing the loop
def test_flat_outputs_verify_and_a_changed_tip_is_located(eng, ipas, pool256):
    from vkzg._lib import lib
    ipa = ipas(256)
    datas, coms, _, _ = pool256
    n = 257
    pairs = _batch256(pool256, "alternating", n)
    ev = np.ascontiguousarray(np.concatenate([d.limbs(256)[:256] for d in datas]))
    from vkzg.scheme import _pt_arrays
    cxy, cinf = _pt_arrays(coms)
    row = np.array([r for r, _ in pairs], dtype=np.uint32)
    pts = _limbs([p for _, p in pairs])
    st, lxy, linf, rxy, rinf, tip, y = _raw(eng, ipa.table, 256, 3, ev, row, cxy, cinf, pts, n)
    assert st == 0
    # the verifiers take the commitment of each opening, the prover's arrays as they are
    vxy, vinf = np.ascontiguousarray(cxy[row]), np.ascontiguousarray(cinf[row])
    seed = np.frombuffer(bytes(range(32)), dtype=np.uint8).copy()

    def verdicts(tips):
        res, each = ctypes.c_int(-1), np.full(n, 7, dtype=np.uint8)
        assert lib().vc_ipa_verify_batch(eng.h, ipa.table, 256, n, _P(vxy), _P(vinf), _P(pts), _P(lxy), _P(linf), _P(rxy),
                                         _P(rinf), _P(tips), _P(y), None, _P(seed), ctypes.byref(res), None) == 0
        assert lib().vc_ipa_verify_many(eng.h, ipa.table, 256, n, _P(vxy), _P(vinf), _P(pts), _P(lxy), _P(linf), _P(rxy),
                                        _P(rinf), _P(tips), _P(y), None, _P(each)) == 0
        return res.value, each.tolist()
    assert verdicts(tip) == (1, [1] * n)
    bad = tip.copy()
    bad[200, 0] ^= 1
    assert verdicts(bad) == (0, [int(i != 200) for i in range(n)])


# ---------------------------------------------------------------- 7. arguments
def test_arguments(eng, ipas, pool256):
    import vkzg
    from vkzg.scheme import _pt_arrays
    ipa = ipas(256)
    N = 256
    datas, coms, _, _ = pool256
    ev = np.ascontiguousarray(np.concatenate([d.limbs(N)[:N] for d in datas[:2]]))      # two rows
    cxy, cinf = _pt_arrays(coms[:2])
    pts = _limbs([3, N + 1, 7])
    row = np.array([0, 1, 1], dtype=np.uint32)

    def call(e=eng, **kw):
        a = dict(table=ipa.table, N=N, rows=2, data=ev, row=row, com=cxy, cinf=cinf, points=pts, n=3)
        a.update(kw)
        return _raw(e, a["table"], a["N"], a["rows"], a["data"], a["row"], a["com"], a["cinf"], a["points"], a["n"],
                    drop=a.get("drop", ()))

    def proofs(out, n=3, K=8):
        from vkzg.scheme import _pt
        from vkzg.engine import limbs_to_int
        _, lxy, linf, rxy, rinf, tip, y = out
        return [{"l": [_pt(lxy[i * K + k], linf[i * K + k]) for k in range(K)],
                 "r": [_pt(rxy[i * K + k], rinf[i * K + k]) for k in range(K)],
                 "tip": limbs_to_int(tip[i]), "y": limbs_to_int(y[i])} for i in range(n)]
    want = [ipa.prove_point(coms[r], p, datas[r]).as_dict() for r, p in zip(row, (3, N + 1, 7))]
    out = call()
    assert out[0] == 0 and proofs(out) == want
    over_r = np.array([[3, 0, 0, 0], [2**64 - 1] * 4, [7, 0, 0, 0]], dtype=np.uint64)
    at_r = np.array([[3, 0, 0, 0], [(R >> (64 * j)) & (2**64 - 1) for j in range(4)], [7, 0, 0, 0]], dtype=np.uint64)
    invalid = [dict(N=0), dict(N=1), dict(N=255), dict(N=512),
               dict(data=None), dict(com=None), dict(cinf=None), dict(points=None)] + \
              [dict(drop=(k,)) for k in ("l_xy", "l_inf", "r_xy", "r_inf", "tip", "y")] + \
              [dict(row=None),                                            # rows (2) != n (3)
               dict(row=np.array([0, 2, 1], dtype=np.uint32)),           # a row index >= rows
               dict(points=over_r), dict(points=at_r),                    # a point >= r
               dict(table=ipas(32).table)]                                # a table of 32 + 1 points at N = 256
    for kw in invalid:
        out = call(**kw)
        assert out[0] == VC_E_INVALID and _untouched(out), kw.keys()
    bls = vkzg.Engine("bls12_381")
    try:
        out = call(e=bls, table=bls.random_bases(N + 1, seed=3))
        assert out[0] == VC_E_INVALID and _untouched(out)
    finally:
        bls.close()
    out = call(table=9999)
    assert out[0] == VC_E_TABLE and _untouched(out)
    w = cases.omega(N)
    for bad in (pow(w, 3, R), R - 1):
        for pos in range(3):
            p3 = [3, N + 1, 7]
            p3[pos] = bad
            out = call(points=_limbs(p3))
            assert out[0] == VC_E_DOMAIN and _untouched(out), (bad, pos)
    out = call(n=0)
    assert out[0] == 0 and _untouched(out)
    out = call(n=0, data=None, row=None, com=None, cinf=None, points=None)
    assert out[0] == 0 and _untouched(out)
    assert ipa.prove_many([], [], []) == []
    # and the context still proves
    out = call()
    assert out[0] == 0 and proofs(out) == want


# ---------------------------------------------------------------- 8. rows already on the device
def test_device_rows_equal_host_rows(eng, ipas, pool256):
    import torch
    from vkzg.scheme import _pt_arrays
    ipa = ipas(256)
    datas, coms, _, _ = pool256
    pairs = _batch256(pool256, "alternating", 65)
    ev = np.ascontiguousarray(np.concatenate([d.limbs(256)[:256] for d in datas]))
    cxy, cinf = _pt_arrays(coms)
    row = np.array([r for r, _ in pairs], dtype=np.uint32)
    pts = _limbs([p for _, p in pairs])
    host = _raw(eng, ipa.table, 256, 3, ev, row, cxy, cinf, pts, 65)
    d_ev = torch.from_numpy(ev.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    dev = _raw(eng, ipa.table, 256, 3, None, row, cxy, cinf, pts, 65, fn="vc_ipa_prove_many_device",
               data_ptr=d_ev.data_ptr())
    assert host[0] == 0 and dev[0] == 0
    for a, b in zip(host[1:], dev[1:]):
        assert np.array_equal(a, b)
    assert not _untouched(dev)
    assert np.array_equal(d_ev.cpu().numpy().view(np.uint64), ev)       # the caller's rows are not written

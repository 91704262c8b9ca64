"""KZG batch proving on the GPU (vc_kzg_prove_many, csrc/kzg_many.hip): n openings in one call, one
proof and one y each. Expected values are the oracle's (tests/kzg_prove_cases.py: q and y from
protocol.KZG.quotient, the proof as one scalar multiplication of g, pinned against
protocol.KZG.prove_point in tests/test_kzg_prove_many_host.py) and the single call's (vc_kzg_prove).
All results are points and field elements: no tolerance anywhere.

r - 1 is among the points the batches are built from: it is -1 = w^(N / 2), an element of every
domain of even size, where the reference divides by zero (the oracle raises), so it belongs to the
points that make the whole call fail with VC_E_DOMAIN; r - 2 stands beside it as the large point
that opens."""
import ctypes
import random

import numpy as np
import pytest

import kzg_prove_cases as cases

pytestmark = pytest.mark.gpu
R = cases.R
VC_E_INVALID, VC_E_TABLE, VC_E_RANGE, VC_E_DOMAIN = -1, -4, -5, -8


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


def _lb(evals, N):
    from vkzg import scheme
    return scheme.LagrangeBasis(list(evals), N)


def _oracle_fails(N, evals, point):
    try:
        cases.quotient(N, evals, point)
    except (IndexError, ZeroDivisionError, ValueError):
        return True
    return False


def _raw(eng, table, N, rows, width, data, row, points, n, fn="vc_kzg_prove_many", nl=8, data_ptr=None, drop=()):
    """the C call with poisoned outputs -> (status, proof_xy, proof_inf, y); drop: outputs passed as NULL"""
    from vkzg._lib import lib
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
    pxy = np.full((max(n, 1), nl), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    pinf = np.full(max(n, 1), 0xA5, dtype=np.uint8)
    y = np.full((max(n, 1), 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    st = getattr(lib(), fn)(eng.h, table, N, rows, width, ctypes.c_void_p(data_ptr) if data_ptr else P(data), P(row),
                            P(points), n, None if "proof_xy" in drop else P(pxy), None if "proof_inf" in drop else P(pinf),
                            None if "y" in drop else P(y))
    return st, pxy, pinf, y


def _untouched(out):
    _, pxy, pinf, y = out
    return bool((pxy == 0xA5A5A5A5A5A5A5A5).all() and (pinf == 0xA5).all() and (y == 0xA5A5A5A5A5A5A5A5).all())


def _limbs(vals):
    import vkzg
    return np.ascontiguousarray(vkzg.ints_to_limbs([int(v) for v in vals], 4))


# ---------------------------------------------------------------- 1. the golden
def test_golden_openings_as_one_batch(eng, kzgs):
    import json
    import os
    from vkzg import scheme
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kzg_256.json")) as f:
        g = json.load(f)
    kz = kzgs(256)
    data = scheme.LagrangeBasis([int(x, 16) for x in g["evals"]], 256)
    good = [op for op in g["openings"] if "error" not in op]
    errs = [op for op in g["openings"] if "error" in op]
    assert len(good) >= 5 and len(errs) >= 1
    got = kz.prove_batch_points(None, [int(op["point"]) for op in good], [data], rows=[0] * len(good))
    for op, pr in zip(good, got):
        assert pr["proof"] == (int(op["proof"][0], 16), int(op["proof"][1], 16)), op["point"]
        assert pr["y"] == int(op["y"], 16), op["point"]
    ev = np.ascontiguousarray(data.limbs())
    for op in errs:
        for pos in (0, len(good)):
            pts = [int(o["point"]) for o in good]
            pts.insert(pos, int(op["point"]))
            with pytest.raises(scheme.VCError) as err:
                kz.prove_batch_points(None, pts, [data], rows=[0] * len(pts))
            assert err.value.status == VC_E_DOMAIN
            out = _raw(eng, kz.table, 256, 1, len(data.evals), ev, np.zeros(len(pts), dtype=np.uint32), _limbs(pts),
                       len(pts))
            assert out[0] == VC_E_DOMAIN and _untouched(out)


# ---------------------------------------------------------------- 2. the oracle, by width
@pytest.mark.parametrize("N", [2, 32, 64, 256, 1024])
def test_widths_against_the_oracle_and_the_single_call(eng, kzgs, N):
    from vkzg import scheme
    kz = kzgs(N)
    width = N - 3 if N > 2 else 1
    evals = cases.row(N, width, 1)
    data = _lb(evals, N)
    nine = cases.standard_points(N, width)
    assert nine[:6] == [0, N - 1, width if N > 2 else 1, N + 1, N + 7, R - 1] and len(nine) == 9
    fails = [p for p in nine if _oracle_fails(N, evals, p)]
    assert fails == [R - 1]                                 # -1 = w^(N / 2)
    with pytest.raises(scheme.VCError) as err:
        kz.prove_batch_points(None, nine, [data], rows=[0] * 9)
    assert err.value.status == VC_E_DOMAIN
    points = [p if p != R - 1 else R - 2 for p in nine]     # 0, N-1 | mid | N+1, N+7, r-2, random x 3
    want = [cases.expected(N, evals, p) for p in points]
    got = kz.prove_batch_points(None, points, [data], rows=[0] * 9)
    assert got == want
    assert want[0]["y"] == evals[0] and (N == 2 or want[2]["y"] == 0)     # a point in [width, N) opens to 0
    assert got == [kz.prove_point(None, p, data) for p in points]
    # one row per opening (row == NULL), the same rows
    assert kz.prove_batch_points(None, points, [data] * 9) == want


@pytest.mark.parametrize("N", [2, 32, 256])
def test_degenerate_rows(kzgs, N):
    kz = kzgs(N)
    m = N - 1
    zero, const = (0,) * N, (12345,) * N
    single = tuple(777 if i == m else 0 for i in range(N))
    datas = [_lb(zero, N), _lb(const, N), _lb(single, N)]
    points = [0, N + 5, 1, N + 9, m, N + 3]
    rows = [0, 0, 1, 1, 2, 2]
    got = kz.prove_batch_points(None, points, datas, rows=rows)
    assert got[0] == got[1] == {"proof": None, "y": 0}
    assert got[2] == got[3] == {"proof": None, "y": 12345}
    want = [cases.expected(N, (zero, const, single)[r], p) for p, r in zip(points, rows)]
    assert got == want
    assert got[4]["y"] == 777 and got[4]["proof"] is not None


# ---------------------------------------------------------------- 3. batch edges at N = 256
def _pool256():
    """40 distinct (row, point) pairs over 3 data rows of width 253: 20 in the domain, 20 outside"""
    N, width = 256, 253
    rows = [cases.row(N, width, s) for s in (11, 12, 13)]
    rng = random.Random(256)
    inside = [0, 1, 63, 64, 65, 127, 128, 191, 252, 253, 254, 255] + rng.sample(range(2, 250), 8)
    outside = [N + 1, N + 7, R - 2, 1 << 64, (1 << 64) + 5] + [rng.randrange(N + 8, R) for _ in range(15)]
    pairs_in = [(k % 3, p) for k, p in enumerate(inside)]
    pairs_out = [(k % 3, p) for k, p in enumerate(outside)]
    return rows, pairs_in, pairs_out


def _batch256(kind, n):
    rows, pin, pout = _pool256()
    # (each pass over the 20 pairs starts one further on, so a pair meets every wave of a block)
    if kind == "inside":
        pairs = [pin[(i + i // 20) % 20] for i in range(n)]
    elif kind == "outside":
        pairs = [pout[(i + i // 20) % 20] for i in range(n)]
    else:  # alternating: the branch changes from wave to wave inside a block
        pairs = [(pin if i % 2 == 0 else pout)[(i // 2 + i // 40) % 20] for i in range(n)]
    return rows, pairs


@pytest.mark.parametrize("kind", ["inside", "outside", "alternating"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 65, 257])
def test_batch_edges(eng, kzgs, kind, n):
    kz = kzgs(256)
    rows, pairs = _batch256(kind, n)
    datas = [_lb(r, 256) for r in rows]
    want = [cases.expected(256, rows[r], p) for r, p in pairs]
    args = (None, [p for _, p in pairs], datas)
    kz.prove_batch_points(*args, rows=[r for r, _ in pairs])     # (the domain's cached tables exist after it)
    eng.enable_timing(True)
    try:
        eng.reset_timing()
        got = kz.prove_batch_points(*args, rows=[r for r, _ in pairs])
        lane, wave, inv = (eng.kernel_time(k)[1] for k in ("kzg_many_lane", "kzg_many_wave", "binv_prep"))
    finally:
        eng.enable_timing(False)
    assert got == want
    assert (lane, wave) == (1, 1)
    # the batch inversion runs once when an opening is outside the domain, never otherwise
    assert inv == (0 if kind == "inside" or (kind == "alternating" and n == 1) else 1)


def test_row_null_takes_row_i(eng, kzgs):
    kz = kzgs(256)
    rows, pairs = _batch256("alternating", 65)
    datas = [_lb(rows[r], 256) for r, _ in pairs]          # 65 rows, one per opening
    want = [cases.expected(256, rows[r], p) for r, p in pairs]
    assert kz.prove_batch_points(None, [p for _, p in pairs], datas) == want


# ---------------------------------------------------------------- 4. chunks
def test_chunks_give_the_same_openings(kzgs, monkeypatch):
    kz = kzgs(256)
    rows, pairs = _batch256("alternating", 130)
    datas = [_lb(r, 256) for r in rows]
    args = (None, [p for _, p in pairs], datas)
    whole = kz.prove_batch_points(*args, rows=[r for r, _ in pairs])
    assert whole == [cases.expected(256, rows[r], p) for r, p in pairs]
    monkeypatch.setenv("VKZG_KZG_PROVE_CHUNK", "64")       # 64 + 64 + 2
    assert kz.prove_batch_points(*args, rows=[r for r, _ in pairs]) == whole
    per_opening = [_lb(rows[r], 256) for r, _ in pairs]     # row == NULL: chunk k starts at row 64 k
    assert kz.prove_batch_points(None, [p for _, p in pairs], per_opening) == whole


# ---------------------------------------------------------------- 5. closing the loop
def test_output_verifies_and_a_changed_y_is_located(kzgs):
    kz = kzgs(256)
    rows, pairs = _batch256("alternating", 257)
    datas = [_lb(r, 256) for r in rows]
    coms = [kz.commit(d) for d in datas]
    points = [p for _, p in pairs]
    proofs = kz.prove_batch_points(None, points, datas, rows=[r for r, _ in pairs])
    cs = [coms[r] for r, _ in pairs]
    assert kz.verify_batch(cs, points, proofs, seed=bytes(range(32))) is True
    assert kz.verify_many(cs, points, proofs) == [True] * 257
    bad = list(proofs)
    bad[200] = {"proof": proofs[200]["proof"], "y": (proofs[200]["y"] + 1) % R}
    assert kz.verify_batch(cs, points, bad, seed=bytes(range(32))) is False
    assert kz.verify_many(cs, points, bad) == [i != 200 for i in range(257)]
    assert kz.verify_batch(cs, points, bad, seed=bytes(range(32)), locate=True) == (False, [i != 200 for i in range(257)])


# ---------------------------------------------------------------- 6. BLS12-381
@pytest.mark.parametrize("N", [32, 256])
def test_bls12_381_equals_the_single_calls(N):
    import vkzg
    from vkzg import dist
    from vkzg._lib import check, lib
    r = dist.BASE_P["bandersnatch"]                         # Bandersnatch's base field = BLS12-381's r
    e = vkzg.Engine("bls12_381")
    try:
        rng = random.Random(381 + N)
        tid = e.random_bases(N, seed=N)
        e.fixed_base_precompute(tid, 8)
        width = N - 3
        ev = np.ascontiguousarray(vkzg.ints_to_limbs([rng.randrange(r) for _ in range(width)]))
        points = [0, 5, N - 1, N + 7, rng.randrange(r)]
        pts = np.array([[(p >> (64 * j)) & (2**64 - 1) for j in range(4)] for p in points], dtype=np.uint64)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        want = []
        for k in range(5):
            pxy, pinf, y = np.zeros(12, dtype=np.uint64), np.zeros(1, dtype=np.uint8), np.zeros(4, dtype=np.uint64)
            check(lib().vc_kzg_prove(e.h, tid, N, P(ev), width, P(pts[k]), P(pxy), P(pinf), P(y)), "kzg_prove")
            want.append((pxy.tolist(), int(pinf[0]), y.tolist()))
        st, pxy, pinf, y = _raw(e, tid, N, 1, width, ev, np.zeros(5, dtype=np.uint32), pts, 5, nl=12)
        assert st == 0
        assert [(pxy[k].tolist(), int(pinf[k]), y[k].tolist()) for k in range(5)] == want
        assert all(w[1] == 0 for w in want) and len({tuple(w[0]) for w in want}) == 5
        # a point >= this field's r, and one equal to N
        for bad, status in ((r, VC_E_INVALID), (N, VC_E_DOMAIN)):
            p2 = pts.copy()
            p2[3] = [(bad >> (64 * j)) & (2**64 - 1) for j in range(4)]
            out = _raw(e, tid, N, 1, width, ev, np.zeros(5, dtype=np.uint32), p2, 5, nl=12)
            assert out[0] == status and _untouched(out)
    finally:
        e.close()


# ---------------------------------------------------------------- 7. arguments
def test_arguments(eng, kzgs):
    kz = kzgs(256)
    N, width = 256, 253
    ev = _limbs(cases.row(N, width, 11) + cases.row(N, width, 12))      # two rows
    pts = _limbs([3, N + 1, 7])
    row = np.array([0, 1, 1], dtype=np.uint32)
    want = [cases.expected(N, cases.row(N, width, 11 + r), p) for r, p in zip(row, (3, N + 1, 7))]

    def call(**kw):
        a = dict(table=kz.table, N=N, rows=2, width=width, data=ev, row=row, points=pts, n=3)
        a.update(kw)
        return _raw(eng, a["table"], a["N"], a["rows"], a["width"], a["data"], a["row"], a["points"], a["n"],
                    drop=a.get("drop", ()))

    from vkzg.scheme import _pt
    from vkzg.engine import limbs_to_int
    st, pxy, pinf, y = call()
    assert st == 0
    assert [{"proof": _pt(pxy[i], pinf[i]), "y": limbs_to_int(y[i])} for i in range(3)] == want
    invalid = [dict(N=255), dict(N=1), dict(N=0), dict(N=2048), dict(width=257), dict(data=None), dict(points=None),
               dict(drop=("proof_xy",)), dict(drop=("proof_inf",)), dict(drop=("y",)),
               dict(row=None),                                           # rows (2) != n (3)
               dict(row=np.array([0, 2, 1], dtype=np.uint32)),          # a row index >= rows
               dict(points=np.array([[3, 0, 0, 0], [2**64 - 1] * 4, [7, 0, 0, 0]], dtype=np.uint64)),   # a point >= r
               dict(points=np.array([[3, 0, 0, 0], [(R >> (64 * j)) & (2**64 - 1) for j in range(4)], [7, 0, 0, 0]],
                                    dtype=np.uint64))]                   # a point == r
    for kw in invalid:
        out = call(**kw)
        assert out[0] == VC_E_INVALID and _untouched(out), kw.keys()
    out = call(table=kzgs(32).table)                                     # the table has 32 points
    assert out[0] == VC_E_RANGE and _untouched(out)
    out = call(table=9999)
    assert out[0] == VC_E_TABLE and _untouched(out)
    w = cases.omega(N)
    for bad in (N, pow(w, 3, R), R - 1):
        out = call(points=_limbs([3, bad, 7]))
        assert out[0] == VC_E_DOMAIN and _untouched(out), bad
    out = call(n=0)
    assert out[0] == 0 and _untouched(out)
    out = call(n=0, data=None, row=None, points=None)
    assert out[0] == 0 and _untouched(out)
    assert kz.prove_batch_points(None, [], []) == []
    # and the context still proves
    assert call()[0] == 0


# ---------------------------------------------------------------- 8. rows already on the device
def test_device_rows_equal_host_rows(eng, kzgs):
    import torch
    kz = kzgs(256)
    rows, pairs = _batch256("alternating", 65)
    ev = _limbs([v for r in rows for v in r])
    row = np.array([r for r, _ in pairs], dtype=np.uint32)
    pts = _limbs([p for _, p in pairs])
    host = _raw(eng, kz.table, 256, 3, 253, ev, row, pts, 65)
    d_ev = torch.from_numpy(ev.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    dev = _raw(eng, kz.table, 256, 3, 253, None, row, pts, 65, fn="vc_kzg_prove_many_device", data_ptr=d_ev.data_ptr())
    assert host[0] == 0 and dev[0] == 0
    for a, b in zip(host[1:], dev[1:]):
        assert np.array_equal(a, b)
    from vkzg.scheme import _pt
    from vkzg.engine import limbs_to_int
    want = [cases.expected(256, rows[r], p) for r, p in pairs]
    assert [{"proof": _pt(dev[1][i], dev[2][i]), "y": limbs_to_int(dev[3][i])} for i in range(65)] == want
    assert np.array_equal(d_ev.cpu().numpy().view(np.uint64), ev)       # the caller's rows are not written

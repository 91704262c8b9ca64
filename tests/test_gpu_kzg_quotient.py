"""GPU: the single KZG open (csrc/poly.hip's quotient kernels behind vc_kzg_quotient, vc_kzg_prove
and its device / part / commit+prove / group forms) past one block, against plain integers.

The expected q and y are tests/kzg_quotient_cases.py's reference() (pinned against the oracle on the
CPU in tests/test_kzg_quotient_cases_host.py); every element of q is compared, as canonical integers,
and proofs as affine points: no tolerance anywhere. The sizes are the smallest at which the kernels
change regime: batch_inverse has two workgroups from n = 2048 (the host step over several workgroup
products) and chunks of 16 from n = 2^18, the barycentric and in-domain sums have two partials from
n = 4096, and the range shards of vc_group_kzg_prove have slices that are no multiple of the chunk
or the workgroup."""
import ctypes

import numpy as np
import pytest

import kzg_quotient_cases as cases

pytestmark = pytest.mark.gpu
POISON64, POISON8 = 0xA5A5A5A5A5A5A5A5, 0xA5


def _P(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _limbs(vals):
    import vkzg
    return np.ascontiguousarray(vkzg.ints_to_limbs(list(vals), 4))


def _word(point):
    return _limbs([point])[0].copy()


def _poison(*shape, dtype=np.uint64):
    return np.full(shape, POISON64 if dtype == np.uint64 else POISON8, dtype=dtype)


def _untouched(*arrays):
    return all(bool((a == (POISON64 if a.dtype == np.uint64 else POISON8)).all()) for a in arrays)


def _setup(e, n):
    """vc_kzg_setup with the public secret 100 -> table id"""
    from vkzg._lib import check, lib
    tid, size = ctypes.c_int(), ctypes.c_size_t()
    check(lib().vc_kzg_setup(e.h, n, _P(_word(cases.SECRET)), ctypes.byref(tid), ctypes.byref(size)), "vc_kzg_setup")
    assert size.value == n
    return tid.value


@pytest.fixture(scope="module")
def engines():
    """curve -> (Engine, n -> SRS table id), made on demand and shared by the module"""
    import vkzg
    made = {}

    class Ctx:
        def __init__(self, curve):
            self.e, self.tables = vkzg.Engine(curve), {}

        def table(self, n):
            if n not in self.tables:
                self.tables[n] = _setup(self.e, n)
            return self.tables[n]

    def get(curve):
        if curve not in made:
            made[curve] = Ctx(curve)
        return made[curve]
    yield get
    for c in made.values():
        c.e.close()


def _quotient(e, n, ev, mx, point):
    """vc_kzg_quotient with poisoned outputs -> (status, q (n, 4), y (4,))"""
    from vkzg._lib import lib
    q, y = _poison(n, 4), _poison(4)
    st = lib().vc_kzg_quotient(e.h, n, _P(ev), mx, _P(_word(point)), _P(q), _P(y))
    return st, q, y


def _assert_quotient(got_q, got_y, want_q, want_y, what):
    import vkzg
    assert vkzg.limbs_to_int(got_y) == want_y, what
    want = _limbs(want_q)
    if not np.array_equal(got_q, want):
        bad = np.nonzero((got_q != want).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} entries of q differ, i = {bad[0]} .. {bad[-1]}")


# ---------------------------------------------------------------- a. the whole q, multi-block
@pytest.mark.parametrize("n", cases.FULL_SIZES)
@pytest.mark.parametrize("curve", cases.CURVE_NAMES)
def test_full_quotient_multi_block(engines, curve, n):
    """vc_kzg_quotient == reference on q[0..n) and y at n = 2048 (two inversion workgroups) and 4096
    (four, and two sum blocks): i == m on the first and last lane of a chunk, a workgroup and a sum
    block, max at and beside the block edges, points outside the domain"""
    e = engines(curve).e
    table = cases.full_cases(curve, n)
    assert len(table) == cases.FULL_COUNT[n]
    for mx, point in table:
        ev = cases.evals(curve, n, mx)
        want_q, want_y = cases.reference(curve, n, ev, point)
        st, q, y = _quotient(e, n, _limbs(ev), mx, point)
        assert st == 0, (mx, point)
        _assert_quotient(q, y, want_q, want_y, (curve, n, mx, point))


# ---------------------------------------------------------------- b. batch_inverse at CH = 16
@pytest.mark.parametrize("curve", cases.CURVE_NAMES)
def test_full_quotient_at_the_chunk_switch(curve):
    """n = 2^18, the smallest size at which batch_inverse takes chunks of 16, on a fresh engine: the
    in-domain open first, so the 1 / (w^k - 1) table is inverted at CH = 16, then a point outside"""
    import vkzg
    n = cases.CH16_N
    table = cases.ch16_cases(curve)
    assert len(table) == 2 and table[0][1] < n < table[1][1]
    e = vkzg.Engine(curve)
    try:
        for mx, point in table:
            ev = cases.evals(curve, n, mx)
            want_q, want_y = cases.reference(curve, n, ev, point)
            st, q, y = _quotient(e, n, _limbs(ev), mx, point)
            assert st == 0, point
            _assert_quotient(q, y, want_q, want_y, (curve, n, mx, point))
    finally:
        e.close()


# ---------------------------------------------------------------- c. proofs at the same sizes
def _prove_forms(e, tid, n, ev, d_ev, mx, point, forms=("host", "device", "parts", "commit")):
    """every form of the single open with poisoned outputs -> {form: (status, outputs..)}; the
    proof of "parts" is the sum of 3 window parts (None when a part failed)"""
    from vkzg._lib import lib
    nl = e.nl
    pt = _word(point)
    dp = ctypes.c_void_p(d_ev.data_ptr()) if mx else None
    out = {}
    if "host" in forms:
        pxy, pinf, y = _poison(2 * nl), _poison(1, dtype=np.uint8), _poison(4)
        st = lib().vc_kzg_prove(e.h, tid, n, _P(ev), mx, _P(pt), _P(pxy), _P(pinf), _P(y))
        out["host"] = (st, pxy, pinf, y)
    if "device" in forms:
        pxy, pinf, y = _poison(2 * nl), _poison(1, dtype=np.uint8), _poison(4)
        st = lib().vc_kzg_prove_device(e.h, tid, n, dp, mx, _P(pt), _P(pxy), _P(pinf), _P(y))
        out["device"] = (st, pxy, pinf, y)
    if "parts" in forms:
        accs, ys, sts = [], [], []
        for k in range(3):
            acc = np.full(e.point_words(), 0xA5A5A5A5, dtype=np.uint32)
            yk = _poison(4)
            sts.append(lib().vc_kzg_prove_device_part(e.h, tid, n, dp, mx, _P(pt), k, 3, _P(acc), _P(yk)))
            accs.append(acc)
            ys.append(yk)
        out["parts"] = (sts, accs, ys)
    if "commit" in forms:
        cxy, cinf = _poison(2 * nl), _poison(1, dtype=np.uint8)
        pxy, pinf, y = _poison(2 * nl), _poison(1, dtype=np.uint8), _poison(4)
        st = lib().vc_kzg_commit_prove_device(e.h, tid, n, dp, mx, _P(pt), _P(cxy), _P(cinf), _P(pxy), _P(pinf),
                                              _P(y))
        out["commit"] = (st, cxy, cinf, pxy, pinf, y)
    return out


def _device(ev):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(ev).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return d


def _assert_forms_agree(e, forms, want_y, what):
    """host == device == the sum of the parts == the proof half of commit+prove; -> (proof_xy, proof_inf, y)"""
    import vkzg
    st, pxy, pinf, y = forms["host"]
    assert st == 0, what
    assert vkzg.limbs_to_int(y) == want_y, what
    st2, pxy2, pinf2, y2 = forms["device"]
    assert st2 == 0 and np.array_equal(pxy2, pxy) and pinf2[0] == pinf[0] and np.array_equal(y2, y), what
    sts, accs, ys = forms["parts"]
    assert sts == [0, 0, 0] and all(np.array_equal(yk, y) for yk in ys), what
    sxy, sinf = e.partials_sum(np.stack(accs))
    assert np.array_equal(sxy, pxy) and sinf == pinf[0], what
    st4, _, _, pxy4, pinf4, y4 = forms["commit"]
    assert st4 == 0 and np.array_equal(pxy4, pxy) and pinf4[0] == pinf[0] and np.array_equal(y4, y), what
    return pxy, pinf, y


@pytest.mark.parametrize("curve", cases.CURVE_NAMES)
def test_proofs_at_two_sum_blocks(engines, curve):
    """n = 4096: vc_kzg_prove == vc_kzg_prove_device == the sum of 3 vc_kzg_prove_device_part == the
    proof half of vc_kzg_commit_prove_device, y == reference, and pi (s - z) == C - y G (s = 100,
    kzg/mod.rs:115-154) with the oracle's group law"""
    import vkzg
    from pyoracle.curves import CURVES
    C = CURVES[curve]
    n = cases.PROOF_N
    ctx = engines(curve)
    e, tid = ctx.e, ctx.table(n)
    table = cases.proof_cases(curve)
    assert len(table) == 2
    for mx, point in table:
        evi = cases.evals(curve, n, mx)
        ev = _limbs(evi)
        _, want_y = cases.reference(curve, n, evi, point)
        forms = _prove_forms(e, tid, n, ev, _device(ev), mx, point)
        pxy, pinf, y = _assert_forms_agree(e, forms, want_y, (curve, mx, point))
        _, cxy, cinf, _, _, _ = forms["commit"]
        mxy, minf = e.msm(tid, ev)
        assert np.array_equal(cxy, mxy) and cinf[0] == minf
        com = vkzg.arrays_to_points(curve, cxy[None, :], cinf)[0]
        proof = vkzg.arrays_to_points(curve, pxy[None, :], pinf)[0]
        zval = pow(cases.omega(curve, n), point, C.r) if point < n else point
        lhs = C.mul(proof, (cases.SECRET - zval) % C.r)
        rhs = C.add(com, C.neg(C.mul(C.g, want_y)))
        assert lhs == rhs, (curve, point)


# ---------------------------------------------------------------- d. range shards with ragged slices
def _single(h, table, nl, n, ev, mx, point):
    """the one-context vc_kzg_prove on a member's context -> (proof_xy, proof_inf, y int)"""
    import vkzg
    from vkzg._lib import check, lib
    pxy, pinf, y = np.zeros(2 * nl, dtype=np.uint64), np.zeros(1, dtype=np.uint8), np.zeros(4, dtype=np.uint64)
    check(lib().vc_kzg_prove(h, table, n, _P(ev), mx, _P(_word(point)), _P(pxy), _P(pinf), _P(y)), "vc_kzg_prove")
    return pxy, int(pinf[0]), vkzg.limbs_to_int(y)


def _assert_group_equals_single(g, tid, curve, n, table):
    h0, t0 = g.member(0), g.member_table(tid, 0)
    for mx, point in table:
        evi = cases.evals(curve, n, mx)
        ev = _limbs(evi)
        _, want_y = cases.reference(curve, n, evi, point)
        pxy, pinf, y = _single(h0, t0, g.nl, n, ev, mx, point)
        gxy, ginf, gy = g.kzg_prove(tid, n, ev, point)
        assert gy == want_y and y == want_y, (curve, n, mx, point)
        assert np.array_equal(gxy, pxy) and ginf == pinf, (curve, n, mx, point)


@pytest.mark.parametrize("n,G,curve", [(n, G, "bn254") for n, G in cases.RANGE_SHAPES] + [(4096, 3, "bls12_381")])
def test_range_shards_equal_the_single_open(n, G, curve):
    """vc_group_kzg_prove over three members on one card, the default index-range split: slices of
    682/683 (a last chunk of 2 or 3), 1365/1366 (two inversion workgroups, the last one ragged) and
    2730/2731 (two sum blocks) entries; proof and y == the one-context vc_kzg_prove on the same SRS
    and y == reference. At n = 4096 the window split too."""
    from vkzg import group as vgroup
    g = vgroup.Group(curve, [0] * G)
    try:
        tid, size = g.kzg_setup(n)
        assert size == n
        table = cases.range_cases(curve, n, G)
        assert len(table) == 10
        _assert_group_equals_single(g, tid, curve, n, table)
        if n == 4096:
            g.set_msm_split(vgroup.SPLIT_WINDOWS)
            table = cases.window_cases(curve)
            assert len(table) == 2
            _assert_group_equals_single(g, tid, curve, n, table)
    finally:
        g.close()


@pytest.mark.parametrize("curve", cases.CURVE_NAMES)
def test_range_shards_with_an_empty_share(curve):
    """size = 2 over three members: member 0 holds no entry (no launch for it, the identity as its
    part of the proof); proof and y == the one-context call and y == reference"""
    from vkzg import group as vgroup
    assert cases.slices(2, 3) == [(0, 0), (0, 1), (1, 2)]
    g = vgroup.Group(curve, [0] * 3)
    try:
        tid, size = g.kzg_setup(2)
        assert size == 2
        table = cases.empty_share_cases(curve)
        assert len(table) == 5
        _assert_group_equals_single(g, tid, curve, 2, table)
    finally:
        g.close()


# ---------------------------------------------------------------- e. status rules of the single open
def _group_raw(g, tid, n, ev, mx, point):
    from vkzg._lib import lib
    xy, inf, y = _poison(2 * g.nl), _poison(1, dtype=np.uint8), _poison(4)
    st = lib().vc_group_kzg_prove(g.h, tid, n, _P(ev), mx, _P(_word(point)), _P(xy), _P(inf), _P(y))
    return st, xy, inf, y


@pytest.mark.parametrize("n", cases.STATUS_SIZES)
@pytest.mark.parametrize("curve", cases.CURVE_NAMES)
def test_status_rules_of_the_single_open(engines, curve, n):
    """vc_kzg_prove, _device, _device_part, vc_kzg_commit_prove_device, vc_kzg_quotient and
    vc_group_kzg_prove (both splits, two members): VC_E_DOMAIN at point == n, at r - 1 = w^(n / 2) and
    at w^3; VC_E_INVALID at r and at 2^256 - 1; the outputs stay as they were. r - 2 opens and equals
    reference."""
    import vkzg
    from vkzg import group as vgroup
    ctx = engines(curve)
    e, tid = ctx.e, ctx.table(n)
    mx = n - 3 if n > 3 else n
    evi = cases.evals(curve, n, mx)
    ev = _limbs(evi)
    d_ev = _device(ev)
    table = cases.status_cases(curve, n)
    assert len(table) == (5 if n == 2 else 6)
    g = vgroup.Group(curve, [0, 0])
    try:
        gtid, gsize = g.kzg_setup(n)
        assert gsize == n
        for split in (vgroup.SPLIT_AUTO, vgroup.SPLIT_WINDOWS):
            g.set_msm_split(split)
            for point, status in table:
                st, gxy, ginf, gy = _group_raw(g, gtid, n, ev, mx, point)
                assert st == status, (split, point, st)
                if status != 0:
                    assert _untouched(gxy, ginf, gy), (split, point)
        for point, status in table:
            what = (curve, n, point)
            st, q, y = _quotient(e, n, ev, mx, point)
            assert st == status, (what, st)
            forms = _prove_forms(e, tid, n, ev, d_ev, mx, point)
            if status != 0:
                assert _untouched(q, y), what
                assert forms["host"][0] == status and _untouched(*forms["host"][1:]), (what, forms["host"][0])
                assert forms["device"][0] == status and _untouched(*forms["device"][1:]), (what, forms["device"][0])
                sts, accs, ys = forms["parts"]
                assert sts == [status] * 3 and all((a == 0xA5A5A5A5).all() for a in accs) and _untouched(*ys), (what, sts)
                assert forms["commit"][0] == status and _untouched(*forms["commit"][1:]), (what, forms["commit"][0])
                continue
            want_q, want_y = cases.reference(curve, n, evi, point)
            _assert_quotient(q, y, want_q, want_y, what)
            pxy, pinf, _ = _assert_forms_agree(e, forms, want_y, what)
            for split in (vgroup.SPLIT_AUTO, vgroup.SPLIT_WINDOWS):
                g.set_msm_split(split)
                gxy, ginf, gy = g.kzg_prove(gtid, n, ev, point)
                assert gy == want_y and np.array_equal(gxy, pxy) and ginf == pinf[0], (what, split)
    finally:
        g.close()
    # and the context still opens
    st, q, y = _quotient(e, n, ev, mx, 0)
    assert st == 0 and vkzg.limbs_to_int(y) == evi[0]

"""CPU: the plain-integer reference of tests/kzg_quotient_cases.py stands on its own before it
judges a kernel (tests/test_gpu_kzg_quotient.py): it equals pyoracle.protocol.KZG.quotient at small
sizes on both curves, raises where the oracle raises, and the GPU file's case tables have the counts
their docstrings state with no "opens" case that raises."""
import random

import pytest

import kzg_quotient_cases as cases
from pyoracle import protocol
from pyoracle.curves import CURVES

RAISES = (IndexError, ZeroDivisionError, ValueError)


def _oracle(curve, n):
    """protocol.KZG(n) without its n Lagrange points (n scalar multiplications that quotient() never
    reads): the object's other fields as protocol.KZG.__init__ sets them"""
    k = protocol.KZG.__new__(protocol.KZG)
    k.curve, k.secret, k.size = CURVES[curve], cases.SECRET, n
    k.pre = protocol.PrecomputedLagrange(n, CURVES[curve])
    return k


def _points(curve, n, mx):
    r = cases.R[curve]
    rng = random.Random(f"host:{curve}:{n}:{mx}")
    pts = [0, 1, mx - 1, n - 1, n + 1, n + 7, r - 2] + [rng.randrange(n + 8, r - 2) for _ in range(3)]
    if mx < n:
        pts.append(mx + (n - mx) // 2)          # in [max, n)
    return sorted(set(pts))


@pytest.mark.parametrize("n", [2, 8, 256])
@pytest.mark.parametrize("curve", cases.CURVE_NAMES)
def test_reference_equals_the_oracle(curve, n):
    C = CURVES[curve]
    kz = _oracle(curve, n)
    assert cases.omega(curve, n) == kz.pre.omega == protocol.group_gen(n, C)
    rng = random.Random(f"evals:{curve}:{n}")
    seen = 0
    for mx in sorted({n, max(n - 3, 1), 1}):
        ev = [rng.randrange(C.r) for _ in range(mx)]
        data = protocol.LagrangeBasis(ev, n, C)
        pts = _points(curve, n, mx)
        assert {0, mx - 1, n - 1, n + 1, n + 7, C.r - 2} <= set(pts) and len(pts) >= (7 if n > 2 else 6)
        for p in pts:
            want_q, want_y = kz.quotient(p, data)
            got_q, got_y = cases.reference(curve, n, ev, p)
            assert got_y == want_y, (mx, p)
            assert got_q == want_q, (mx, p)
            assert len(got_q) == n and all(0 <= v < C.r for v in got_q)
            seen += 1
        # where the reference panics, both raise
        bad = [n, C.r - 1] + ([pow(cases.omega(curve, n), 3, C.r)] if n >= 8 else [])
        for p in bad:
            with pytest.raises(RAISES):
                kz.quotient(p, data)
            with pytest.raises(RAISES):
                cases.reference(curve, n, ev, p)
    assert seen >= (11 if n == 2 else 30)
    # a point that is no canonical field element: the oracle reduces it, the reference refuses it
    for p in (C.r, (1 << 256) - 1, -1):
        with pytest.raises(ValueError):
            cases.reference(curve, n, [1] * n, p)


@pytest.mark.parametrize("curve", cases.CURVE_NAMES)
def test_reference_at_a_multi_block_size_satisfies_the_quotient_identity(curve):
    """n = 4096 is beyond the oracle's reach; there q is pinned by what it is: with f and q as
    evaluations over the domain, f(X) - y = q(X) (X - z) holds at a point s off the domain, both
    sides by the barycentric formula (an independent per-element pow(., -1, r) here)"""
    r, n = cases.R[curve], 4096
    pw = cases.powers(curve, n)
    s = 100

    def at_s(vals):
        t = (pow(s, n, r) - 1) * pow(n, -1, r) % r
        return t * sum(v * x * pow(s - x, -1, r) for v, x in zip(vals, pw)) % r

    for mx, p in cases.proof_cases(curve):
        ev = cases.evals(curve, n, mx)
        q, y = cases.reference(curve, n, ev, p)
        z = pw[p] if p < n else p
        assert (at_s(ev) - y) % r == at_s(q) * (s - z) % r
        if p < n:
            assert y == ev[p]


def _opens(curve, n, point):
    cases.point_class(curve, n, point)      # raises where reference() does
    return True


@pytest.mark.parametrize("curve", cases.CURVE_NAMES)
def test_case_tables(curve):
    r = cases.R[curve]
    for n in cases.FULL_SIZES:
        table = cases.full_cases(curve, n)
        assert len(table) == cases.FULL_COUNT[n] == len(set(table))
        assert {mx for mx, _ in table} == {n, n - 3, 1, 0} | ({2049} if n == 4096 else set())
        for mx, p in table:
            assert mx <= n and _opens(curve, n, p)
        for mx in {mx for mx, _ in table}:
            inside = {p for m2, p in table if m2 == mx and p < n}
            assert {0, 1, 1023, 1024, 2047, n - 1} <= inside and (n == 2048 or 2048 in inside)
            assert mx == n or any(p >= mx for p in inside)
            assert sum(1 for m2, p in table if m2 == mx and p > n) == 4
        f = cases.evals(curve, n, n)
        assert f[0] == 0 and f[1023] == 0 and (n == 2048 or f[2048] == 0) and f[1] != 0 and f[1024] != 0
    assert cases.CH16_N == 1 << 18
    t = cases.ch16_cases(curve)
    assert len(t) == 2 and t[0] == (cases.CH16_N - 5, (1 << 17) + 1) and t[1][1] > cases.CH16_N
    assert all(_opens(curve, cases.CH16_N, p) for _, p in t)
    t = cases.proof_cases(curve)
    assert len(t) == 2 and 2048 <= t[0][1] < 4096 < t[1][1] and all(_opens(curve, 4096, p) for _, p in t)
    for n, G in cases.RANGE_SHAPES:
        t = cases.range_cases(curve, n, G)
        assert len(t) == 10 == len(set(t)) and all(mx <= n and _opens(curve, n, p) for mx, p in t)
        assert sum(1 for _, p in t if p < n) == 5 and {mx for mx, _ in t} == {n - 3, n // 2 + 1, 100, 0}
        assert any((hi - lo) % 4 for lo, hi in cases.slices(n, G))       # a ragged last chunk
    t = cases.window_cases(curve)
    assert len(t) == 2 and t[0][1] < 4096 < t[1][1] and all(_opens(curve, 4096, p) for _, p in t)
    t = cases.empty_share_cases(curve)
    assert len(t) == 5 and all(_opens(curve, 2, p) for _, p in t) and cases.slices(2, 3)[0] == (0, 0)
    for n in cases.STATUS_SIZES:
        t = cases.status_cases(curve, n)
        assert len(t) == (5 if n == 2 else 6)
        assert [s for _, s in t] == [-8] * (2 if n == 2 else 3) + [-1, -1, 0]
        for p, status in t:
            if status == 0:
                assert p == r - 2 and _opens(curve, n, p)
            else:
                with pytest.raises(RAISES) as err:
                    cases.point_class(curve, n, p)
                assert (err.type is ValueError) == (status == -1)

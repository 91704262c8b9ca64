"""Test helper for the single KZG open (vc_kzg_quotient, vc_kzg_prove and its device / part /
commit+prove / group forms): a plain-integer reference of KZG::prove_point's quotient and the case
tables of tests/test_gpu_kzg_quotient.py. Nothing here calls the code under test, and nothing builds
the oracle's KZG object (its SRS is one Python scalar multiplication per point);
tests/test_kzg_quotient_cases_host.py pins reference() against pyoracle.protocol.KZG.quotient at
small sizes and checks the tables.

The formulas (lagrange_basis.rs:91-142, precompute.rs:72-90), over the domain w^i, i < n, with
max = len(evals) and f_i = 0 for i >= max:
  in the domain, point = m < n:  q_i = (f_i - f_m) / (w^i - w^m)  (i != m),
                                 q_m = -w^-m sum_{i != m} q_i w^i,   y = f_m
  outside, z = point > n:        y = ((z^n - 1) / n) sum_i f_i w^i / (z - w^i),
                                 q_i = (f_i - y) / (w^i - z)
All n denominators of a call go through one Montgomery-trick batch inversion (one pow(., -1, r)), so
n = 2^18 takes about a second."""
import functools
import random

from pyoracle.curves import CURVES

CURVE_NAMES = ("bn254", "bls12_381")
R = {c: CURVES[c].r for c in CURVE_NAMES}
FR_GENERATOR = {"bn254": 5, "bls12_381": 7}     # w = g^((r - 1) / n)
SECRET = 100                                    # the reference's public test secret


@functools.lru_cache(maxsize=None)
def omega(curve, n):
    r = R[curve]
    assert n >= 1 and n & (n - 1) == 0 and (r - 1) % n == 0
    return pow(FR_GENERATOR[curve], (r - 1) // n, r)


@functools.lru_cache(maxsize=None)
def powers(curve, n):
    """(w^0, .., w^(n-1))"""
    r, w = R[curve], omega(curve, n)
    out, cur = [], 1
    for _ in range(n):
        out.append(cur)
        cur = cur * w % r
    return tuple(out)


def batch_inverse(vals, r):
    """[1 / v] for non-zero v, one modular inversion (Montgomery's trick)"""
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % r
    inv = pow(acc, -1, r)           # ValueError if a v is zero
    out = [0] * len(vals)
    for k in range(len(vals) - 1, -1, -1):
        out[k] = inv * pre[k] % r
        inv = inv * vals[k] % r
    return out


def point_class(curve, n, point):
    """m for an opening in the domain at m, None for one outside it; the only place reference()
    raises: ValueError for a point that is no canonical field element, IndexError at point == n
    (the reference's vanishing_at(size)), ZeroDivisionError for a domain element that is not below
    n (z^n == 1: the reference divides by zero, precompute.rs:86)"""
    r = R[curve]
    if not 0 <= point < r:
        raise ValueError("point is not below r")
    if point < n:
        return point
    if point == n:
        raise IndexError("vanishing_at(size) out of bounds")
    if pow(point, n, r) == 1:
        raise ZeroDivisionError("the point is a domain element")
    return None


def reference(curve, n, evals, point):
    """(q, y): q a list of n integers below r"""
    r = R[curve]
    mx = len(evals)
    assert mx <= n
    m = point_class(curve, n, point)
    pw = powers(curve, n)
    f = list(evals) + [0] * (n - mx)
    if m is not None:
        wm, fm = pw[m], f[m]
        den = [(x - wm) % r for x in pw]
        den[m] = 1
        inv = batch_inverse(den, r)
        q = [(fi - fm) * iv % r for fi, iv in zip(f, inv)]
        q[m] = 0
        s = sum(qi * x for qi, x in zip(q, pw)) % r
        q[m] = -pw[(n - m) % n] * s % r
        return q, fm
    z = point
    inv = batch_inverse([(x - z) % r for x in pw], r)        # 1 / (w^i - z)
    t = (pow(z, n, r) - 1) * pow(n, -1, r) % r
    y = -t * sum(fi * x * iv for fi, x, iv in zip(f[:mx], pw, inv)) % r
    return [(fi - y) * iv % r for fi, iv in zip(f, inv)], y


@functools.lru_cache(maxsize=None)
def evals(curve, n, mx, seed=0):
    """mx seeded random values with f_0 = 0 and a zero on either side of a block edge (f_1023, the
    last entry of the first inversion workgroup, and f_2048, the first of the second sum block)"""
    rng = random.Random(f"{curve}:{n}:{mx}:{seed}")
    f = [rng.randrange(R[curve]) for _ in range(mx)]
    for i in (0, 1023, 2048):
        if i < mx:
            f[i] = 0
    return tuple(f)


def slices(n, G):
    """the index ranges of vc_group_kzg_prove's default split: member k holds [n k / G, n (k+1) / G)"""
    return [(n * k // G, n * (k + 1) // G) for k in range(G)]


# ---------------------------------------------------------------- part a: the whole q, multi-block
FULL_SIZES = (2048, 4096)


def full_cases(curve, n):
    """(max, point) for vc_kzg_quotient at n = 2048 (two inversion workgroups, one sum block) and
    n = 4096 (four and two); every case opens. Per max in {n, n - 3, 2049 (n = 4096), 1, 0}: the
    in-domain points {0, 1, 1023, 1024, 2047, 2048 (n = 4096), n - 1} -- the chunk, workgroup and
    sum-block edges -- and n - 2 >= max where max < n, then n + 1, r - 2 and two seeded random points
    outside. 39 cases at n = 2048 (9 + 3 x 10), 59 at n = 4096 (11 + 4 x 12)."""
    r = R[curve]
    rng = random.Random(f"full:{curve}:{n}")
    out = []
    for mx in [n, n - 3] + ([2049] if n == 4096 else []) + [1, 0]:
        inside = sorted({0, 1, 1023, 1024, 2047, n - 1} | ({2048} if n > 2048 else set()))
        if mx < n:
            inside.append(n - 2)
        outside = [n + 1, r - 2, rng.randrange(n + 2, r - 2), rng.randrange(n + 2, r - 2)]
        out += [(mx, p) for p in inside + outside]
    return out


FULL_COUNT = {2048: 39, 4096: 59}

# ---------------------------------------------------------------- part b: batch_inverse at CH = 16
CH16_N = 1 << 18        # the smallest size at which batch_inverse takes chunks of 16


def ch16_cases(curve):
    """(max, point), 2 cases, both open: m = 2^17 + 1 in the domain first (on a fresh engine the
    1 / (w^k - 1) table is then inverted at CH = 16), then a seeded random point outside"""
    n = CH16_N
    rng = random.Random(f"ch16:{curve}")
    return [(n - 5, (1 << 17) + 1), (n - 5, rng.randrange(n + 2, R[curve] - 2))]


# ---------------------------------------------------------------- part c: proofs at n = 4096
PROOF_N = 4096


def proof_cases(curve):
    """(max, point), 2 cases, both open: m = 3001 in the second sum block, and a seeded random
    point outside"""
    rng = random.Random(f"proof:{curve}")
    return [(PROOF_N - 3, 3001), (PROOF_N - 3, rng.randrange(PROOF_N + 2, R[curve] - 2))]


# ---------------------------------------------------------------- part d: range shards
RANGE_SHAPES = ((2048, 3), (4096, 3), (8192, 3))    # L = 682/683, 1365/1366, 2730/2731


def range_cases(curve, n, G):
    """(max, point) for vc_group_kzg_prove's index-range split, 10 cases, all open:
    m in the first slice and in the last (f_m travels by value to the other members), m >= max,
    max inside the middle slice (its nvalid partial, the last slice's zero) in the domain and outside,
    max inside the first slice (nvalid = 0 on the others), max = 0 in the domain and outside, and two
    points outside at max = n - 3"""
    r = R[curve]
    sl = slices(n, G)
    assert G == 3 and sl[1][0] < n // 2 + 1 < sl[1][1] and 100 < sl[0][1]
    rng = random.Random(f"range:{curve}:{n}:{G}")
    z = rng.randrange(n + 2, r - 2)
    m_first, m_last = 5, n - 7
    assert sl[0][0] <= m_first < sl[0][1] and sl[-1][0] <= m_last < sl[-1][1]
    return [(n - 3, m_first), (n - 3, m_last), (n - 3, n - 2),
            (n // 2 + 1, m_last), (n // 2 + 1, z), (100, rng.randrange(n + 2, r - 2)),
            (0, m_first), (0, n + 1),
            (n - 3, n + 1), (n - 3, rng.randrange(n + 2, r - 2))]


def window_cases(curve):
    """(max, point) at (4096, 3) with the window split, 2 cases, both open"""
    rng = random.Random(f"windows:{curve}")
    return [(4093, 2049), (4093, rng.randrange(4098, R[curve] - 2))]


def empty_share_cases(curve):
    """(max, point) at size = 2 with three members (member 0's slice is empty), 5 cases, all open"""
    return [(2, 0), (2, 1), (1, 1), (2, 3), (1, R[curve] - 2)]


# ---------------------------------------------------------------- part e: status rules
STATUS_SIZES = (2, 256, 4096)
VC_E_INVALID, VC_E_DOMAIN = -1, -8


def status_cases(curve, n):
    """(point, status) for every form of the single open: VC_E_DOMAIN at n, at r - 1 = w^(n / 2) and
    (n >= 8) at w^3; VC_E_INVALID at r and at 2^256 - 1; 0 at r - 2, which opens. 5 cases at n = 2,
    6 otherwise"""
    r = R[curve]
    out = [(n, VC_E_DOMAIN), (r - 1, VC_E_DOMAIN)]
    if n >= 8:
        out.append((pow(omega(curve, n), 3, r), VC_E_DOMAIN))
    return out + [(r, VC_E_INVALID), ((1 << 256) - 1, VC_E_INVALID), (r - 2, 0)]

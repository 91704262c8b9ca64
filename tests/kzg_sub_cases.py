"""Test helper for KZG subvector proofs (vc_kzg_prove_subvector_many, vc_kzg_verify_subvector): every
expected value comes from Python integers and the oracle's curves. For a row f over the domain of
size N, a set S of distinct indices and the trapdoor s = 100:
  Z_S = prod_{i in S} (X - w^i),  I = the interpolant of f on S,  c_i = 1 / Z_S'(w^i),
  the expected proof is ((f(s) - I(s)) / Z_S(s)) * G, f(s) through protocol.kzg_lagrange_scalars.
quotient_row gives the evaluations of (f - I) / Z_S on the domain by polynomial long division in the
monomial basis, a route that shares nothing with the partial-fraction formula of csrc/kzg_sub.hpp;
tests/test_kzg_sub_host.py pins both against protocol.KZG at N = 16. Nothing here calls the code
under test. Both curves: curve = "bn254" or "bls12_381"."""
import functools
import random

from pyoracle import protocol
from pyoracle.curves import CURVES

SECRET = 100


def curve_of(name):
    return CURVES[name]


@functools.lru_cache(maxsize=None)
def scalars(N, curve="bn254"):
    return tuple(protocol.kzg_lagrange_scalars(N, SECRET, curve_of(curve)))


@functools.lru_cache(maxsize=None)
def omega(N, curve="bn254"):
    return protocol.group_gen(N, curve_of(curve))


@functools.lru_cache(maxsize=None)
def row(N, width, seed, curve="bn254"):
    """a random data row (a tuple: the caches key on it)"""
    rng = random.Random(1000 * N + seed)
    return tuple(rng.randrange(curve_of(curve).r) for _ in range(width))


def value(evals, i):
    return evals[i] if i < len(evals) else 0


def _xs(N, S, curve):
    r, w = curve_of(curve).r, omega(N, curve)
    return [pow(w, i, r) for i in S]


def weights(N, S, curve="bn254"):
    """c_i = prod_{l in S, l != i} 1 / (w^i - w^l), in S's order"""
    r = curve_of(curve).r
    x = _xs(N, S, curve)
    out = []
    for a, xa in enumerate(x):
        d = 1
        for b, xb in enumerate(x):
            if a != b:
                d = d * (xa - xb) % r
        out.append(pow(d, -1, r))
    return out


def z_coeffs(N, S, curve="bn254"):
    """the k + 1 monomial coefficients of Z_S, lowest first"""
    r = curve_of(curve).r
    z = [1]
    for xi in _xs(N, S, curve):
        z = [((z[t - 1] if t else 0) - xi * (z[t] if t < len(z) else 0)) % r for t in range(len(z) + 1)]
    return z


def _divide(num, den, r):
    """num / den in the monomial basis (den monic) -> (quotient, remainder)"""
    num = list(num)
    k = len(den) - 1
    q = [0] * max(len(num) - k, 0)
    for t in range(len(num) - 1, k - 1, -1):
        c = num[t]
        q[t - k] = c
        for u in range(k + 1):
            num[t - k + u] = (num[t - k + u] - c * den[u]) % r
    return q, num[:k]


def i_coeffs(N, S, ys, curve="bn254"):
    """the k monomial coefficients of the polynomial of degree < k through (w^i, y_i), lowest first"""
    r = curve_of(curve).r
    z, x, c = z_coeffs(N, S, curve), _xs(N, S, curve), weights(N, S, curve)
    out = [0] * len(S)
    for xi, yi, ci in zip(x, ys, c):
        li, rem = _divide(z, [(-xi) % r, 1], r)
        assert rem == [0]
        for t in range(len(S)):
            out[t] = (out[t] + yi * ci * li[t]) % r
    return out


def _horner(coeffs, x, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % r
    return acc


def proof_scalar(N, evals, S, curve="bn254"):
    """(f(s) - I(s)) / Z_S(s) mod r"""
    r = curve_of(curve).r
    fs = sum(c * v for c, v in zip(scalars(N, curve), evals)) % r
    ys = [value(evals, i) for i in S]
    Is = _horner(i_coeffs(N, S, ys, curve), SECRET, r)
    Zs = _horner(z_coeffs(N, S, curve), SECRET, r)
    return (fs - Is) * pow(Zs, -1, r) % r


def expected(N, evals, S, curve="bn254"):
    """{"proof": point | None, "ys": the values in S's order}"""
    C = curve_of(curve)
    s = proof_scalar(N, tuple(evals), tuple(S), curve)
    return {"proof": C.mul(C.g, s) if s else None, "ys": [value(evals, i) for i in S]}


def quotient_row(N, evals, S, curve="bn254"):
    """the N evaluations of (f - I) / Z_S on the domain, by long division of the coefficients"""
    r, w = curve_of(curve).r, omega(N, curve)
    ninv, winv = pow(N, -1, r), pow(w, -1, r)
    f = [value(evals, j) for j in range(N)]
    coef = []                                                       # the inverse DFT of the row
    for t in range(N):
        step, cur, acc = pow(winv, t, r), 1, 0
        for j in range(N):
            acc += f[j] * cur
            cur = cur * step % r
        coef.append(acc % r * ninv % r)
    I = i_coeffs(N, S, [value(evals, i) for i in S], curve)
    num = [(c - (I[t] if t < len(I) else 0)) % r for t, c in enumerate(coef)]
    q, rem = _divide(num, z_coeffs(N, S, curve), r)
    assert not any(rem), "f - I is divisible by Z_S"
    return [_horner(q, pow(w, j, r), r) for j in range(N)]


def standard_sets(N, width):
    """the index sets a width-`width` row of the domain N is proven on: k = 1, 2, 3, 63, 64, 65 where
    they fit, N - 1 and N, a set holding 0 and N - 1, one lying wholly in [width, N), one unsorted"""
    rng = random.Random(31 * N + width)
    sets = []
    for k in (1, 2, 3, 63, 64, 65, N - 1, N):
        if 1 <= k <= N and not any(len(s) == k for s in sets):
            sets.append(sorted(rng.sample(range(N), k)))
    sets.append(sorted({0, N - 1} | set(rng.sample(range(N), min(3, N)))))
    if width < N:
        sets.append(list(range(width, N)))
    mixed = rng.sample(range(N), min(5, N))
    sets.append(mixed if mixed != sorted(mixed) or N == 2 else mixed[::-1])
    return sets

"""Test helper for KZG subvector batch verification (vc_kzg_verify_subvector_batch): batches of
subvector proofs and their expected folds, from Python integers through tests/kzg_sub_cases.py
(z_coeffs, i_coeffs, the trapdoor s = 100) and pyoracle.curves. An entry is kept as scalars:
  {"c": the commitment's scalar f(s), "S": the index set, "ys": the values, "q": the proof's scalar}
with C = c G and pi = q G (None for 0), so every expected point of the fold is one scalar times G:
  P_t = (sum_j rho^j z_{j,t} q_j) G,
  P_H = (sum_j rho^j z_{j,0} q_j + sum_t a_t s^t - sum_j rho^j c_j) G,
and an entry is valid exactly when q Z_S(s) == c - I(s) (mod r). Nothing here calls the code under
test."""
import random

import kzg_sub_cases as cases

S_ = cases.SECRET


def set_of(N, k, seed):
    rng = random.Random(7919 * N + 31 * k + seed)
    S = rng.sample(range(N), k)
    return S


def entry(N, S, seed, curve="bn254"):
    """a valid entry over a random row of N - 3 values (N itself below 8)"""
    r = cases.curve_of(curve).r
    evals = cases.row(N, N - 3 if N >= 8 else N, seed, curve)
    c = sum(a * v for a, v in zip(cases.scalars(N, curve), evals)) % r
    return {"c": c, "S": list(S), "ys": [cases.value(evals, i) for i in S],
            "q": cases.proof_scalar(N, evals, tuple(S), curve)}


def batch(N, ks, seed=1, curve="bn254"):
    return [entry(N, set_of(N, k, seed + j), seed + j, curve) for j, k in enumerate(ks)]


def point(scalar, curve="bn254"):
    C = cases.curve_of(curve)
    scalar %= C.r
    return C.mul(C.g, scalar) if scalar else None


def args(entries, curve="bn254"):
    """(commitments, index_sets, ys, proofs) as KZGSubvectorKey.verify_batch takes them"""
    return ([point(e["c"], curve) for e in entries], [e["S"] for e in entries], [e["ys"] for e in entries],
            [point(e["q"], curve) for e in entries])


def _poly_at(coeffs, r):
    return sum(c * pow(S_, t, r) for t, c in enumerate(coeffs)) % r


def is_valid(N, e, curve="bn254"):
    r = cases.curve_of(curve).r
    if any(not 0 <= v < r for v in e["ys"]):
        return False
    z = cases.z_coeffs(N, e["S"], curve)
    I = cases.i_coeffs(N, e["S"], e["ys"], curve)
    return (e["q"] * _poly_at(z, r) - e["c"] + _poly_at(I, r)) % r == 0


def fold_scalars(N, entries, rho, curve="bn254"):
    """the scalars of [P_H, P_1 .. P_Kmax]"""
    r = cases.curve_of(curve).r
    kmax = max(len(e["S"]) for e in entries)
    p = [0] * (kmax + 1)
    a = [0] * kmax
    w = 1
    for e in entries:
        z = cases.z_coeffs(N, e["S"], curve)
        I = cases.i_coeffs(N, e["S"], e["ys"], curve)
        for t, zt in enumerate(z):
            p[t] = (p[t] + w * zt * e["q"]) % r
        for t, it in enumerate(I):
            a[t] = (a[t] + w * it) % r
        p[0] = (p[0] - w * e["c"]) % r
        w = w * rho % r
    p[0] = (p[0] + _poly_at(a, r)) % r
    return p


def fold_points(N, entries, rho, curve="bn254"):
    return [point(v, curve) for v in fold_scalars(N, entries, rho, curve)]


def tampered(e, what, r):
    """a copy of the entry with one thing changed (still well-formed)"""
    e = dict(e, ys=list(e["ys"]))
    if what == "y":
        e["ys"][len(e["ys"]) // 2] = (e["ys"][len(e["ys"]) // 2] + 1) % r
    elif what == "proof":
        e["q"] = (e["q"] + 5) % r
    elif what == "commitment":
        e["c"] = (e["c"] + 9) % r
    else:
        raise ValueError(what)
    return e

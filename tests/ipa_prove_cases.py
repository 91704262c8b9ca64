"""Test helper for IPA batch proving (vc_ipa_prove_many): the CRS of tests/golden/ipa_crs_bn254.json,
seeded data rows, and every expected value from the oracle -- the proofs from
pyoracle.protocol.IPA.prove_point (N <= 32: a proof costs well under a second there) and, for the host
check of csrc/ipa_many.hpp, the field side of a proof round by round (weights, y, w, the challenges,
a, b, the coefficients over the original CRS and the two rows of N + 1 scalars) restated from
low_level_ipa (ipa/mod.rs:268-319) with the oracle's own helpers. Nothing here calls the code under
test."""
import functools
import json
import os
import random

from pyoracle import arkser, protocol
from pyoracle.curves import BN254, BN254_R

HERE = os.path.dirname(os.path.abspath(__file__))
R = BN254_R


def _P(h):
    return None if h is None else (int(h[0], 16), int(h[1], 16))


@functools.lru_cache(maxsize=None)
def crs():
    with open(os.path.join(HERE, "golden", "ipa_crs_bn254.json")) as f:
        return [_P(h) for h in json.load(f)["points"]]


@functools.lru_cache(maxsize=None)
def golden256():
    """tests/golden/ipa_256.json: (data, commitment, [in-domain proof, out-of-domain proof]) with
    integers and point tuples"""
    with open(os.path.join(HERE, "golden", "ipa_256.json")) as f:
        g = json.load(f)
    proofs = []
    for key in ("proof_in_domain", "proof_out_domain"):
        p = g[key]
        proofs.append({"point": int(p["point"]), "l": [_P(x) for x in p["l"]], "r": [_P(x) for x in p["r"]],
                       "tip": int(p["tip"], 16), "y": int(p["y"], 16)})
    return tuple(int(x, 16) for x in g["data"]), _P(g["commitment"]), proofs


def omega(N):
    return protocol.group_gen(N)


@functools.lru_cache(maxsize=None)
def row(N, seed):
    rng = random.Random(1000 * N + seed)
    return tuple(rng.randrange(R) for _ in range(N))


@functools.lru_cache(maxsize=None)
def oracle_ipa(N):
    return protocol.IPA(N, points=crs()[:N + 1])


@functools.lru_cache(maxsize=None)
def commitment(N, evals):
    return oracle_ipa(N).commit(protocol.LagrangeBasis(list(evals), N))


@functools.lru_cache(maxsize=None)
def expected(N, evals, point, com="own"):
    """the oracle's proof {"l", "r", "tip", "y"} of the row `evals` (a tuple) at `point`; com: the
    commitment the transcript takes ("own": the row's)"""
    assert N <= 32, "the Python oracle proves at N <= 32 only"
    c = commitment(N, evals) if com == "own" else com
    return oracle_ipa(N).prove_point(c, point, protocol.LagrangeBasis(list(evals), N))


def standard_points(N, seed=7):
    """0, N - 1, one mid index, N + 1, r - 2, one seeded random (r - 1 = w^(N / 2) is a domain error)"""
    return [0, N - 1, N // 2 if N > 2 else 1, N + 1, R - 2, random.Random(N + seed).randrange(N + 2, R - 2)]


def field_trace(N, evals, point, com, l, r):
    """The field side of low_level_ipa for the recorded L_k, R_k, in the coefficient representation
    (the folded generator j of a round of width m is sum of coeff_i g_i over i = j mod m):
    {"b", "y", "w", "rounds": [{"x", "sl", "sr", "a", "b", "coeff"}], "tip"} -- sl / sr are the round's
    rows of N + 1 scalars before its challenge, a / b / coeff the state after its fold."""
    K = len(l)
    assert 1 << K == N
    a = [v % R for v in evals]
    b = oracle_ipa(N).pre.compute_barycentric_coefficients(point) if N <= 32 else \
        protocol.PrecomputedLagrange(N).compute_barycentric_coefficients(point)
    y = protocol.inner_product_f(a, b, R)
    tr = arkser.TranscriptHasher("ipa", BN254)
    tr.append_point(com, "C")
    tr.append_fr(point % R, "input point")
    tr.append_fr(y, "output point")
    w = tr.digest("w", True)
    out = {"b": list(b), "y": y, "w": w, "rounds": []}
    coeff = [1] * N
    for k in range(K):
        m = N >> k
        half = m // 2
        al, ar = protocol.split(a)
        bl, br = protocol.split(b)
        sl, sr = [0] * (N + 1), [0] * (N + 1)
        for i in range(N):
            j = i % m
            if j >= half:       # gens_R with a_L
                sl[i] = al[j - half] * coeff[i] % R
            else:               # gens_L with a_R
                sr[i] = ar[j] * coeff[i] % R
        sl[N] = w * protocol.inner_product_f(al, br, R) % R
        sr[N] = w * protocol.inner_product_f(ar, bl, R) % R
        tr.append_point(l[k], "L")
        tr.append_point(r[k], "R")
        x = tr.digest("x", True)
        a = protocol.vec_add_and_distribute_f(al, ar, x, R)
        b = protocol.vec_add_and_distribute_f(br, bl, x, R)
        coeff = [c * x % R if (i % m) < half else c for i, c in enumerate(coeff)]  # g <- g_R + x g_L
        out["rounds"].append({"x": x, "sl": sl, "sr": sr, "a": list(a), "b": list(b), "coeff": list(coeff)})
    out["tip"] = a[0]
    return out

"""Test helper for IPA batch verification (vc_ipa_verify_batch): batches built from
tests/golden/ipa_verify_many.json, and every expected value from the oracle -- E_j, the left side of
the identity low_level_verify_ipa checks, and the fold S = sum_j rho^j sigma_j E_j in
pyoracle.curves.BN254 big-int arithmetic with the fixture's recorded challenges w / x; the verdicts
are the fixture's `valid` (pyoracle.protocol.IPA.verify_point). Nothing here calls the code under
test."""
import functools
import json
import os

from pyoracle import arkser, protocol
from pyoracle.curves import BN254, BN254_R

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = [bytes(32), bytes(range(32)), bytes([0xA5] * 32)]
DST = b"vkzg-ipa-batch"


def _load(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def _P(h):
    return None if h is None else (int(h[0], 16), int(h[1], 16))


@functools.lru_cache(maxsize=None)
def crs():
    return [_P(h) for h in _load("ipa_crs_bn254.json")["points"]]


@functools.lru_cache(maxsize=None)
def entries():
    """the fixture's entries with integers and point tuples; `id` is the index in the file"""
    out = []
    for i, e in enumerate(_load("ipa_verify_many.json")["entries"]):
        out.append({"id": i, "name": e["name"], "N": e["N"], "commitment": _P(e["commitment"]),
                    "point": int(e["point"], 16), "l": [_P(x) for x in e["l"]], "r": [_P(x) for x in e["r"]],
                    "tip": int(e["tip"], 16), "y": int(e["y"], 16),
                    "prefix": None if e["prefix"] is None else [int(v, 16) for v in e["prefix"]],
                    "w": int(e["w"], 16), "x": [int(v, 16) for v in e["x"]], "valid": e["valid"]})
    return out


def fresh(N):
    return [e for e in entries() if e["N"] == N and e["prefix"] is None]


def valid_pool():
    """the 21 valid fresh-transcript N = 32 entries"""
    pool = [e for e in fresh(32) if e["valid"]]
    assert len(pool) == 21
    return pool


def tampered_pool():
    """the 7 tampered fresh-transcript N = 32 entries"""
    pool = [e for e in fresh(32) if not e["valid"]]
    assert len(pool) == 7 and all(e["name"].startswith("tamper_") for e in pool)
    return pool


def valid_batch(n):
    pool = valid_pool()
    return [pool[(5 * i + 1) % len(pool)] for i in range(n)]


def tampered_batch(n):
    """valid entries with tampered ones at positions 0, 63, 64 and n - 1"""
    out, bad = valid_batch(n), tampered_pool()
    for k, pos in enumerate(sorted({0, 63, 64, n - 1})):
        if pos < n:
            out[pos] = bad[(3 * k + n) % len(bad)]
    return out


def _s_coeffs(xs):
    """points_coeffs (ipa/mod.rs:340): round 0 decides the most significant bit, a clear bit takes
    the round's challenge"""
    K = len(xs)
    out = []
    for i in range(1 << K):
        s = 1
        for k in range(K):
            if not (i >> (K - 1 - k)) & 1:
                s = s * xs[k] % BN254_R
        out.append(s)
    return out


def sigma(e):
    """1 for a point below N, else z^N - 1 = prod_i (z - w^i)"""
    return 1 if e["point"] < e["N"] else (pow(e["point"], e["N"], BN254_R) - 1) % BN254_R


@functools.lru_cache(maxsize=None)
def _E(idx):
    e = entries()[idx]
    r, C, N, xs, z = BN254_R, BN254, e["N"], e["x"], e["point"]
    K = len(xs)
    s = _s_coeffs(xs)
    if z < N:
        bs = s[z]
    else:
        om = protocol.group_gen(N)
        t = (pow(z, N, r) - 1) * pow(N, -1, r) % r
        bs = sum(t * pow(om, i, r) * pow(z - pow(om, i, r), -1, r) * s[i] for i in range(N)) % r
    prodx = 1
    for x in xs:
        prodx = prodx * x % r
    acc = C.mul(e["commitment"], prodx)
    P = 1
    for k in range(K - 1, -1, -1):
        acc = C.add(acc, C.mul(e["l"][k], P))
        acc = C.add(acc, C.mul(e["r"][k], P * xs[k] * xs[k] % r))
        P = P * xs[k] % r
    g = crs()
    for i in range(N):
        acc = C.add(acc, C.mul(g[i], (-e["tip"] * s[i]) % r))
    return C.add(acc, C.mul(g[N], (prodx * e["w"] * e["y"] - e["w"] * e["tip"] * bs) % r))


def E(e):
    """the left side of the verifier's identity for a fixture entry (cached per entry): the identity
    (None) exactly when the entry is valid"""
    return _E(e["id"])


def oracle_fold(batch, rho):
    """S = sum_j rho^j sigma_j E_j"""
    S, w = None, 1
    for e in batch:
        S = BN254.add(S, BN254.mul(E(e), w * sigma(e) % BN254_R))
        w = w * rho % BN254_R
    return S


def oracle_rho(seed):
    return arkser.hash_to_field(seed, DST, BN254_R)


def malformed_variants(g):
    """tests/test_gpu_ipa_verify_many.py's six malformed variants of the valid entry g"""
    from pyoracle.curves import BN254_P
    cx, cy = g["commitment"]

    def v(**kw):
        return dict(g, valid=False, **kw)
    return [v(l=[(1, 1)] + g["l"][1:]),                                             # L_0 off the curve
            v(r=g["r"][:3] + [(g["r"][3][0] + BN254_P, g["r"][3][1])] + g["r"][4:]),  # x of R_3 >= p
            v(tip=BN254_R),
            v(y=g["y"] + BN254_R),
            v(point=g["point"] + BN254_R),
            v(commitment=(cx, (cy + 1) % BN254_P))]                                 # C off the curve

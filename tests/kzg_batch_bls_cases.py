"""Test helper for KZG verification on BLS12-381: tests/golden/kzg_verify_bls_16.json
(tests/golden/make_kzg_verify_bls_golden.py) as Python values, batches built from it, and every
expected value from the oracle -- the fold P1 / P2 in pyoracle.curves.BLS12_381 big-int arithmetic
with p_i from protocol.KZG.eval_point, the verdicts from protocol.KZG.verify_point with the
trapdoor, False for anything the verifier calls malformed (a point outside the subgroup of order r
included). Modelled on kzg_batch_cases.py. Nothing here calls the code under test."""
import functools
import json
import os
import random

from pyoracle import protocol
from pyoracle.curves import BLS12_381, BLS_P, BLS_R

HERE = os.path.dirname(os.path.abspath(__file__))
CURVE = "bls12_381"
SEEDS = [bytes(32), bytes(range(32)), bytes([0xA5] * 32)]


def _pt(h):
    return None if h is None else (int(h[0], 16), int(h[1], 16))


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(HERE, "golden", "kzg_verify_bls_16.json")) as f:
        g = json.load(f)
    assert g["curve"] == CURVE
    g2 = tuple(tuple(int(v, 16) for v in c) for c in g["g2"])
    entries = [{"name": e["name"], "commitment": _pt(e["commitment"]), "point": int(e["point"], 16),
                "proof": {"proof": _pt(e["proof"]), "y": int(e["y"], 16)}, "valid": e["valid"]}
               for e in g["entries"]]
    return {"secret": g["secret"], "size": g["size"], "g2": g2, "entries": entries,
            "data": [int(v, 16) for v in g["data"]], "T": _pt(g["small_order_point"]),
            "oracle": protocol.KZG(g["size"], BLS12_381, g["secret"])}


def entry(commitment, point, proof, y, name=""):
    return {"name": name, "commitment": commitment, "point": point, "proof": {"proof": proof, "y": y}}


def raw_mul(P, k):
    """k P by a double-and-add ladder over C.add / C.double. SWCurve.mul reduces its scalar mod r,
    so it cannot do cofactor work ([r] P would always come out as the identity)."""
    C = BLS12_381
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = C.double(acc)
        if bit == "1":
            acc = C.add(acc, P)
    return acc


@functools.lru_cache(maxsize=None)
def in_subgroup(P):
    return P is None or raw_mul(P, BLS_R) is None


def oracle_verdict(e):
    """protocol.KZG.verify_point, or False for an entry the verifier calls malformed (the oracle
    reduces what it is given; the verifier rejects a coordinate >= p, a point off the curve or
    outside the subgroup, y or point >= r before any arithmetic)"""
    return _verdict(e["commitment"], e["point"], e["proof"]["proof"], e["proof"]["y"])


@functools.lru_cache(maxsize=None)
def _verdict(commitment, point, proof, y):      # (the batches cycle through a few entries)
    for P in (commitment, proof):
        if P is not None and (P[0] >= BLS_P or P[1] >= BLS_P or not BLS12_381.is_on_curve(P) or not in_subgroup(P)):
            return False
    if y >= BLS_R or point >= BLS_R:
        return False
    return fixture()["oracle"].verify_point(commitment, point, {"proof": proof, "y": y})


@functools.lru_cache(maxsize=None)
def valid_pool():
    """the 18 valid fixture entries with the edge entries among the first ones: C = identity with
    y = 0, a constant polynomial (proof = identity), and an opening at point == size (the point 16
    itself, not omega^16; made with the trapdoor)"""
    C = BLS12_381
    f = fixture()
    kzg = f["oracle"]
    fx = [e for e in f["entries"] if e["valid"]]
    assert [e["name"] for e in fx] == [f"open_{i}" for i in range(16)] + ["open_17", "open_big"]
    com, size = fx[0]["commitment"], f["size"]
    y_size = 0x5eed
    pi_size = C.mul(C.add(com, C.neg(C.mul(C.g, y_size))), pow(f["secret"] - size, -1, BLS_R))
    edge = [entry(None, 9, None, 0, "identity_commitment"),
            entry(C.mul(C.g, 4242), 5, None, 4242, "constant"),
            entry(com, size, pi_size, y_size, "point_equals_size")]
    pool = [fx[0], edge[0], fx[16], edge[1], fx[17], edge[2]] + fx[1:16]
    assert kzg.eval_point(size) == size and kzg.eval_point(size - 1) != size - 1
    for e in pool:
        assert oracle_verdict(e), e["name"]
    return pool


def tampered_pool():
    """the fixture's invalid entries that are well-formed (wrong, not malformed)"""
    return [e for e in fixture()["entries"] if not e["valid"] and e["name"].startswith("tamper_")
            and e["name"] not in ("tamper_proof_off_curve", "tamper_y_equals_r")]


def subgroup_cases():
    """(name, entry): pi + T with C valid, C + T with pi valid, R itself as pi -- on the curve,
    outside the subgroup of order r; all malformed"""
    out = [(e["name"], e) for e in fixture()["entries"] if e["name"].startswith("subgroup_")]
    assert [n for n, _ in out] == ["subgroup_proof_plus_T", "subgroup_commitment_plus_T", "subgroup_R_as_proof"]
    for _, e in out:
        for P in (e["commitment"], e["proof"]["proof"]):
            assert BLS12_381.is_on_curve(P)
        assert not (in_subgroup(e["commitment"]) and in_subgroup(e["proof"]["proof"]))
        assert oracle_verdict(e) is False
    return out


def valid_batch(n):
    pool = valid_pool()
    return [pool[i % len(pool)] for i in range(n)]


@functools.lru_cache(maxsize=None)
def _scaled_pool(seed):
    """valid entries of other polynomials: entry (C, z, pi, y) scaled by k is (k C, z, k pi, k y),
    which the check accepts as it accepts the entry. A handful of scalings, made once."""
    C = BLS12_381
    rng = random.Random(seed)
    out = []
    for e in valid_pool():
        k = rng.randrange(2, BLS_R)
        out.append(entry(C.mul(e["commitment"], k), e["point"], C.mul(e["proof"]["proof"], k),
                         e["proof"]["y"] * k % BLS_R, e["name"] + "_scaled"))
    return tuple(out)


def other_valid_batch(n, seed=1):
    """a valid batch that differs from valid_batch(n) in every non-trivial point (for a second run
    through one context): scaled entries in another order"""
    pool = _scaled_pool(seed)
    return [pool[(5 * i + 3) % len(pool)] for i in range(n)]


def arrays(batch):
    return [e["commitment"] for e in batch], [e["point"] for e in batch], [e["proof"] for e in batch]


def oracle_fold(batch, rho, unweighted=False):
    """(P1, P2) with the weights rho^i (all 1 when unweighted)"""
    kzg = fixture()["oracle"]
    C, r = BLS12_381, BLS_R
    P1 = var = None
    sy, w = 0, 1
    for e in batch:
        pi, p = e["proof"]["proof"], kzg.eval_point(e["point"])
        P1 = C.add(P1, C.mul(pi, w))
        var = C.add(var, C.add(C.mul(e["commitment"], w), C.mul(pi, w * p % r)))
        sy = (sy + w * e["proof"]["y"]) % r
        if not unweighted:
            w = w * rho % r
    return P1, C.add(C.mul(C.g, sy), C.neg(var))


def trapdoor_accepts(P1, P2):
    """e(P1, [s]_2) e(P2, H) == 1 with s known: s P1 + P2 is the identity"""
    C = BLS12_381
    return C.add(C.mul(P1, fixture()["secret"]), P2) is None


def cancelling_y(n=8, a=2, b=6):
    """valid entries with y_a += 5 and y_b -= 5: the unweighted sums do not change"""
    batch = [dict(e) for e in valid_batch(n)]
    for k, d in ((a, 5), (b, -5)):
        pr = batch[k]["proof"]
        batch[k] = dict(batch[k], proof={"proof": pr["proof"], "y": (pr["y"] + d) % BLS_R})
    return batch, (a, b)


def cancelling_proofs(n=8, a=2, b=6):
    """two copies of one entry (same point) at a and b with pi_a += T and pi_b -= T, T = 7 G"""
    C = BLS12_381
    batch = [dict(e) for e in valid_batch(n)]
    src = fixture()["entries"][3]
    T = C.mul(C.g, 7)
    for k, t in ((a, T), (b, C.neg(T))):
        batch[k] = entry(src["commitment"], src["point"], C.add(src["proof"]["proof"], t), src["proof"]["y"])
    return batch, (a, b)


def malformed_cases():
    """(name, entry): a coordinate + p, a point off the curve, y = r, point >= r, and the three
    subgroup cases"""
    e = fixture()["entries"][1]
    x, y = e["proof"]["proof"]
    cx, cy = e["commitment"]
    return [("proof_x_plus_p", entry(e["commitment"], e["point"], (x + BLS_P, y), e["proof"]["y"])),
            ("proof_off_curve", entry(e["commitment"], e["point"], (x, (y + 1) % BLS_P), e["proof"]["y"])),
            ("commitment_off_curve", entry((cx, (cy + 1) % BLS_P), e["point"], (x, y), e["proof"]["y"])),
            ("y_equals_r", entry(e["commitment"], e["point"], (x, y), BLS_R)),
            ("point_plus_r", entry(e["commitment"], e["point"] + BLS_R, (x, y), e["proof"]["y"]))] + subgroup_cases()

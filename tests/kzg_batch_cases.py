"""Test helper for KZG batch verification (vc_kzg_verify_batch): batches built from
tests/golden/kzg_verify_16.json, and every expected value from the oracle -- the fold P1 / P2 in
pyoracle.curves.BN254 big-int arithmetic with p_i from protocol.KZG.eval_point, the verdicts from
protocol.KZG.verify_point. Nothing here calls the code under test."""
import functools

import kzg_verify_fixture
from pyoracle import protocol
from pyoracle.curves import BN254, BN254_P, BN254_R

SEEDS = [bytes(32), bytes(range(32)), bytes([0xA5] * 32)]


@functools.lru_cache(maxsize=None)
def fixture():
    f = kzg_verify_fixture.load()
    f["oracle"] = protocol.KZG(f["size"], secret=f["secret"])
    return f


def entry(commitment, point, proof, y, name=""):
    return {"name": name, "commitment": commitment, "point": point, "proof": {"proof": proof, "y": y}}


def oracle_verdict(e):
    """protocol.KZG.verify_point, or False for an entry the verifier calls malformed (the oracle
    reduces what it is given; the verifier rejects a coordinate >= p, a point off the curve, y or
    point >= r before any arithmetic)"""
    return _verdict(e["commitment"], e["point"], e["proof"]["proof"], e["proof"]["y"])


@functools.lru_cache(maxsize=None)
def _verdict(commitment, point, proof, y):      # (the batches cycle through a few entries)
    for P in (commitment, proof):
        if P is not None and (P[0] >= BN254_P or P[1] >= BN254_P or not BN254.is_on_curve(P)):
            return False
    if y >= BN254_R or point >= BN254_R:
        return False
    return fixture()["oracle"].verify_point(commitment, point, {"proof": proof, "y": y})


@functools.lru_cache(maxsize=None)
def valid_pool():
    """the 18 valid fixture entries with the edge entries among the first ones: C = identity with
    y = 0, a constant polynomial (proof = identity), and an opening at point == size (the point 16
    itself, not omega^16; made with the trapdoor, since the reference's prover panics there)"""
    f = fixture()
    kzg = f["oracle"]
    fx = [e for e in f["entries"] if e["valid"]]
    assert [e["name"] for e in fx] == [f"open_{i}" for i in range(16)] + ["open_17", "open_big"]
    com, size = fx[0]["commitment"], f["size"]
    y_size = 0x5eed
    pi_size = BN254.mul(BN254.add(com, BN254.neg(BN254.mul(BN254.g, y_size))), pow(f["secret"] - size, -1, BN254_R))
    edge = [entry(None, 9, None, 0, "identity_commitment"),
            entry(BN254.mul(BN254.g, 4242), 5, None, 4242, "constant"),
            entry(com, size, pi_size, y_size, "point_equals_size")]
    pool = [fx[0], edge[0], fx[16], edge[1], fx[17], edge[2]] + fx[1:16]
    assert kzg.eval_point(size) == size and kzg.eval_point(size - 1) != size - 1
    for e in pool:
        assert oracle_verdict(e), e["name"]
    return pool


def tampered_pool():
    return [e for e in fixture()["entries"] if not e["valid"]]


def valid_batch(n):
    pool = valid_pool()
    return [pool[i % len(pool)] for i in range(n)]


def arrays(batch):
    return [e["commitment"] for e in batch], [e["point"] for e in batch], [e["proof"] for e in batch]


def oracle_fold(batch, rho, unweighted=False):
    """(P1, P2) with the weights rho^i (all 1 when unweighted)"""
    kzg = fixture()["oracle"]
    C, r = BN254, BN254_R
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
    return BN254.add(BN254.mul(P1, fixture()["secret"]), P2) is None


def cancelling_y(n=8, a=2, b=6):
    """valid entries with y_a += 5 and y_b -= 5: the unweighted sums do not change"""
    batch = [dict(e) for e in valid_batch(n)]
    for k, d in ((a, 5), (b, -5)):
        pr = batch[k]["proof"]
        batch[k] = dict(batch[k], proof={"proof": pr["proof"], "y": (pr["y"] + d) % BN254_R})
    return batch, (a, b)


def cancelling_proofs(n=8, a=2, b=6):
    """two copies of one entry (same point) at a and b with pi_a += T and pi_b -= T, T = 7 G"""
    batch = [dict(e) for e in valid_batch(n)]
    src = fixture()["entries"][3]
    T = BN254.mul(BN254.g, 7)
    for k, t in ((a, T), (b, BN254.neg(T))):
        batch[k] = entry(src["commitment"], src["point"], BN254.add(src["proof"]["proof"], t), src["proof"]["y"])
    return batch, (a, b)


def malformed_cases():
    """(name, entry): a coordinate + p, a point off the curve, y = r, point >= r"""
    e = fixture()["entries"][1]
    x, y = e["proof"]["proof"]
    cx, cy = e["commitment"]
    return [("proof_x_plus_p", entry(e["commitment"], e["point"], (x + BN254_P, y), e["proof"]["y"])),
            ("proof_off_curve", entry(e["commitment"], e["point"], (x, (y + 1) % BN254_P), e["proof"]["y"])),
            ("commitment_off_curve", entry((cx, (cy + 1) % BN254_P), e["point"], (x, y), e["proof"]["y"])),
            ("y_equals_r", entry(e["commitment"], e["point"], (x, y), BN254_R)),
            ("point_plus_r", entry(e["commitment"], e["point"] + BN254_R, (x, y), e["proof"]["y"]))]

#!/usr/bin/env python3
"""Write tests/golden/kzg_verify_bls_16.json from the oracle: KZG on BLS12-381 over an SRS of 16
with 8 data values and the public secret s = 100 -- tests/golden/kzg_verify_16.json's shape on the
other curve (protocol.KZG(16, curve=BLS12_381, secret=100)).

Every entry is (commitment, point, proof point, y) with the verdict of the oracle's
KZG.verify_point (the trapdoor identity pi (s - p) == C - y G): openings at indices 0..15, at
17 and at one 250-bit point, then tampered copies, then the subgroup cases. G1 of BLS12-381 has a
cofactor: x = 5 gives a point R of E(Fq) outside G1, and T = [r] R is a non-identity point of small
order, so pi + T, C + T and R itself are on the curve; the oracle's trapdoor arithmetic reduces its
scalars mod r and cannot judge them, and the verifier calls them malformed: their verdict is
written as false. Points are [x, y] hex pairs, null = identity; g2 = 100 H is
[[x.c0, x.c1], [y.c0, y.c1]]."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
sys.path.insert(0, os.path.dirname(HERE))

import bls12_381_g2  # noqa: E402
from pyoracle import protocol  # noqa: E402
from pyoracle.curves import BLS12_381, BLS_P, BLS_R, sqrt_mod  # noqa: E402

SECRET, SRS, NDATA = 100, 16, 8
BIG_POINT = (1 << 249) + 0x1234567


def hx(v):
    return hex(v)


def pt(P):
    return None if P is None else [hx(P[0]), hx(P[1])]


def raw_mul(P, k):
    """k P by double-and-add over C.add / C.double: SWCurve.mul reduces k mod r, so it cannot do
    cofactor work"""
    C = BLS12_381
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = C.double(acc)
        if bit == "1":
            acc = C.add(acc, P)
    return acc


def small_order_point():
    """(R, T): R = (5, sqrt(129)) on E(Fq) outside G1, T = [r] R != O of order dividing the cofactor"""
    C = BLS12_381
    R = (5, sqrt_mod(5 ** 3 + 4, BLS_P))
    assert C.is_on_curve(R)
    T = raw_mul(R, BLS_R)
    assert T is not None and C.is_on_curve(T) and raw_mul(T, BLS_R) is not None
    h = (BLS_P + 1 - (-0xd201000000010000 + 1)) // BLS_R  # #E(Fq) = p + 1 - t, t = x + 1
    assert raw_mul(T, h) is None
    return R, T


def main():
    C = BLS12_381
    kzg = protocol.KZG(SRS, C, SECRET)
    data = protocol.LagrangeBasis([pow(3, 40 * i + 5, BLS_R) for i in range(NDATA)], kzg.size, C)
    com = kzg.commit(data)
    entries = []

    def entry(name, commitment, point, proof, y, expect=None, malformed=False):
        v = False if malformed else kzg.verify_point(commitment, point, {"proof": proof, "y": y})
        if expect is not None:
            assert v == expect, (name, v)
        entries.append({"name": name, "commitment": pt(commitment), "point": hx(point), "proof": pt(proof),
                        "y": hx(y), "valid": bool(v)})

    proofs = {}
    for point in list(range(16)) + [17, BIG_POINT]:
        pr = kzg.prove_point(com, point, data)
        proofs[point] = pr
        if 8 <= point <= 15:
            assert pr["y"] == 0
        entry(f"open_{point if point < 32 else 'big'}", com, point, pr["proof"], pr["y"], True)
    for i in (0, 3, 17, BIG_POINT):
        pr = proofs[i]
        tag = i if i < 32 else "big"
        entry(f"tamper_y_plus_1_{tag}", com, i, pr["proof"], (pr["y"] + 1) % BLS_R, False)
        entry(f"tamper_proof_doubled_{tag}", com, i, C.double(pr["proof"]), pr["y"], False)
        entry(f"tamper_commitment_plus_g_{tag}", C.add(com, C.g), i, pr["proof"], pr["y"], False)
    for i in (0, 7, 14):
        entry(f"tamper_index_{i}_as_{i + 1}", com, i + 1, proofs[i]["proof"], proofs[i]["y"], False)
    x, y = proofs[2]["proof"]
    entry("tamper_proof_off_curve", com, 2, (x, (y + 1) % BLS_P), proofs[2]["y"], False)
    assert proofs[1]["y"] != 0
    entry("tamper_y_equals_r", com, 1, proofs[1]["proof"], BLS_R, False)
    # the subgroup cases: on the curve, outside G1
    R, T = small_order_point()
    pr = proofs[3]
    for name, c, p in (("subgroup_proof_plus_T", com, C.add(pr["proof"], T)),
                       ("subgroup_commitment_plus_T", C.add(com, T), pr["proof"]),
                       ("subgroup_R_as_proof", com, R)):
        assert C.is_on_curve(c) and C.is_on_curve(p)
        assert raw_mul(c, BLS_R) is not None or raw_mul(p, BLS_R) is not None
        entry(name, c, 3, p, pr["y"], malformed=True)
    g2 = bls12_381_g2.mul(bls12_381_g2.H, SECRET)
    assert bls12_381_g2.on_twist(g2) and bls12_381_g2.mul(g2, BLS_R) is None
    out = {"curve": "bls12_381", "secret": SECRET, "size": kzg.size, "data": [hx(v) for v in data.evals],
           "g2": [[hx(g2[0][0]), hx(g2[0][1])], [hx(g2[1][0]), hx(g2[1][1])]],
           "small_order_point": pt(T), "entries": entries}
    with open(os.path.join(HERE, "kzg_verify_bls_16.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

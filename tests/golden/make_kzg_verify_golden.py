#!/usr/bin/env python3
"""Write tests/golden/kzg_verify_16.json from the oracle: KZG over an SRS of 16 with 8 data
values and the reference's public secret s = 100 (kzg_point_generator.rs:23) -- the shape of the
reference's test_single_proof (kzg/mod.rs:278-297).

Every entry is (commitment, point, proof point, y) with the verdict of the oracle's
KZG.verify_point (the trapdoor identity pi (s - p) == C - y G): openings at indices 0..15, at
17 and at one 250-bit point, then tampered copies. Points are [x, y] hex pairs, null = identity;
g2 = 100 H is [[x.c0, x.c1], [y.c0, y.c1]]."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
sys.path.insert(0, os.path.dirname(HERE))

import bn254_g2  # noqa: E402
from pyoracle import protocol  # noqa: E402
from pyoracle.curves import BN254, BN254_P, BN254_R  # noqa: E402

SECRET, SRS, NDATA = 100, 16, 8
BIG_POINT = (1 << 249) + 0x1234567


def hx(v):
    return hex(v)


def pt(P):
    return None if P is None else [hx(P[0]), hx(P[1])]


def main():
    kzg = protocol.KZG(SRS, BN254, SECRET)
    # 8 values over the key's domain of 16 (from_vec_and_domain in the reference's test setup)
    data = protocol.LagrangeBasis([pow(3, 40 * i + 5, BN254_R) for i in range(NDATA)], kzg.size)
    com = kzg.commit(data)
    entries = []

    def entry(name, commitment, point, proof, y, expect=None):
        v = kzg.verify_point(commitment, point, {"proof": proof, "y": y})
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
        entry(f"tamper_y_plus_1_{tag}", com, i, pr["proof"], (pr["y"] + 1) % BN254_R, False)
        entry(f"tamper_proof_doubled_{tag}", com, i, BN254.double(pr["proof"]), pr["y"], False)
        entry(f"tamper_commitment_plus_g_{tag}", BN254.add(com, BN254.g), i, pr["proof"], pr["y"], False)
    for i in (0, 7, 14):
        entry(f"tamper_index_{i}_as_{i + 1}", com, i + 1, proofs[i]["proof"], proofs[i]["y"], False)
    x, y = proofs[2]["proof"]
    entry("tamper_proof_off_curve", com, 2, (x, (y + 1) % BN254_P), proofs[2]["y"], False)
    assert proofs[1]["y"] != 0
    entry("tamper_y_equals_r", com, 1, proofs[1]["proof"], BN254_R, False)
    g2 = bn254_g2.mul(bn254_g2.H, SECRET)
    assert bn254_g2.on_twist(g2) and bn254_g2.mul(g2, BN254_R) is None
    out = {"secret": SECRET, "size": kzg.size, "data": [hx(v) for v in data.evals],
           "g2": [[hx(g2[0][0]), hx(g2[0][1])], [hx(g2[1][0]), hx(g2[1][1])]], "entries": entries}
    with open(os.path.join(HERE, "kzg_verify_16.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

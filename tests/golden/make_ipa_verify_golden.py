#!/usr/bin/env python3
"""Write tests/golden/ipa_verify_many.json from the oracle alone (pyoracle.protocol.IPA over the
CRS of ipa_crs_bn254.json): IPA openings with the verdict of the oracle's verify_point per entry
(`valid`), for the batch verifier's tests.

  N = 32   3 data vectors, openings at 0, 13, 31 (the one-hot branch), 32, 1000 and two seeded
           254-bit points; per tamper kind one accepted proof tampered (tip + 1, y + 1, L and R
           swapped, L_0 = identity, R_{K-1} doubled, C replaced by another commitment, a proof for
           point 1000 checked at 77); one valid and one tampered opening verified after a prior
           transcript: TranscriptHasher("multiproof") with append_fr(v, "t") for each v of `prefix`.
  N = 256  the two proofs of ipa_256.json, a tip + 1 variant and a wrong-point variant.
  N = 4    one valid, one tampered (the smallest N at which the order of points_coeffs matters).

Each entry also records the challenges w and x_0..x_{K-1} of its transcript, so a host check needs
no SHA-256. Points are [x, y] hex pairs, null = identity.
usage: make_ipa_verify_golden.py [out.json] [--small]   (--small: without the N = 256 entries)"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

from pyoracle import arkser, protocol  # noqa: E402
from pyoracle.curves import BN254  # noqa: E402

R = BN254.r


def hx(v):
    return hex(int(v))


def pt(P):
    return None if P is None else [hx(P[0]), hx(P[1])]


def P(h):
    return None if h is None else (int(h[0], 16), int(h[1], 16))


def load(name):
    with open(os.path.join(HERE, name)) as f:
        return json.load(f)


def prior(prefix):
    if prefix is None:
        return None
    tr = arkser.TranscriptHasher("multiproof")
    for v in prefix:
        tr.append_fr(v, "t")
    return tr


def challenges(com, point, proof, prefix):
    """w and the x_k of low_level_verify_ipa's transcript (ipa/mod.rs:321-338)"""
    tr = prior(prefix) or arkser.TranscriptHasher("ipa")
    tr.append_point(com, "C")
    tr.append_fr(point, "input point")
    tr.append_fr(proof["y"], "output point")
    w = tr.digest("w", True)
    xs = []
    for L, Rr in zip(proof["l"], proof["r"]):
        tr.append_point(L, "L")
        tr.append_point(Rr, "R")
        xs.append(tr.digest("x", True))
    return w, xs


class Maker:
    def __init__(self, N, crs):
        self.N = N
        self.ipa = protocol.IPA(N, points=crs[:N + 1])
        self.entries = []

    def entry(self, name, com, point, proof, prefix=None, expect=None):
        v = self.ipa.verify_point(com, point, proof, prior(prefix))
        if expect is not None:
            assert v == expect, (name, v)
        w, xs = challenges(com, point, proof, prefix)
        self.entries.append({"name": name, "N": self.N, "commitment": pt(com), "point": hx(point),
                             "l": [pt(x) for x in proof["l"]], "r": [pt(x) for x in proof["r"]],
                             "tip": hx(proof["tip"]), "y": hx(proof["y"]),
                             "prefix": None if prefix is None else [hx(v) for v in prefix],
                             "w": hx(w), "x": [hx(x) for x in xs], "valid": bool(v)})


def tampered(proof, **kw):
    q = {"l": list(proof["l"]), "r": list(proof["r"]), "tip": proof["tip"], "y": proof["y"]}
    q.update(kw)
    return q


def make_32(crs):
    m = Maker(32, crs)
    rng = random.Random(0x1FA32)
    datas = [protocol.LagrangeBasis.from_vec([rng.randrange(R) for _ in range(32)]) for _ in range(3)]
    coms = [m.ipa.commit(d) for d in datas]
    big = [rng.randrange(1 << 253, R) for _ in range(2)]
    points = [0, 13, 31, 32, 1000] + big
    proofs = {}
    for d in range(3):
        for i, z in enumerate(points):
            pr = m.ipa.prove_point(coms[d], z, datas[d])
            proofs[(d, z)] = pr
            m.entry(f"open_d{d}_p{i}", coms[d], z, pr, expect=True)
    a, b, c = proofs[(0, 13)], proofs[(1, 1000)], proofs[(2, big[0])]
    m.entry("tamper_tip_plus_1", coms[0], 13, tampered(a, tip=(a["tip"] + 1) % R), expect=False)
    m.entry("tamper_y_plus_1", coms[1], 1000, tampered(b, y=(b["y"] + 1) % R), expect=False)
    m.entry("tamper_l_r_swapped", coms[2], big[0], tampered(c, l=c["r"], r=c["l"]), expect=False)
    m.entry("tamper_l0_identity", coms[0], 13, tampered(a, l=[None] + a["l"][1:]), expect=False)
    m.entry("tamper_r_last_doubled", coms[1], 1000, tampered(b, r=b["r"][:-1] + [BN254.double(b["r"][-1])]),
            expect=False)
    m.entry("tamper_other_commitment", coms[1], 13, a, expect=False)
    m.entry("tamper_point_1000_as_77", coms[1], 77, b, expect=False)
    prefix = [rng.randrange(R) for _ in range(3)]
    pp = m.ipa.prove_point(coms[0], 1000, datas[0], prior(prefix))
    m.entry("prefix_valid", coms[0], 1000, pp, prefix=prefix, expect=True)
    m.entry("prefix_tamper_tip_plus_1", coms[0], 1000, tampered(pp, tip=(pp["tip"] + 1) % R), prefix=prefix,
            expect=False)
    return m.entries


def make_4(crs):
    m = Maker(4, crs)
    rng = random.Random(0x1FA04)
    data = protocol.LagrangeBasis.from_vec([rng.randrange(R) for _ in range(4)])
    com = m.ipa.commit(data)
    pr = m.ipa.prove_point(com, 9, data)
    m.entry("n4_open", com, 9, pr, expect=True)
    m.entry("n4_tamper_y_plus_1", com, 9, tampered(pr, y=(pr["y"] + 1) % R), expect=False)
    return m.entries


def make_256(crs):
    m = Maker(256, crs)
    g = load("ipa_256.json")
    com = P(g["commitment"])

    def proof(key):
        pr = g[key]
        return pr["point"], {"l": [P(x) for x in pr["l"]], "r": [P(x) for x in pr["r"]], "tip": int(pr["tip"], 16),
                             "y": int(pr["y"], 16)}
    zi, pin = proof("proof_in_domain")
    zo, pout = proof("proof_out_domain")
    m.entry("n256_in_domain", com, zi, pin, expect=True)
    m.entry("n256_out_domain", com, zo, pout, expect=True)
    m.entry("n256_tamper_tip_plus_1", com, zo, tampered(pout, tip=(pout["tip"] + 1) % R), expect=False)
    m.entry("n256_wrong_point", com, zi + 1, pin, expect=False)
    return m.entries


def build(small=False):
    crs = [P(h) for h in load("ipa_crs_bn254.json")["points"]]
    entries = make_32(crs) + make_4(crs)
    if not small:
        entries += make_256(crs)
    return {"source": "oracle/pyoracle protocol.IPA (ipa/mod.rs restated); valid = its verify_point",
            "entries": entries}


def write(path, small=False):
    with open(path, "w") as f:
        json.dump(build(small), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--small"]
    write(args[0] if args else os.path.join(HERE, "ipa_verify_many.json"), "--small" in sys.argv)

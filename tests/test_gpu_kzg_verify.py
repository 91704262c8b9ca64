"""Batched KZG verification on the GPU (vc_kzg_verify_many, csrc/pairing.hip): one verdict per
opening. Expected verdicts are the oracle's (protocol.KZG.verify_point, the trapdoor identity;
protocol.verify_multiproof), never the code under test's; the host verifier (vc_kzg_verify) must
agree byte for byte. All results are booleans: no tolerance anywhere."""
import json
import os

import pytest

import kzg_verify_fixture

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def eng():
    import vkzg
    e = vkzg.Engine("bn254")
    yield e
    e.close()


@pytest.fixture(scope="module")
def fx():
    """the fixture, its verifying key, and the host verifier's verdict per entry (computed once)"""
    from vkzg import scheme
    f = kzg_verify_fixture.load()
    f["vk"] = scheme.KZGVerifyingKey(f["g2"], f["size"])
    for e in f["entries"]:
        e["host"] = f["vk"].verify_point(e["commitment"], e["point"], e["proof"])
        assert e["host"] == e["valid"], e["name"]
    return f


def _batch(fx, n):
    """n entries cycling through the whole fixture, with tampered ones forced at positions 0, 63,
    64 and n - 1 (the ends of the first wave, the first lane of the second, the last lane)"""
    ents = fx["entries"]
    tampered = [e for e in ents if not e["valid"]]
    out = [ents[(5 * i + 1) % len(ents)] for i in range(n)]
    for k, pos in enumerate(sorted({0, 63, 64, n - 1})):
        if pos < n:
            out[pos] = tampered[(3 * k + n) % len(tampered)]
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_verify_many_matches_oracle_and_host(eng, fx, n):
    batch = _batch(fx, n)
    got = fx["vk"].verify_many(eng, [e["commitment"] for e in batch], [e["point"] for e in batch],
                               [e["proof"] for e in batch])
    assert got == [e["valid"] for e in batch]
    assert got == [e["host"] for e in batch]
    assert not got[0] and not got[n - 1]
    if n > 1:
        assert any(got)


def test_edge_entries_in_one_batch(eng, fx):
    from pyoracle import protocol
    from pyoracle.curves import BN254, BN254_P, BN254_R
    kzg = protocol.KZG(fx["size"], secret=fx["secret"])
    ents = fx["entries"]
    x, y = ents[2]["proof"]["proof"]
    const = BN254.mul(BN254.g, 4242)
    cases = [
        # (commitment, point, proof, expected); expected from the oracle where it is defined
        (const, 5, {"proof": None, "y": 4242}, None),                       # constant polynomial
        (const, 5, {"proof": None, "y": 4243}, None),
        (None, 9, {"proof": None, "y": 0}, None),                           # C = identity, y = 0
        (None, 9, {"proof": None, "y": 1}, None),
        (ents[16]["commitment"], ents[16]["point"], ents[16]["proof"], None),   # points >= size
        (ents[17]["commitment"], ents[17]["point"], ents[17]["proof"], None),
        (ents[0]["commitment"], fx["size"], ents[0]["proof"], None),        # point == size: itself, not omega^size
        (ents[2]["commitment"], 2, {"proof": (x, (y + 1) % BN254_P), "y": ents[2]["proof"]["y"]}, False),   # off curve
        (ents[2]["commitment"], 2, {"proof": (x + BN254_P, y), "y": ents[2]["proof"]["y"]}, False),   # x >= p
        (ents[1]["commitment"], 1, {"proof": ents[1]["proof"]["proof"], "y": BN254_R}, False),       # y = r
        (ents[1]["commitment"], 1, {"proof": ents[1]["proof"]["proof"], "y": ents[1]["proof"]["y"] + BN254_R}, False),
        (ents[1]["commitment"], 1 + BN254_R, ents[1]["proof"], False),                              # point >= r
        (ents[1]["commitment"], 1, ents[1]["proof"], None),                 # a good one after the bad ones
    ]
    want = [kzg.verify_point(c, p, pr) if exp is None else exp for c, p, pr, exp in cases]
    assert want == [True, False, True, False, True, True, False, False, False, False, False, False, True]
    got = fx["vk"].verify_many(eng, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    assert got == want
    assert got == [fx["vk"].verify_point(c, p, pr) for c, p, pr, _ in cases]


def test_amortized_proofs_of_size_256(eng):
    """test_amortized_proof (kzg/mod.rs:299-308) at 256: every FK opening verifies, and with the y
    of entries 0, 100 and 255 changed exactly those three fail"""
    from vkzg import scheme
    kzg = scheme.KZG(eng, 256)
    data = scheme.LagrangeBasis([pow(7, 3 * i + 1, scheme.R_BN254) for i in range(256)])
    com = kzg.commit(data)
    proofs = kzg.prove_all_points(data, mode=1)
    assert len(proofs) == 256 and [p["y"] for p in proofs] == list(data.evals)
    assert kzg.verify_many([com] * 256, list(range(256)), proofs) == [True] * 256
    bad = {0, 100, 255}
    tampered = [{"proof": p["proof"], "y": (p["y"] + 1) % scheme.R_BN254} if i in bad else p
                for i, p in enumerate(proofs)]
    assert kzg.verify_many([com] * 256, list(range(256)), tampered) == [i not in bad for i in range(256)]


def test_two_keys_alternate_on_one_context(eng, fx):
    """s = 100 and s = 101 on one context: each key accepts its own openings and rejects the
    other's (the uploaded line tables are keyed per verifying key)"""
    from pyoracle import protocol
    from vkzg import scheme
    k100, k101 = scheme.KZG(eng, 16, secret=100), scheme.KZG(eng, 16, secret=101)
    assert k100.g2() == fx["g2"] and k101.g2() != fx["g2"]
    data = scheme.LagrangeBasis(fx["data"], 16)
    pts = [0, 5, 11, 17]
    sets = {}
    for k in (k100, k101):
        com = k.commit(data)
        sets[k.secret] = (com, [k.prove_point(com, p, data) for p in pts])
    oracles = {s: protocol.KZG(16, secret=s) for s in (100, 101)}
    for _ in range(2):
        for k in (k100, k101):
            for s, (com, proofs) in sets.items():
                want = [oracles[k.secret].verify_point(com, p, pr) for p, pr in zip(pts, proofs)]
                assert want == [s == k.secret] * len(pts)
                assert k.verify_many([com] * len(pts), pts, proofs) == want


def test_verify_multiproof_kzg_golden_256(eng):
    """the oracle-made KZG multiproof of multiproof_256.json (Q = 64) is accepted; with D replaced,
    with one query's y changed, and with the inner proof's y changed it is rejected -- the verdicts
    of protocol.verify_multiproof"""
    from pyoracle import protocol
    from pyoracle.curves import BN254
    from vkzg import scheme
    with open(os.path.join(HERE, "golden", "multiproof_256.json")) as f:
        g = json.load(f)
    P = lambda h: None if h is None else (int(h[0], 16), int(h[1], 16))  # noqa: E731
    N = 256
    vq = [(P(cw), z, (int(r0, 16) + z) % scheme.R_BN254) for r0, z, cw in zip(g["r0"], g["z"], g["kzg"]["commits"])]
    mp = {"d": P(g["kzg"]["d"]), "proof": {"proof": P(g["kzg"]["proof"]["proof"]), "y": int(g["kzg"]["proof"]["y"], 16)}}
    vq_bad = list(vq)
    vq_bad[10] = (vq[10][0], vq[10][1], (vq[10][2] + 1) % scheme.R_BN254)
    cases = [(vq, mp),
             (vq, {"d": BN254.double(mp["d"]), "proof": mp["proof"]}),
             (vq_bad, mp),
             (vq, {"d": mp["d"], "proof": {"proof": mp["proof"]["proof"], "y": (mp["proof"]["y"] + 1) % scheme.R_BN254}})]
    oracle = protocol.KZG(N)
    want = [protocol.verify_multiproof(oracle, q, m) for q, m in cases]
    assert want == [True, False, False, False]
    kzg = scheme.KZG(eng, N)
    assert [scheme.verify_multiproof_kzg(kzg, q, m) for q, m in cases] == want
    # the existing call keeps returning the claim, and the host verifier accepts it with the proof
    claim = scheme.verify_multiproof(kzg, vq, mp)
    assert kzg.verify_point(claim["commitment"], claim["t"], mp["proof"])

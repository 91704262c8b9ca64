"""GPU: verkle tree proofs (include/vc_verkle.h: vc_verkle_prove / vc_verkle_verify) against the
oracle. The statement -- which openings a set of keys needs, in which order -- is restated over
the oracle tree in tests/verkle_proof_walk.py; pyoracle.protocol.prove_multiproof (multiproof.rs:99-176)
over those queries gives the expected D and inner proof, compared exactly (group and field elements).

Trees: key length 3 (the reference tests') and 32 (the bench's), over KZG(256) and IPA(256); N = 32
holds the boundary stems and the level-skipping quirk keys of tests/verkle32_keys.py, both trees one
key whose value is 32 zero bytes (its C_half is the identity). Keys the oracle's get_single does not
find are left out by the helper. The prover's sparse field phase is also compared with the dense
route composed from existing calls: vc_multiproof_prove over vc_verkle_proof_queries' rows."""
import ctypes
import json
import os

import numpy as np
import pytest

import verkle_proof_walk as vw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 23


def _ipa_points():
    with open(os.path.join(HERE, "golden", "ipa_crs_bn254.json")) as f:
        return [(int(h[0], 16), int(h[1], 16)) for h in json.load(f)["points"]][:257]


@pytest.fixture(scope="module")
def eng():
    import vkzg
    e = vkzg.Engine("bn254")
    yield e
    e.close()


_VC = {}


def _vc(eng, scheme_name):
    """(engine scheme object, oracle scheme object, the oracle tree's commit function)"""
    if scheme_name not in _VC:
        from pyoracle import cref, protocol
        from pyoracle.curves import BN254
        from vkzg import scheme
        if scheme_name == "kzg":
            cj = protocol.kzg_lagrange_scalars(256)

            def commit(vals):  # L_j = c_j G  ->  sum v_j L_j = (sum c_j v_j) G
                return BN254.mul(BN254.g, sum(c * v for c, v in zip(cj, vals)) % BN254.r)
            _VC[scheme_name] = (scheme.KZG(eng, 256), protocol.KZG(256), commit)
        else:
            pts = _ipa_points()

            def commit(vals):
                return cref.msm("bn254", pts[:len(vals)], list(vals), 16)
            _VC[scheme_name] = (scheme.IPA(eng, 256, pts), protocol.IPA(256, points=pts), commit)
    return _VC[scheme_name]


_TREES = {}


@pytest.fixture(params=[("kzg", 3), ("kzg", 32), ("ipa", 3), ("ipa", 32)], ids=lambda p: f"{p[0]}-N{p[1]}")
def setup(request, eng, oracle_c):
    """per (scheme, N), built once: the engine tree and the oracle tree, both committed, the provable
    (key, value) pairs, and the oracle's proofs by key subset (computed on first use)"""
    scheme_name, N = request.param
    if request.param not in _TREES:
        from pyoracle import verkle as ov
        from vkzg._lib import VCError
        from vkzg.verkle import VerkleTree
        vc, ovc, commit = _vc(eng, scheme_name)
        o, items = vw.build(N, SEED, ov.VerkleTree, ov.VerklePanic)
        t, items_e = vw.build(N, SEED, VerkleTree, VCError)
        assert items == items_e
        oroot = o.commitment(commit)
        assert t.commitment(eng, vc.table) == oroot
        kv = vw.provable(o, items)
        assert len(kv) >= 20 and kv[-1][1] == bytes(32)
        _TREES[request.param] = {"N": N, "t": t, "o": o, "vc": vc, "ovc": ovc, "commit": commit, "root": oroot,
                                 "kv": kv, "scheme": scheme_name, "want": {}}
    return _TREES[request.param]


def _subsets(S):
    kv = S["kv"]
    # two keys sharing every internal node: the deepest pair under one parent the walk finds
    d = vw.walk(S["o"], [k for k, _ in kv])["depth"]
    by_prefix = {}
    for (k, v), dk in zip(kv, d):
        by_prefix.setdefault(k[:dk - 1] if dk > 1 else b"", []).append((k, v))
    pair = max(by_prefix.items(), key=lambda pg: (len(pg[1]) >= 2, len(pg[0])))[1][:2]
    assert len(pair) == 2
    return {"one": kv[:1], "pair": pair, "twice": [kv[1], kv[1]], "all": kv}


def _want(S, name):
    """the oracle's proof of subset `name` (cached)"""
    if name not in S["want"]:
        from pyoracle import protocol
        kv = _subsets(S)[name]
        w = vw.walk(S["o"], [k for k, _ in kv], S["commit"])
        qs = [(protocol.LagrangeBasis(ev, 256), C, z, y) for ev, C, z, y in w["queries"]]
        w["mp"] = protocol.prove_multiproof(S["ovc"], qs)
        S["want"][name] = w
    return S["want"][name]


def _same_inner(S, got, want):
    if S["scheme"] == "ipa":
        return got.l == want["l"] and got.r == want["r"] and got.tip == want["tip"] and got.y == want["y"]
    return got["proof"] == want["proof"] and got["y"] == want["y"]


@pytest.mark.parametrize("name", ["one", "pair", "twice", "all"])
def test_proof_matches_oracle(eng, setup, name):
    """D, the inner proof, the commitment list and the depths == the oracle's; proof_size == the
    lengths produced == the test's own walk. `all`: many queries per z row, several nodes in one
    column of a row, extension columns 0..3 colliding with internal columns."""
    S = setup
    kv = _subsets(S)[name]
    keys = [k for k, _ in kv]
    want = _want(S, name)
    root, proof = S["t"].prove(eng, S["vc"], keys)
    assert root == S["root"]
    assert proof.depth == want["depth"]
    assert proof.commitments == want["commitments"]
    assert proof.d == want["mp"]["d"], "D differs: the per-point sums"
    assert _same_inner(S, proof.inner, want["mp"]["proof"])
    n_com, n_q = S["t"].proof_size(keys)
    assert (n_com, n_q) == (len(proof.commitments), want["n_queries"]) == (want["n_com"], want["n_queries"])
    cxy, cinf, z, y = S["t"].proof_queries(eng, S["vc"].table, keys)
    assert len(z) == n_q and [int(v) for v in z] == [q[2] for q in want["queries"]]
    from vkzg import limbs_to_int
    assert [limbs_to_int(r) for r in y] == [q[3] for q in want["queries"]]


def _dense_route(eng, S, keys):
    """vc_multiproof_prove over vc_verkle_proof_queries' dense rows"""
    from vkzg import scheme
    from vkzg._lib import check, lib
    P = scheme._p
    cxy, cinf, z, y, rows = S["t"].proof_queries(eng, S["vc"].table, keys, rows=True)
    Q = len(z)
    dxy = np.zeros(8, dtype=np.uint64)
    dinf = np.zeros(1, dtype=np.uint8)
    if S["scheme"] == "ipa":
        b, arrs = scheme.IPAProof._alloc(8)
        check(lib().vc_multiproof_prove(eng.h, 0, S["vc"].table, 256, Q, P(rows), P(cxy), P(cinf), P(z), P(y), P(dxy),
                                        P(dinf), ctypes.byref(b), None, None, None), "vc_multiproof_prove")
        return scheme._pt(dxy, dinf[0]), scheme.IPAProof._from(b, arrs).as_dict()
    kxy = np.zeros(8, dtype=np.uint64)
    kinf = np.zeros(1, dtype=np.uint8)
    ky = np.zeros(4, dtype=np.uint64)
    check(lib().vc_multiproof_prove(eng.h, 1, S["vc"].table, 256, Q, P(rows), P(cxy), P(cinf), P(z), P(y), P(dxy),
                                    P(dinf), None, P(kxy), P(kinf), P(ky)), "vc_multiproof_prove")
    return scheme._pt(dxy, dinf[0]), {"proof": scheme._pt(kxy, kinf[0]), "y": scheme.limbs_to_int(ky)}


@pytest.mark.parametrize("name", ["one", "all"])
def test_sparse_field_phase_equals_dense_route(eng, setup, name):
    S = setup
    keys = [k for k, _ in _subsets(S)[name]]
    _, proof = S["t"].prove(eng, S["vc"], keys)
    d, inner = _dense_route(eng, S, keys)
    assert proof.d == d
    assert _same_inner(S, proof.inner, inner)


def _some(S):
    """a handful of keys for the verifier tests: the first five and the zero-valued one"""
    return S["kv"][:5] + S["kv"][-1:]


def _verify(eng, S, root, kv, proof):
    from vkzg import verkle
    return verkle.verify(eng, S["vc"], S["N"], root, [k for k, _ in kv], [v for _, v in kv], proof)


def test_verify_accepts(eng, setup):
    S = setup
    for kv in (_some(S), S["kv"], [S["kv"][1], S["kv"][1]]):
        root, proof = S["t"].prove(eng, S["vc"], [k for k, _ in kv])
        assert _verify(eng, S, root, kv, proof)


def test_verify_rejects(eng, setup):
    """verdict 0 (no error) for: a value byte flipped, a depth changed, two commitments swapped, a
    commitment replaced by another valid point, two keys swapped under their values, D replaced, the
    root replaced"""
    import copy
    S = setup
    kv = _some(S)
    root, proof = S["t"].prove(eng, S["vc"], [k for k, _ in kv])
    assert _verify(eng, S, root, kv, proof)

    bad = list(kv)
    bad[2] = (bad[2][0], bytes([bad[2][1][0] ^ 1]) + bad[2][1][1:])
    assert not _verify(eng, S, root, bad, proof)
    bad = list(kv)
    bad[-1] = (bad[-1][0], bytes(31) + b"\x01")  # the zero value's high half
    assert not _verify(eng, S, root, bad, proof)

    for delta in (1, -1):
        p = copy.deepcopy(proof)
        p.depth[1] += delta
        assert not _verify(eng, S, root, kv, p)
    p = copy.deepcopy(proof)
    p.depth[0] = S["N"]
    assert not _verify(eng, S, root, kv, p)

    p = copy.deepcopy(proof)
    i, j = next((a, b) for a in range(len(p.commitments)) for b in range(a + 1, len(p.commitments))
                if p.commitments[a] != p.commitments[b])
    p.commitments[i], p.commitments[j] = p.commitments[j], p.commitments[i]
    assert not _verify(eng, S, root, kv, p)

    p = copy.deepcopy(proof)
    p.commitments[0] = proof.d
    assert not _verify(eng, S, root, kv, p)

    p = copy.deepcopy(proof)
    p.commitments.append(proof.d)  # a count that does not match the walk
    assert not _verify(eng, S, root, kv, p)

    swapped = [(kv[1][0], kv[0][1]), (kv[0][0], kv[1][1])] + kv[2:]
    assert not _verify(eng, S, root, swapped, proof)

    p = copy.deepcopy(proof)
    p.d = proof.commitments[0]
    assert not _verify(eng, S, root, kv, p)

    assert not _verify(eng, S, proof.commitments[0], kv, proof)

    # the same key twice with two values: one opening, two claims
    twice = [kv[0], (kv[0][0], kv[1][1])]
    r2, p2 = S["t"].prove(eng, S["vc"], [kv[0][0], kv[0][0]])
    assert _verify(eng, S, r2, [kv[0], kv[0]], p2)
    assert not _verify(eng, S, r2, twice, p2)


def test_verify_malformed_point_is_a_verdict(eng, setup):
    S = setup
    import copy
    kv = _some(S)
    root, proof = S["t"].prove(eng, S["vc"], [k for k, _ in kv])
    p = copy.deepcopy(proof)
    x, y = p.commitments[0]
    p.commitments[0] = (x, y ^ 1)  # off the curve
    assert not _verify(eng, S, root, kv, p)


def test_absent_key_is_an_error(eng, setup):
    from vkzg._lib import VCError
    S = setup
    absent = bytes([S["kv"][0][0][0] ^ 0x55]) + bytes([250] * (S["N"] - 1))
    assert S["o"].get_single(absent) is None
    with pytest.raises(VCError):
        S["t"].prove(eng, S["vc"], [S["kv"][0][0], absent])
    with pytest.raises(VCError):
        S["t"].proof_size([absent])


def _fresh_tree(S):
    from vkzg._lib import VCError
    from vkzg.verkle import VerkleTree
    t, _ = vw.build(S["N"], SEED, VerkleTree, VCError)
    return t


def test_prove_commits_a_dirty_tree(eng, setup):
    """insert after a commitment, then prove without committing: the proof is against the new root"""
    S = setup
    t = _fresh_tree(S)
    old = t.commitment(eng, S["vc"].table)
    assert old == S["root"]
    new_key = bytes([S["kv"][0][0][0]]) + bytes([251] * (S["N"] - 1))
    new_val = bytes(range(100, 132))
    t.insert_single(new_key, new_val)
    assert t.stats()["dirty"] > 0
    kv = [S["kv"][0], (new_key, new_val)]
    root, proof = t.prove(eng, S["vc"], [k for k, _ in kv])
    assert t.stats()["dirty"] == 0
    assert root != old and root == t.commitment(eng, S["vc"].table)
    assert _verify(eng, S, root, kv, proof)
    assert not _verify(eng, S, old, kv, proof)


def test_prove_after_a_host_path_commitment(eng, setup, monkeypatch):
    """the tree last committed on the host path (VKZG_VERKLE_DEV=0): proving uploads the host arrays
    into a fresh device mirror -- the same proof as after a device-path commitment"""
    S = setup
    kv = _some(S)
    keys = [k for k, _ in kv]
    t = _fresh_tree(S)
    monkeypatch.setenv("VKZG_VERKLE_DEV", "0")
    assert t.commitment(eng, S["vc"].table) == S["root"]
    monkeypatch.delenv("VKZG_VERKLE_DEV")
    root, proof = t.prove(eng, S["vc"], keys)
    root2, proof2 = S["t"].prove(eng, S["vc"], keys)
    assert root == root2 == S["root"]
    assert proof.as_dict() == proof2.as_dict()
    assert _verify(eng, S, root, kv, proof)

"""vc_multiproof_verify_many_ipa / _kzg and vc_multiproof_claims_many (csrc/mp_verify.hip): P
multiproofs verified in one call, a verdict each, against the single calls
(vc_multiproof_verify_ipa / _kzg, vc_multiproof_kzg_claim) and the oracle. The batches and the
damage are tests/mp_verify_cases.py."""
import json
import os

import numpy as np
import pytest

import mp_verify_cases as mc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def eng():
    import vkzg
    e = vkzg.Engine("bn254")
    yield e
    e.close()


@pytest.fixture(scope="module")
def ipa8(eng):
    from vkzg import scheme
    return scheme.IPA(eng, 8, scheme.ipa_crs(9))


@pytest.fixture(scope="module")
def batch70(ipa8):
    """70 proofs (a second block of the lane-per-proof kernels), ragged; entry 2 has 7 queries and
    entry 69 three, for the damage that needs them. Made once, never changed: tests copy."""
    counts = mc.counts_for(70, seed=11, forced={2: 7, 69: 3})
    batch = mc.make_batch(ipa8, 8, counts, seed=12)
    return batch, mc.arrays(ipa8, batch)


def test_parity_ipa(ipa8, batch70):
    batch, a = batch70
    assert sorted(set(len(vq) for vq, _ in batch)) == sorted(mc.QCOUNTS)
    st, cxy, cinf, t, bad = mc.call_claims(ipa8, 8, a)
    assert st == mc.VC_OK and not bad.any()
    for p in range(70):
        s1, oxy, oinf, ot = mc.single_claim(ipa8, 8, a, p)
        assert s1 == mc.VC_OK
        assert int(cinf[p]) == oinf and np.array_equal(cxy[p], oxy) and np.array_equal(t[p], ot), p
    st, res = mc.call_ipa(ipa8.engine.h, ipa8.table, 8, a)
    assert st == mc.VC_OK and res.tolist() == [1] * 70
    for p in (0, 17, 69):
        assert mc.single_ipa(ipa8, 8, a, p) == (mc.VC_OK, 1)


def test_claims_against_the_oracle(ipa8, batch70):
    """E - D and t of three entries == what pyoracle.protocol.verify_multiproof hands verify_point"""
    from pyoracle import protocol
    from vkzg import scheme
    batch, a = batch70
    st, cxy, cinf, t, bad = mc.call_claims(ipa8, 8, a)
    assert st == mc.VC_OK

    class Capture:  # verify_multiproof's `vc`: records what the inner verifier would be given
        curve, N = protocol.BN254, 8

        def verify_point(self, com, point, proof, tr):
            self.got = (com, point)
            return True

    lens = [len(vq) for vq, _ in batch]
    picks = [lens.index(1), lens.index(3), lens.index(65)]
    for p in picks:
        cap = Capture()
        vq, mp = batch[p]
        protocol.verify_multiproof(cap, vq, {"d": mp["d"], "proof": None})
        assert scheme._pt(cxy[p], cinf[p]) == cap.got[0] and scheme.limbs_to_int(t[p]) == cap.got[1], p


def test_uniform_layout_on_prove_many_output(eng):
    """q_ptr == NULL: vc_multiproof_prove_many's [P][Q] arrays passed on without repacking"""
    import torch
    import vkzg
    from vkzg import scheme
    N, P, Q = 8, 5, 65
    ipa = scheme.IPA(eng, N, scheme.ipa_crs(N + 1))
    rng = np.random.default_rng(5)
    data = vkzg.random_scalars("bn254", P * Q * N, rng)
    z = rng.integers(0, N, size=(P, Q)).astype(np.uint64)
    d_all = torch.from_numpy(data.view(np.int64).copy()).cuda()
    cxy, cinf = eng.msm_batch(ipa.table, data, N)
    cxy = np.ascontiguousarray(cxy.reshape(P, Q, 8))
    cinf = np.ascontiguousarray(cinf.reshape(P, Q))
    y = np.ascontiguousarray(data.reshape(P * Q, N, 4)[np.arange(P * Q), z.reshape(-1).astype(np.int64)].reshape(P, Q, 4))
    mps = scheme.prove_multiproof_many(ipa, cxy, cinf, z, y, d_all.data_ptr())
    dxy, dinf = scheme._pt_arrays_many([mp["d"] for mp in mps])
    (_, _, _, lxy, linf, rxy, rinf, tips, ys), good = ipa._verify_many_arrays([None] * P, [0] * P, [mp["proof"] for mp in mps])
    assert all(good)
    a = {"P": P, "cxy": cxy, "cinf": cinf, "z": z, "y": y, "dxy": dxy, "dinf": dinf, "lxy": lxy, "linf": linf,
         "rxy": rxy, "rinf": rinf, "tip": tips, "iy": ys}
    st, res = mc.call_ipa(eng.h, ipa.table, N, a, q_ptr=None, Q=Q)
    assert st == mc.VC_OK and res.tolist() == [1] * P
    # and through the Python call, which repacks into ragged form
    vq = [[(scheme._pt(cxy[p, i], cinf[p, i]), int(z[p, i]), scheme.limbs_to_int(y[p, i])) for i in range(Q)] for p in range(P)]
    assert scheme.verify_multiproof_many(ipa, vq, mps) == [True] * P
    y[3, 64, 0] ^= 1
    st, res = mc.call_ipa(eng.h, ipa.table, N, a, q_ptr=None, Q=Q)
    assert st == mc.VC_OK and res.tolist() == [1, 1, 1, 0, 1]


def test_parity_kzg(eng):
    from vkzg import scheme
    N = 16
    kz = scheme.KZG(eng, N)
    counts = [1, 2, 3, 7, 63, 64, 65, 130, 2, 3]
    batch = mc.make_batch(kz, N, counts, seed=21)
    a = mc.arrays(kz, batch)
    st, res = mc.call_kzg(kz, N, a)
    assert st == mc.VC_OK and res.tolist() == [1] * 10
    for p in range(10):
        assert mc.single_kzg(kz, N, a, p) == (mc.VC_OK, 1), p
    assert scheme.verify_multiproof_many(kz, [vq for vq, _ in batch], [mp for _, mp in batch]) == [True] * 10
    claims = scheme.multiproof_claims_many(kz, [vq for vq, _ in batch], [mp["d"] for _, mp in batch])
    assert claims == [scheme.verify_multiproof(kz, vq, mp) for vq, mp in batch]
    b = mc.copy_arrays(a)
    b["ky"][4][0] ^= 1                                  # the inner y of entry 4
    mc.damage(b, "y", 6, None)                          # a query's y of entry 6
    b["kxy"][8][4:] = mc._limbs((mc._int(b["kxy"][8][4:]) + 1) % mc.P_BN254)  # entry 8's inner proof off the curve
    st, res = mc.call_kzg(kz, N, b)
    assert st == mc.VC_OK and res.tolist() == [0 if p in (4, 6, 8) else 1 for p in range(10)]
    for p in (4, 6):
        assert mc.single_kzg(kz, N, b, p) == (mc.VC_OK, 0)


def test_rejection_entry_by_entry(ipa8, batch70):
    """one thing damaged in each of 13 entries: only those verdicts become 0, and each equals the
    single call's result wherever that call returns VC_OK"""
    _, a = batch70
    b = mc.copy_arrays(a)
    valid = ipa8.g[1]
    where = mc.place(b, ("drop_last",) + mc.WELL_FORMED[:-1] + mc.MALFORMED)  # 13 entries, one kind each
    assert where["drop_last"] == 69 and len(set(where.values())) == 13
    for kind, p in where.items():
        mc.damage(b, kind, p, valid)
    st, res = mc.call_ipa(ipa8.engine.h, ipa8.table, 8, b)
    assert st == mc.VC_OK
    hit = set(where.values())
    assert res.tolist() == [0 if p in hit else 1 for p in range(70)]
    for kind, p in where.items():
        s1, r1 = mc.single_ipa(ipa8, 8, b, p)
        if kind in mc.WELL_FORMED:
            assert (s1, r1) == (mc.VC_OK, 0), kind
        elif s1 == mc.VC_OK:
            assert r1 == 0, kind
    # the claims call names the entries whose content is malformed before the inner proof is read
    st, cxy, cinf, t, bad = mc.call_claims(ipa8, 8, b)
    assert st == mc.VC_OK
    early = {where[k] for k in ("c_off_curve", "coord_ge_p", "y_ge_r", "d_off_curve")}
    assert [p for p in range(70) if bad[p]] == sorted(early)
    for p in sorted(set(range(70)) - hit):  # untouched entries: the same claim as before
        s1, oxy, oinf, ot = mc.single_claim(ipa8, 8, b, p)
        assert int(cinf[p]) == oinf and np.array_equal(cxy[p], oxy) and np.array_equal(t[p], ot), p


def test_statuses(eng, ipa8, batch70):
    import vkzg
    from vkzg import scheme
    _, full = batch70
    a = mc.tile(full, [0, 1, 2])
    h, tb = ipa8.engine.h, ipa8.table
    assert mc.call_ipa(h, tb, 8, a)[1].tolist() == [1, 1, 1]
    b = mc.copy_arrays(a)
    b["z"][-1] = 8
    st, res = mc.call_ipa(h, tb, 8, b)
    assert st == mc.VC_E_DOMAIN and res.tolist() == [0xAA] * 3
    st, _, _, t, bad = mc.call_claims(ipa8, 8, b)
    assert st == mc.VC_E_DOMAIN and not t.any() and not bad.any()
    qp = a["q_ptr"].copy()
    qp[2] = qp[1]                                                   # a proof with no query
    assert mc.call_ipa(h, tb, 8, a, q_ptr=qp)[0] == mc.VC_E_INVALID
    qp = a["q_ptr"].copy()
    qp[1], qp[2] = a["q_ptr"][2], a["q_ptr"][1]                      # descending
    assert mc.call_ipa(h, tb, 8, a, q_ptr=qp)[0] == mc.VC_E_INVALID
    assert mc.call_ipa(h, tb, 8, a, q_ptr=None, Q=4097)[0] == mc.VC_E_INVALID
    assert mc.call_ipa(h, tb, 8, a, q_ptr=None, Q=0)[0] == mc.VC_E_INVALID
    qp = np.array([0, 4097, 4098, 4099], dtype=np.uint64)          # a proof of 4097 queries
    assert mc.call_ipa(h, tb, 8, a, q_ptr=qp)[0] == mc.VC_E_INVALID
    b = dict(a)
    b["z"] = None
    assert mc.call_ipa(h, tb, 8, b)[0] == mc.VC_E_INVALID
    assert mc.call_ipa(h, tb, 6, a)[0] == mc.VC_E_INVALID            # not a power of two
    assert mc.call_ipa(h, tb, 1, a)[0] == mc.VC_E_INVALID
    assert mc.call_ipa(h, tb, 16, a)[0] == mc.VC_E_INVALID           # the table has 9 points, not 17
    assert mc.call_ipa(h, 9999, 8, a)[0] == mc.VC_E_TABLE
    bls = vkzg.Engine("bls12_381")
    try:
        st, res = mc.call_ipa(bls.h, 0, 8, a)
        assert st == mc.VC_E_INVALID and res.tolist() == [0xAA] * 3
    finally:
        bls.close()
    empty = dict(a)
    empty["P"] = 0
    assert mc.call_ipa(h, tb, 8, empty)[0] == mc.VC_OK
    assert scheme.verify_multiproof_many(ipa8, [], []) == []
    with pytest.raises(vkzg.VCError) as e:
        scheme.verify_multiproof_many(ipa8, [[(None, 8, 0)]], [{"d": None, "proof": scheme.IPAProof([None] * 3, [None] * 3, 0, 0)}])
    assert e.value.status == mc.VC_E_DOMAIN


@pytest.fixture(scope="module")
def tiles(eng):
    """8 distinct N = 4 proofs of 1-2 queries"""
    from vkzg import scheme
    ipa = scheme.IPA(eng, 4, scheme.ipa_crs(5))
    batch = mc.make_batch(ipa, 4, [1, 2, 2, 1, 2, 1, 1, 2], seed=31)
    return ipa, mc.arrays(ipa, batch)


def test_chunk_boundary_proof_cap(tiles, monkeypatch):
    """VKZG_MPV_CHUNK_P = 64: one entry more than a chunk holds, the last chunk is a damaged entry alone"""
    ipa, a8 = tiles
    cap = 64
    monkeypatch.setenv("VKZG_MPV_CHUNK_P", str(cap))
    P = cap + 1
    big = mc.tile(a8, [j % 8 for j in range(P)])
    mc.damage(big, "tip", P - 1, None)
    mc.damage(big, "y", cap - 1, None)
    st, res = mc.call_ipa(ipa.engine.h, ipa.table, 4, big)
    assert st == mc.VC_OK
    assert res.tolist() == [0 if p in (cap - 1, P - 1) else 1 for p in range(P)]
    # a cap of one entry: every chunk boundary there is
    monkeypatch.setenv("VKZG_MPV_CHUNK_P", "1")
    st, res1 = mc.call_ipa(ipa.engine.h, ipa.table, 4, big)
    assert st == mc.VC_OK and np.array_equal(res1, res)


def test_chunk_boundary_query_cap(tiles, monkeypatch):
    """VKZG_MPV_CHUNK_Q = 5: the query cap, not the proof cap, ends every chunk (3 or 4 entries each)"""
    ipa, a8 = tiles
    monkeypatch.setenv("VKZG_MPV_CHUNK_Q", "5")
    P = 27
    big = mc.tile(a8, [(5 * j) % 8 for j in range(P)])
    mc.damage(big, "y", P - 1, None)
    mc.damage(big, "tip", 9, None)
    st, res = mc.call_ipa(ipa.engine.h, ipa.table, 4, big)
    assert st == mc.VC_OK and res.tolist() == [0 if p in (9, P - 1) else 1 for p in range(P)]
    st, cxy, cinf, t, bad = mc.call_claims(ipa, 4, big)
    assert st == mc.VC_OK and not bad.any()
    for p in (0, 8, 9, 26):
        s1, oxy, oinf, ot = mc.single_claim(ipa, 4, big, p)
        assert int(cinf[p]) == oinf and np.array_equal(cxy[p], oxy) and np.array_equal(t[p], ot), p


@pytest.mark.parametrize("name", ["ipa", "kzg"])
def test_real_size_golden(eng, name):
    """the proofs of tests/golden/multiproof_256.json (N = 256, Q = 64), read only, verify to 1"""
    from vkzg import scheme

    def pt(h):
        return None if h is None else (int(h[0], 16), int(h[1], 16))

    with open(os.path.join(HERE, "golden", "multiproof_256.json")) as f:
        g = json.load(f)
    N = 256
    if name == "ipa":
        with open(os.path.join(HERE, "golden", "ipa_crs_bn254.json")) as f:
            vc = scheme.IPA(eng, N, [pt(h) for h in json.load(f)["points"]][:N + 1])
        pr = g["ipa"]["proof"]
        proof = scheme.IPAProof([pt(x) for x in pr["l"]], [pt(x) for x in pr["r"]], int(pr["tip"], 16), int(pr["y"], 16))
    else:
        vc = scheme.KZG(eng, N)
        proof = {"proof": pt(g["kzg"]["proof"]["proof"]), "y": int(g["kzg"]["proof"]["y"], 16)}
    vq = [(pt(cw), z, (int(r0, 16) + z) % scheme.R_BN254) for r0, z, cw in zip(g["r0"], g["z"], g[name]["commits"])]
    mp = {"d": pt(g[name]["d"]), "proof": proof}
    assert scheme.verify_multiproof_many(vc, [vq, vq], [mp, mp]) == [True, True]
    bad = list(vq)
    bad[10] = (bad[10][0], bad[10][1], (bad[10][2] + 1) % scheme.R_BN254)
    assert scheme.verify_multiproof_many(vc, [vq, bad], [mp, mp]) == [True, False]

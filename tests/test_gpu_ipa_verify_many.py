"""Batched IPA verification on the GPU (vc_ipa_verify_many, csrc/ipa_verify.hip): one verdict per
opening. Expected verdicts are the oracle's, recorded in tests/golden/ipa_verify_many.json
(`valid`, pyoracle.protocol.IPA.verify_point), never the code under test's; the single call
(vc_ipa_verify) must agree entry by entry. Malformed entries are False by definition. All results
are booleans: no tolerance anywhere."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK_ENV = "VKZG_IPA_VERIFY_CHUNK"  # proofs per chunk, read per call: the one knob of the batch verifier


def load(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def P(h):
    return None if h is None else (int(h[0], 16), int(h[1], 16))


@pytest.fixture(scope="module")
def eng():
    import vkzg
    e = vkzg.Engine("bn254")
    yield e
    e.close()


def _prior(prefix):
    from vkzg import scheme
    if prefix is None:
        return None
    tr = scheme.TranscriptHasher("multiproof")
    for v in prefix:
        tr.append_fr(v, "t")
    return tr


@pytest.fixture(scope="module")
def fx(eng):
    """the fixture by N, an IPA per N, and the single call's verdict per entry (computed once)"""
    from vkzg import scheme
    crs = [P(h) for h in load("ipa_crs_bn254.json")["points"]]
    by_n, ipas = {}, {}
    for e in load("ipa_verify_many.json")["entries"]:
        N = e["N"]
        if N not in ipas:
            ipas[N] = scheme.IPA(eng, N, crs[:N + 1])
        ent = {"name": e["name"], "commitment": P(e["commitment"]), "point": int(e["point"], 16),
               "proof": scheme.IPAProof([P(x) for x in e["l"]], [P(x) for x in e["r"]], int(e["tip"], 16),
                                        int(e["y"], 16)),
               "prefix": None if e["prefix"] is None else [int(v, 16) for v in e["prefix"]], "valid": e["valid"]}
        ent["single"] = ipas[N].verify_point(ent["commitment"], ent["point"], ent["proof"], _prior(ent["prefix"]))
        assert ent["single"] == ent["valid"], e["name"]
        by_n.setdefault(N, []).append(ent)
    return {"by_n": by_n, "ipa": ipas}


def _run(ipa, batch, transcripts=None):
    return ipa.verify_many([e["commitment"] for e in batch], [e["point"] for e in batch],
                           [e["proof"] for e in batch], transcripts)


def _batch(fx, n):
    """n N = 32 entries (fresh transcripts) cycling through the fixture, with tampered ones forced
    at positions 0, 63, 64 and n - 1"""
    ents = [e for e in fx["by_n"][32] if e["prefix"] is None]
    tampered = [e for e in ents if not e["valid"]]
    out = [ents[(5 * i + 1) % len(ents)] for i in range(n)]
    for k, pos in enumerate(sorted({0, 63, 64, n - 1})):
        if pos < n:
            out[pos] = tampered[(3 * k + n) % len(tampered)]
    return out


def _check_batch(fx, n):
    batch = _batch(fx, n)
    got = _run(fx["ipa"][32], batch)
    assert got == [e["valid"] for e in batch]
    assert got == [e["single"] for e in batch]
    assert not got[0] and not got[n - 1]
    if n > 2:  # (at n = 2 both positions are forced ones: nothing is left to be true)
        assert any(got)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_batch_sizes_match_oracle_and_single_call(eng, fx, n):
    """across the fixed-base engine's latency / throughput switch (64 rows) and the wave edges"""
    _check_batch(fx, n)


def test_chunk_boundary(eng, fx, monkeypatch):
    """chunks of 48: 130 proofs are 48 + 48 + 34"""
    monkeypatch.setenv(CHUNK_ENV, "48")
    _check_batch(fx, 130)
    monkeypatch.setenv(CHUNK_ENV, "1")
    _check_batch(fx, 3)
    monkeypatch.delenv(CHUNK_ENV)


@pytest.mark.parametrize("N", [256, 4])
def test_other_sizes(eng, fx, N):
    batch = fx["by_n"][N]
    assert len(batch) == (4 if N == 256 else 2)
    got = _run(fx["ipa"][N], batch)
    assert got == [e["valid"] for e in batch] == [e["single"] for e in batch]
    assert any(got) and not all(got)


def test_prior_transcripts(eng, fx):
    ents = fx["by_n"][32]
    pre = [e for e in ents if e["prefix"] is not None]
    assert [e["valid"] for e in pre] == [True, False]
    plain = [e for e in ents if e["prefix"] is None]
    batch = [plain[0], pre[0], plain[7], pre[1], plain[1]]
    got = _run(fx["ipa"][32], batch, [_prior(e["prefix"]) for e in batch])
    assert got == [e["valid"] for e in batch]
    # the same openings without their prefix: a different transcript, rejected
    assert _run(fx["ipa"][32], pre) == [False, False]
    assert _run(fx["ipa"][32], pre, [None, None]) == [False, False]


def test_malformed_entries_do_not_touch_their_neighbours(eng, fx):
    from pyoracle.curves import BN254_P, BN254_R
    from vkzg import scheme
    good = [e for e in fx["by_n"][32] if e["valid"] and e["prefix"] is None]
    g = good[4]
    pr = g["proof"]

    def variant(commitment=None, point=None, **kw):
        q = scheme.IPAProof(list(pr.l), list(pr.r), pr.tip, pr.y)
        for k, v in kw.items():
            setattr(q, k, v)
        return {"commitment": g["commitment"] if commitment is None else commitment,
                "point": g["point"] if point is None else point, "proof": q, "valid": False}
    cx, cy = g["commitment"]
    bad = [
        variant(l=[(1, 1)] + pr.l[1:]),                                       # L_0 off the curve
        variant(r=pr.r[:3] + [(pr.r[3][0] + BN254_P, pr.r[3][1])] + pr.r[4:]),  # x of R_3 >= p
        variant(tip=BN254_R),
        variant(y=pr.y + BN254_R),
        variant(point=g["point"] + BN254_R),
        variant(commitment=(cx, (cy + 1) % BN254_P)),                         # C off the curve
    ]
    batch = []
    for i, b in enumerate(bad):
        batch += [good[i], b]
    batch.append(good[6])
    got = _run(fx["ipa"][32], batch)
    assert got == [e["valid"] for e in batch]
    assert got[-1] and got[0::2] == [True] * 7 and got[1::2] == [False] * 6


def test_domain_elements_as_points(eng, fx):
    """omega^3 is a domain element that is not below N: the reference divides by zero there, the
    call fails as a whole (VC_E_DOMAIN) and writes nothing; 1 = omega^0 is below N: one-hot branch"""
    import vkzg
    from pyoracle import protocol
    from vkzg import scheme
    ipa = fx["ipa"][32]
    good = [e for e in fx["by_n"][32] if e["valid"] and e["prefix"] is None][:3]
    w3 = pow(protocol.group_gen(32), 3, scheme.R_BN254)
    points = [good[0]["point"], w3, good[2]["point"]]
    with pytest.raises(vkzg.VCError) as err:
        ipa.verify_many([e["commitment"] for e in good], points, [e["proof"] for e in good])
    assert err.value.status == -8
    arrs, ok = ipa._verify_many_arrays([e["commitment"] for e in good], points, [e["proof"] for e in good])
    assert all(ok)
    out = np.full(3, 0xAA, dtype=np.uint8)
    st = vkzg.lib().vc_ipa_verify_many(eng.h, ipa.table, 32, 3, *[a.ctypes.data_as(ctypes.c_void_p) for a in arrs],
                                       None, out.ctypes.data_as(ctypes.c_void_p))
    assert st == -8 and out.tolist() == [0xAA] * 3
    # the point 1: proved and verified on the one-hot branch
    data = scheme.LagrangeBasis([pow(11, i + 2, scheme.R_BN254) for i in range(32)])
    com = ipa.commit(data)
    pr = ipa.prove_point(com, 1, data)
    assert pr.y == data[1]
    assert ipa.verify_many([com, com], [1, 2], [pr, pr]) == [True, False]


def test_round_trip_with_the_engines_prover(eng, fx):
    from vkzg import scheme
    ipa = fx["ipa"][32]
    rng = random.Random(5)
    datas = [scheme.LagrangeBasis([rng.randrange(scheme.R_BN254) for _ in range(32)]) for _ in range(5)]
    coms = ipa.commit_batch(datas)
    pts = [3, 40, 31, 0, 12345]
    proofs = ipa.prove_batch_points(coms, pts, datas)
    assert ipa.verify_many(coms, pts, proofs) == [True] * 5
    assert ipa.verify_many(coms[1:] + coms[:1], pts, proofs) == [False] * 5
    assert ipa.verify_many([], [], []) == []

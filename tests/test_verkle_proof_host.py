"""CPU: the host side of the verkle tree proofs (include/vc_verkle.h) -- vc_verkle_proof_size (the
prover's walk, no GPU) against the statement restated over the oracle tree
(tests/verkle_proof_walk.py), the absent-key error, the argument checks of the four calls, and the
VerkleProof <-> vc_verkle_proof marshalling."""
import ctypes

import pytest

import verkle_proof_walk as vw

SEED = 23


def _trees(N):
    from pyoracle import verkle as ov
    from vkzg._lib import VCError
    from vkzg.verkle import VerkleTree
    o, items = vw.build(N, SEED, ov.VerkleTree, ov.VerklePanic)
    t, items_e = vw.build(N, SEED, VerkleTree, VCError)
    assert items == items_e
    return t, o, vw.provable(o, items)


@pytest.mark.parametrize("N", [3, 32])
def test_proof_size_matches_the_walk(N):
    t, o, kv = _trees(N)
    keys = [k for k, _ in kv]
    assert len(keys) >= 20
    for sub in (keys[:1], keys[:2], [keys[1], keys[1]], keys[::3], keys):
        w = vw.walk(o, sub)
        assert t.proof_size(sub) == (w["n_com"], w["n_queries"])
    # a repeated key adds nothing
    assert t.proof_size(keys + keys[:4]) == t.proof_size(keys)
    assert all(1 <= d <= N - 1 for d in vw.walk(o, keys)["depth"])


def test_absent_key_is_invalid():
    from vkzg._lib import VCError
    t, o, kv = _trees(3)
    for absent in (bytes([kv[0][0][0] ^ 0x55, 250, 250]),           # no such child of the root
                   kv[0][0][:2] + bytes([kv[0][0][2] ^ 1])):        # another stem / another leaf
        assert o.get_single(absent) is None and t.get_single(absent) is None
        with pytest.raises(VCError) as e:
            t.proof_size([kv[0][0], absent])
        assert e.value.status == -1


def test_null_arguments():
    import numpy as np
    import vkzg
    from vkzg.verkle import VerkleProof
    L = vkzg.lib()
    t, _, kv = _trees(3)
    k = np.frombuffer(kv[0][0], dtype=np.uint8).copy()
    kp = k.ctypes.data_as(ctypes.c_void_p)
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.vc_verkle_proof_size(None, kp, 1, ctypes.byref(a), ctypes.byref(b)) == -1
    assert L.vc_verkle_proof_size(t.h, None, 1, ctypes.byref(a), ctypes.byref(b)) == -1
    assert L.vc_verkle_proof_size(t.h, kp, 0, ctypes.byref(a), ctypes.byref(b)) == -1
    assert L.vc_verkle_proof_size(t.h, kp, 1, None, ctypes.byref(b)) == -1
    assert L.vc_verkle_proof_size(t.h, kp, 1, ctypes.byref(a), ctypes.byref(b)) == 0
    buf, keep = VerkleProof._alloc(1, a.value, False)
    xy = np.zeros(8, dtype=np.uint64)
    inf = np.zeros(1, dtype=np.uint8)
    res = ctypes.c_int(7)
    P = ctypes.c_void_p
    # no context: every device call refuses before it touches anything
    assert L.vc_verkle_prove(None, 1, 0, t.h, kp, 1, xy.ctypes.data_as(P), inf.ctypes.data_as(P), ctypes.byref(buf)) == -1
    assert L.vc_verkle_proof_queries(None, 0, t.h, kp, 1, 0, None, None, None, None, None, ctypes.byref(a)) == -1
    v = np.zeros(32, dtype=np.uint8)
    assert L.vc_verkle_verify(None, 1, 0, None, 3, xy.ctypes.data_as(P), 0, kp, v.ctypes.data_as(P), 1,
                              ctypes.byref(buf), ctypes.byref(res)) == -1
    assert res.value == 0


def test_verkle_proof_round_trip():
    from vkzg.scheme import IPAProof
    from vkzg.verkle import VerkleProof
    pts = [(1, 2), None, (5, 7 << 200), ((1 << 253) + 9, 11)]
    kz = VerkleProof([1, 2, 31], pts, (3, 4), {"proof": (8, 9), "y": (1 << 250) + 5})
    ip = VerkleProof([2], pts[:1], None,
                     IPAProof([(i + 1, i + 2) for i in range(8)], [None] + [(i + 3, i + 4) for i in range(7)], 12345, 1 << 200))
    for p, ipa in ((kz, False), (ip, True)):
        b, keep = p._to()
        assert b.n_keys == len(p.depth) and b.n_com == len(p.commitments)
        assert VerkleProof._from(b, keep, ipa).as_dict() == p.as_dict()

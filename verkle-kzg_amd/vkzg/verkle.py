"""VerkleTree over the engine (include/vc_verkle.h), mirroring /root/reference/verkle-tree/src
(lib.rs VerkleTree<N, u8, VC, U256>; node.rs Node). Keys: N bytes; values: 32 bytes.
The tree lives in libvkzg.so (C++); commitments are level-batched on the GPU against any
BN254 table (KZG Lagrange SRS from KZG(...).table, or an IPA CRS from IPA(...).table)."""
import ctypes

import numpy as np

from ._lib import VCError, check, lib
from .engine import ints_to_limbs, limbs_to_int
from .scheme import IPA, IPAProof, _M256, _ProofBuf, _pt, _pt_arrays


def _b(x):
    a = np.frombuffer(bytes(x), dtype=np.uint8).copy()
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _keys_array(keys, key_len):
    for k in keys:
        assert len(k) == key_len
    return np.frombuffer(b"".join(bytes(k) for k in keys), dtype=np.uint8).copy()


class _VerkleProofBuf(ctypes.Structure):
    """vc_verkle_proof (include/vc_verkle.h)"""
    _fields_ = [("n_keys", ctypes.c_size_t), ("depth", ctypes.c_void_p), ("n_com", ctypes.c_size_t),
                ("com_xy", ctypes.c_void_p), ("com_inf", ctypes.c_void_p), ("d_xy", ctypes.c_uint64 * 8),
                ("d_inf", ctypes.c_uint8), ("ipa", _ProofBuf), ("kzg_proof_xy", ctypes.c_uint64 * 8),
                ("kzg_proof_inf", ctypes.c_uint8), ("kzg_y", ctypes.c_uint64 * 4)]


class VerkleProof:
    """A tree proof (include/vc_verkle.h): depth per key, the path commitments other than the root
    (points, None = identity), the multiproof's D and the inner proof -- an IPAProof, or the KZG
    {"proof": point, "y": int}."""

    def __init__(self, depth, commitments, d, inner):
        self.depth, self.commitments, self.d, self.inner = list(depth), list(commitments), d, inner

    def as_dict(self):
        inner = self.inner if isinstance(self.inner, dict) else self.inner.as_dict()
        return {"depth": self.depth, "commitments": self.commitments, "d": self.d, "inner": inner}

    @staticmethod
    def _alloc(n_keys, n_com, ipa):
        """an empty vc_verkle_proof with room for n_com commitments -> (struct, the arrays it points to)"""
        keep = {"depth": np.zeros(max(n_keys, 1), dtype=np.uint8),
                "com_xy": np.zeros((max(n_com, 1), 8), dtype=np.uint64),
                "com_inf": np.zeros(max(n_com, 1), dtype=np.uint8)}
        b = _VerkleProofBuf()
        b.n_keys, b.n_com = n_keys, n_com
        b.depth, b.com_xy, b.com_inf = (keep[k].ctypes.data for k in ("depth", "com_xy", "com_inf"))
        if ipa:
            b.ipa, keep["ipa"] = IPAProof._alloc(8)
        return b, keep

    @staticmethod
    def _from(b, keep, ipa):
        coms = [_pt(keep["com_xy"][k], keep["com_inf"][k]) for k in range(b.n_com)]
        d = _pt(np.array(b.d_xy[:], dtype=np.uint64), b.d_inf)
        if ipa:
            inner = IPAProof._from(b.ipa, keep["ipa"])
        else:
            inner = {"proof": _pt(np.array(b.kzg_proof_xy[:], dtype=np.uint64), b.kzg_proof_inf),
                     "y": int.from_bytes(bytes(b.kzg_y), "little")}
        return VerkleProof([int(v) for v in keep["depth"][:b.n_keys]], coms, d, inner)

    def _to(self):
        """the vc_verkle_proof of this proof -> (struct, the arrays it points to)"""
        ipa = not isinstance(self.inner, dict)
        b, keep = VerkleProof._alloc(len(self.depth), len(self.commitments), False)
        keep["depth"][:len(self.depth)] = self.depth
        if self.commitments:
            keep["com_xy"][:], keep["com_inf"][:] = _pt_arrays(self.commitments)
        xy, inf = _pt_arrays([self.d])
        b.d_xy[:] = [int(v) for v in xy[0]]
        b.d_inf = int(inf[0])
        if ipa:
            b.ipa, keep["ipa"] = self.inner._to()
        else:
            xy, inf = _pt_arrays([self.inner["proof"]])
            b.kzg_proof_xy[:] = [int(v) for v in xy[0]]
            b.kzg_proof_inf = int(inf[0])
            b.kzg_y[:] = [int(v) for v in ints_to_limbs([int(self.inner["y"]) & _M256], 4)[0]]
        return b, keep


def verify(engine, vc, key_len, root, keys, values, proof):
    """vc_verkle_verify: do `keys` map to `values` under `root` (a point, None = identity)?
    vc: a scheme.IPA (its table) or a scheme.KZG (its verifying key). Needs no tree."""
    ipa = isinstance(vc, IPA)
    for v in values:
        assert len(v) == 32
    k = _keys_array(keys, key_len)
    v = np.frombuffer(b"".join(bytes(x) for x in values), dtype=np.uint8).copy()
    rxy, rinf = _pt_arrays([root])
    b, keep = proof._to()
    res = ctypes.c_int()
    check(lib().vc_verkle_verify(engine.h, 0 if ipa else 1, vc.table, None if ipa else vc.verifying_key().h, key_len,
                                 rxy.ctypes.data_as(ctypes.c_void_p), int(rinf[0]), k.ctypes.data_as(ctypes.c_void_p),
                                 v.ctypes.data_as(ctypes.c_void_p), len(keys), ctypes.byref(b), ctypes.byref(res)),
          "vc_verkle_verify")
    return bool(res.value)


class VerkleTree:
    def __init__(self, key_len):
        self.N = key_len
        self.h = lib().vc_verkle_new(key_len)
        if not self.h:
            raise VCError(-1, "vc_verkle_new")

    def __del__(self):
        if getattr(self, "h", None):
            try:
                lib().vc_verkle_free(self.h)
            except TypeError:  # interpreter shutdown: module globals already cleared
                pass
            self.h = None

    def insert_single(self, key, value):
        """lib.rs:112-116; VCError(VC_E_INVALID) where the reference panics."""
        assert len(key) == self.N and len(value) == 32
        k, kp = _b(key)
        v, vp = _b(value)
        check(lib().vc_verkle_insert(self.h, kp, vp), "vc_verkle_insert")

    def get_single(self, key):
        k, kp = _b(key)
        out = np.zeros(32, dtype=np.uint8)
        found = ctypes.c_int()
        check(lib().vc_verkle_get(self.h, kp, ctypes.c_void_p(out.ctypes.data), ctypes.byref(found)), "vc_verkle_get")
        return out.tobytes() if found.value else None

    def path_to_stem(self, key):
        """[(prefix, unit)] as node.rs:97-120; VCError for InvalidPath."""
        k, kp = _b(key)
        units = np.zeros(self.N, dtype=np.uint8)
        n = ctypes.c_size_t()
        check(lib().vc_verkle_path(self.h, kp, self.N, ctypes.c_void_p(units.ctypes.data), ctypes.byref(n)),
              "vc_verkle_path")
        return [(tuple(key[:d + 1]), key[d]) for d in range(n.value)]

    def debug_ext_stage(self, reps=5):
        """median us of the device path's extension host stage over every extension (no GPU)"""
        us = ctypes.c_double()
        check(lib().vc_verkle_debug_ext_stage(self.h, reps, ctypes.byref(us)), "vc_verkle_debug_ext_stage")
        return us.value

    def debug_nodes(self):
        """per node id: (type 0 internal / 1 extension, level, committed item as int)"""
        n = ctypes.c_size_t()
        check(lib().vc_verkle_debug_nodes(self.h, 0, None, None, None, ctypes.byref(n)), "vc_verkle_debug_nodes")
        m = n.value
        ty = np.zeros(m, dtype=np.uint8)
        lv = np.zeros(m, dtype=np.int32)
        it = np.zeros((m, 4), dtype=np.uint64)
        check(lib().vc_verkle_debug_nodes(self.h, m, ctypes.c_void_p(ty.ctypes.data), ctypes.c_void_p(lv.ctypes.data),
                                          ctypes.c_void_p(it.ctypes.data), ctypes.byref(n)), "vc_verkle_debug_nodes")
        return [(int(ty[i]), int(lv[i]), limbs_to_int(it[i])) for i in range(m)]

    def stats(self):
        a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        check(lib().vc_verkle_stats(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "vc_verkle_stats")
        return {"internal": a.value, "extension": b.value, "dirty": c.value}

    def commitment(self, engine, table):
        """lib.rs:127-129: root commitment (canonical affine (x, y) or None)."""
        xy = np.zeros(8, dtype=np.uint64)
        inf = np.zeros(1, dtype=np.uint8)
        check(lib().vc_verkle_commitment(engine.h, table, self.h, ctypes.c_void_p(xy.ctypes.data),
                                         ctypes.c_void_p(inf.ctypes.data)), "vc_verkle_commitment")
        return None if inf[0] else (limbs_to_int(xy[:4]), limbs_to_int(xy[4:]))

    def proof_size(self, keys):
        """(commitments, queries) of a proof of `keys` (host only); VCError for an absent key"""
        k = _keys_array(keys, self.N)
        nc, nq = ctypes.c_size_t(), ctypes.c_size_t()
        check(lib().vc_verkle_proof_size(self.h, k.ctypes.data_as(ctypes.c_void_p), len(keys), ctypes.byref(nc),
                                         ctypes.byref(nq)), "vc_verkle_proof_size")
        return nc.value, nq.value

    def prove(self, engine, vc, keys):
        """vc_verkle_prove: (root, VerkleProof) for keys present in the tree; vc: the scheme.IPA
        (256) or scheme.KZG (256) the tree is committed with. Commits a dirty tree first."""
        ipa = isinstance(vc, IPA)
        n_com, _ = self.proof_size(keys)
        k = _keys_array(keys, self.N)
        b, keep = VerkleProof._alloc(len(keys), n_com, ipa)
        rxy = np.zeros(8, dtype=np.uint64)
        rinf = np.zeros(1, dtype=np.uint8)
        check(lib().vc_verkle_prove(engine.h, 0 if ipa else 1, vc.table, self.h, k.ctypes.data_as(ctypes.c_void_p),
                                    len(keys), rxy.ctypes.data_as(ctypes.c_void_p), rinf.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.byref(b)), "vc_verkle_prove")
        return _pt(rxy, rinf[0]), VerkleProof._from(b, keep, ipa)

    def proof_queries(self, engine, table, keys, rows=False):
        """diagnostic (vc_verkle_proof_queries): the prover's query list as (commitment limbs (Q, 8),
        identity flags (Q,), z (Q,), y limbs (Q, 4)[, dense rows (Q, 256, 4)]) numpy arrays"""
        k = _keys_array(keys, self.N)
        _, q = self.proof_size(keys)
        cxy = np.zeros((q, 8), dtype=np.uint64)
        cinf = np.zeros(q, dtype=np.uint8)
        z = np.zeros(q, dtype=np.uint64)
        y = np.zeros((q, 4), dtype=np.uint64)
        data = np.zeros((q, 256, 4), dtype=np.uint64) if rows else None
        cnt = ctypes.c_size_t()
        P = ctypes.c_void_p
        check(lib().vc_verkle_proof_queries(engine.h, table, self.h, k.ctypes.data_as(P), len(keys), q,
                                            cxy.ctypes.data_as(P), cinf.ctypes.data_as(P), z.ctypes.data_as(P),
                                            y.ctypes.data_as(P), data.ctypes.data_as(P) if rows else None,
                                            ctypes.byref(cnt)), "vc_verkle_proof_queries")
        assert cnt.value == q
        return (cxy, cinf, z, y, data) if rows else (cxy, cinf, z, y)

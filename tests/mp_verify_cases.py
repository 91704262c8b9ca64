"""Cases of the multiproof many-verifier (tests/test_gpu_multiproof_verify_many.py): batches of
multiproofs made with vc_multiproof_prove, their flat arrays in the layout
vc_multiproof_verify_many_* reads, the single calls they are compared with, and the damage done to
single entries. Nothing here touches the GPU until a function is called with a scheme object."""
import ctypes
import random

import numpy as np

QCOUNTS = (1, 2, 3, 7, 63, 64, 65, 130)  # below, at and above a block of 64 lanes; the 8 / 64 lane split at 32
P_BN254 = 21888242871839275222246405745257275088696311157297823662689037894645226208583
ALL_ONES = (1 << 256) - 1
VC_OK, VC_E_INVALID, VC_E_TABLE, VC_E_DOMAIN = 0, -1, -4, -8


def counts_for(P, seed, forced=None):
    rng = random.Random(seed)
    c = [QCOUNTS[i % len(QCOUNTS)] for i in range(P)]
    rng.shuffle(c)
    for k, v in (forced or {}).items():
        c[k] = v
    return c


def make_batch(vc, N, counts, seed):
    """len(counts) multiproofs over a pool of 6 data vectors (one all zero: its commitment is the
    identity), so commitments repeat inside a proof, and z drawn with repeats -> [(vqueries, mp)]"""
    from vkzg import scheme
    rng = random.Random(seed)
    pool = [scheme.LagrangeBasis([rng.randrange(scheme.R_BN254) for _ in range(N)]) for _ in range(5)]
    pool.append(scheme.LagrangeBasis([0] * N))
    coms = vc.commit_batch(pool) if hasattr(vc, "commit_batch") else [vc.commit(d) for d in pool]
    assert coms[5] is None
    out = []
    for q in counts:
        queries = []
        for i in range(q):
            k = rng.randrange(6)
            z = queries[-1][2] if (i and rng.randrange(4) == 0) else rng.randrange(N)
            queries.append((pool[k], coms[k], z, pool[k][z]))
        mp = scheme.prove_multiproof(vc, queries)
        out.append(([(c, z, y) for _, c, z, y in queries], mp))
    return out


def arrays(vc, batch):
    """the flat arrays of a batch: the queries, D, and the inner proofs of the scheme"""
    from vkzg import scheme
    qpp = [vq for vq, _ in batch]
    q_ptr, cxy, cinf, z, y = scheme._queries_many(qpp)
    dxy, dinf = scheme._pt_arrays_many([mp["d"] for _, mp in batch])
    a = {"P": len(batch), "q_ptr": q_ptr, "cxy": cxy, "cinf": cinf, "z": z, "y": y, "dxy": dxy, "dinf": dinf}
    if isinstance(vc, scheme.IPA):
        P = len(batch)
        (_, _, _, lxy, linf, rxy, rinf, tips, ys), good = vc._verify_many_arrays([None] * P, [0] * P,
                                                                                 [mp["proof"] for _, mp in batch])
        assert all(good)
        a.update(lxy=lxy, linf=linf, rxy=rxy, rinf=rinf, tip=tips, iy=ys)
    else:
        kxy, kinf = scheme._pt_arrays_many([mp["proof"]["proof"] for _, mp in batch])
        ky = scheme.ints_to_limbs([int(mp["proof"]["y"]) for _, mp in batch], 4)
        a.update(kxy=kxy, kinf=kinf, ky=ky)
    return {k: (np.ascontiguousarray(v).copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


def copy_arrays(a):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


def tile(a, idx):
    """the arrays of the batch whose entry j is entry idx[j] of a"""
    qp = a["q_ptr"].astype(np.int64)
    qsel = np.concatenate([np.arange(qp[i], qp[i + 1]) for i in idx])
    out = {"P": len(idx)}
    out["q_ptr"] = np.concatenate([[0], np.cumsum([qp[i + 1] - qp[i] for i in idx])]).astype(np.uint64)
    for k in ("cxy", "cinf", "z", "y"):
        out[k] = np.ascontiguousarray(a[k][qsel])
    idx = np.asarray(idx)
    for k in ("dxy", "dinf", "tip", "iy", "kxy", "kinf", "ky"):
        if k in a:
            out[k] = np.ascontiguousarray(a[k][idx])
    if "lxy" in a:
        K = a["lxy"].shape[0] // a["P"]
        rows = (idx[:, None] * K + np.arange(K)[None, :]).reshape(-1)
        for k in ("lxy", "linf", "rxy", "rinf"):
            out[k] = np.ascontiguousarray(a[k][rows])
    return out


def _ptr(x):
    from vkzg import scheme
    return None if x is None else scheme._p(x)


def call_claims(vc, N, a, q_ptr="own", Q=0):
    from vkzg._lib import lib
    P = a["P"]
    oxy = np.zeros((max(P, 1), 8), dtype=np.uint64)
    oinf = np.zeros(max(P, 1), dtype=np.uint8)
    t = np.zeros((max(P, 1), 4), dtype=np.uint64)
    bad = np.zeros(max(P, 1), dtype=np.uint8)
    qp = a["q_ptr"] if isinstance(q_ptr, str) else q_ptr
    st = lib().vc_multiproof_claims_many(vc.engine.h, N, P, _ptr(qp), Q, _ptr(a["cxy"]), _ptr(a["cinf"]), _ptr(a["z"]),
                                         _ptr(a["y"]), _ptr(a["dxy"]), _ptr(a["dinf"]), _ptr(oxy), _ptr(oinf), _ptr(t),
                                         _ptr(bad))
    return st, oxy, oinf, t, bad


def call_ipa(engine_h, table, N, a, q_ptr="own", Q=0, fill=0xAA):
    from vkzg._lib import lib
    P = a["P"]
    res = np.full(max(P, 1), fill, dtype=np.uint8)
    qp = a["q_ptr"] if isinstance(q_ptr, str) else q_ptr
    st = lib().vc_multiproof_verify_many_ipa(engine_h, table, N, P, _ptr(qp), Q, _ptr(a["cxy"]), _ptr(a["cinf"]),
                                             _ptr(a["z"]), _ptr(a["y"]), _ptr(a["dxy"]), _ptr(a["dinf"]), _ptr(a["lxy"]),
                                             _ptr(a["linf"]), _ptr(a["rxy"]), _ptr(a["rinf"]), _ptr(a["tip"]),
                                             _ptr(a["iy"]), _ptr(res))
    return st, res


def call_kzg(vc, N, a, fill=0xAA):
    from vkzg._lib import lib
    P = a["P"]
    res = np.full(max(P, 1), fill, dtype=np.uint8)
    st = lib().vc_multiproof_verify_many_kzg(vc.engine.h, vc.verifying_key().h, N, P, _ptr(a["q_ptr"]), 0, _ptr(a["cxy"]),
                                             _ptr(a["cinf"]), _ptr(a["z"]), _ptr(a["y"]), _ptr(a["dxy"]), _ptr(a["dinf"]),
                                             _ptr(a["kxy"]), _ptr(a["kinf"]), _ptr(a["ky"]), _ptr(res))
    return st, res


def _slice(a, p):
    lo, hi = int(a["q_ptr"][p]), int(a["q_ptr"][p + 1])
    return hi - lo, tuple(np.ascontiguousarray(a[k][lo:hi]) for k in ("cxy", "cinf", "z", "y"))


def single_claim(vc, N, a, p):
    """vc_multiproof_kzg_claim of entry p -> (status, c_xy, c_inf, t)"""
    from vkzg._lib import lib
    Q, (cxy, cinf, z, y) = _slice(a, p)
    oxy = np.zeros(8, dtype=np.uint64)
    oinf = np.zeros(1, dtype=np.uint8)
    t = np.zeros(4, dtype=np.uint64)
    dxy = np.ascontiguousarray(a["dxy"][p])
    st = lib().vc_multiproof_kzg_claim(vc.engine.h, N, Q, _ptr(cxy), _ptr(cinf), _ptr(z), _ptr(y), _ptr(dxy),
                                       int(a["dinf"][p]), _ptr(oxy), _ptr(oinf), _ptr(t))
    return st, oxy, int(oinf[0]), t


def single_ipa(vc, N, a, p):
    """vc_multiproof_verify_ipa of entry p, straight from the flat arrays -> (status, result)"""
    from vkzg import scheme
    from vkzg._lib import lib
    Q, (cxy, cinf, z, y) = _slice(a, p)
    K = a["lxy"].shape[0] // a["P"]
    rows = slice(p * K, (p + 1) * K)
    keep = [np.ascontiguousarray(a[k][rows]) for k in ("lxy", "linf", "rxy", "rinf")]
    b = scheme._ProofBuf(K, keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data)
    b.tip[:] = [int(v) for v in a["tip"][p]]
    b.y[:] = [int(v) for v in a["iy"][p]]
    dxy = np.ascontiguousarray(a["dxy"][p])
    res = ctypes.c_int(-1)
    st = lib().vc_multiproof_verify_ipa(vc.engine.h, vc.table, N, Q, _ptr(cxy), _ptr(cinf), _ptr(z), _ptr(y), _ptr(dxy),
                                        int(a["dinf"][p]), ctypes.byref(b), ctypes.byref(res))
    return st, res.value


def single_kzg(vc, N, a, p):
    from vkzg._lib import lib
    Q, (cxy, cinf, z, y) = _slice(a, p)
    res = ctypes.c_int(-1)
    dxy, kxy, ky = (np.ascontiguousarray(a[k][p]) for k in ("dxy", "kxy", "ky"))
    st = lib().vc_multiproof_verify_kzg(vc.engine.h, vc.verifying_key().h, N, Q, _ptr(cxy), _ptr(cinf), _ptr(z), _ptr(y),
                                        _ptr(dxy), int(a["dinf"][p]), _ptr(kxy), int(a["kinf"][p]), _ptr(ky),
                                        ctypes.byref(res))
    return st, res.value


# ---------------------------------------------------------------- damage
def _limbs(v):
    return [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]


def _int(row):
    return sum(int(x) << (64 * j) for j, x in enumerate(row))


def _first_real(a, p):
    """a query of entry p whose commitment is not the identity"""
    for i in range(int(a["q_ptr"][p]), int(a["q_ptr"][p + 1])):
        if not a["cinf"][i]:
            return i
    raise AssertionError("entry %d has identity commitments only" % p)


def damage(a, kind, p, valid_point):
    """damages one thing of entry p in place; valid_point: a point on the curve the batch does not use there"""
    R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    lo, hi = int(a["q_ptr"][p]), int(a["q_ptr"][p + 1])
    vxy = _limbs(valid_point[0]) + _limbs(valid_point[1]) if valid_point else None
    if kind == "y":
        a["y"][lo] = _limbs((_int(a["y"][lo]) + 1) % R)
    elif kind == "c_swap":
        i = _first_real(a, p)
        a["cxy"][i] = vxy
    elif kind == "z_swap":
        pairs = [(i, j) for i in range(lo, hi) for j in range(i + 1, hi)
                 if a["z"][i] != a["z"][j] and (a["cinf"][i], tuple(a["cxy"][i]), tuple(a["y"][i]))
                 != (a["cinf"][j], tuple(a["cxy"][j]), tuple(a["y"][j]))]
        assert pairs, "entry %d has no two queries whose exchange changes it" % p
        i, j = pairs[0]
        a["z"][i], a["z"][j] = a["z"][j], a["z"][i]
    elif kind == "d":
        a["dxy"][p] = vxy
        a["dinf"][p] = 0
    elif kind == "tip":
        a["tip"][p] = _limbs((_int(a["tip"][p]) + 1) % R)
    elif kind == "l":
        K = a["lxy"].shape[0] // a["P"]
        a["lxy"][p * K + K - 1] = vxy
        a["linf"][p * K + K - 1] = 0
    elif kind == "drop_last":
        assert p == a["P"] - 1 and hi - lo >= 2
        a["q_ptr"][p + 1] -= 1
    elif kind == "c_off_curve":
        i = _first_real(a, p)
        a["cxy"][i][4:] = _limbs((_int(a["cxy"][i][4:]) + 1) % P_BN254)
    elif kind == "coord_ge_p":
        i = _first_real(a, p)
        a["cxy"][i][:4] = _limbs(ALL_ONES)
    elif kind == "y_ge_r":
        a["y"][hi - 1] = _limbs(ALL_ONES)
    elif kind == "tip_ge_r":
        a["tip"][p] = _limbs(R)
    elif kind == "d_off_curve":
        assert not a["dinf"][p]
        a["dxy"][p][4:] = _limbs((_int(a["dxy"][p][4:]) + 1) % P_BN254)
    elif kind == "r_ge_p":
        K = a["rxy"].shape[0] // a["P"]
        a["rxy"][p * K][4:] = _limbs(P_BN254)
        a["rinf"][p * K] = 0
    else:
        raise ValueError(kind)


def suits(a, kind, p):
    """whether entry p has what the damage `kind` needs (a commitment or a D that is not the identity,
    two queries whose exchange changes the proof, a second query to drop)"""
    lo, hi = int(a["q_ptr"][p]), int(a["q_ptr"][p + 1])
    if kind in ("c_swap", "c_off_curve", "coord_ge_p"):
        return not a["cinf"][lo:hi].all()
    if kind == "d_off_curve":
        return not a["dinf"][p]
    if kind == "z_swap":
        return any(a["z"][i] != a["z"][j] and (a["cinf"][i], tuple(a["cxy"][i]), tuple(a["y"][i]))
                   != (a["cinf"][j], tuple(a["cxy"][j]), tuple(a["y"][j])) for i in range(lo, hi) for j in range(i + 1, hi))
    if kind == "drop_last":
        return p == a["P"] - 1 and hi - lo >= 2
    return True


def place(a, kinds):
    """kind -> entry: the first entry not yet taken that suits each kind, in order"""
    where, taken = {}, set()
    for kind in kinds:
        where[kind] = next(p for p in (range(a["P"] - 1, -1, -1) if kind == "drop_last" else range(a["P"]))
                           if p not in taken and suits(a, kind, p))
        taken.add(where[kind])
    return where


WELL_FORMED = ("y", "c_swap", "z_swap", "d", "tip", "l", "drop_last")
MALFORMED = ("c_off_curve", "coord_ge_p", "y_ge_r", "tip_ge_r", "d_off_curve", "r_ge_p")

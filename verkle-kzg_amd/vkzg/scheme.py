"""Reference-shaped VectorCommitment API over the HIP engine (include/vc_scheme.h).

Mirrors /root/reference/vector-commit/src: `IPA` (ipa/mod.rs), `KZG` (kzg/mod.rs),
`LagrangeBasis` (lagrange_basis.rs), `TranscriptHasher` (transcript.rs),
`prove_multiproof` / `verify_multiproof` / `verify_multiproof_kzg` (multiproof.rs), `to_data_item`
(lib.rs:56-67). KZG openings are verified with pairings through `KZGVerifyingKey`; subvector proofs
(`KZG.prove_subvector`, the reference's prove_batch) through `KZGSubvectorKey`.
Same names, argument meaning and error behaviour (errors raise `VCError` where the Rust
returns Err or panics). Curve: BN254 G1 (the reference's only instantiation); `KZG`,
`KZGVerifyingKey`, `kzg_g2_from_secret`, `kzg_batch_challenge` and `pairing_check` also work on
BLS12-381 (an `Engine("bls12_381")` / `curve="bls12_381"`; G1 coordinates are then 6 u64 limbs).
Points are canonical affine (x, y) tuples, the identity is None; field elements are ints.
All arithmetic runs in libvkzg.so; this module only marshals.
"""
import ctypes

import numpy as np

from ._lib import VCError, check, lib
from .engine import Engine, ints_to_limbs, limbs_to_int

R_BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R_BLS12_381 = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
_P = ctypes.c_void_p
# the curves with a pairing: scalar field, u64 limbs of a base-field coordinate, the ABI's curve id
_PAIRING_CURVES = {"bn254": (R_BN254, 4, 0), "bls12_381": (R_BLS12_381, 6, 1)}


def _curve_params(curve):
    if curve not in _PAIRING_CURVES:
        raise ValueError(f"no pairing on curve {curve!r}")
    return _PAIRING_CURVES[curve]


def _p(a):
    # data_as keeps a reference to the array in the pointer object: callers pass temporaries
    # (e.g. _p(_fr(point))), and a bare c_void_p(a.ctypes.data) let the array be freed before the
    # foreign call read it -- harmless single-threaded by luck, garbage once another thread
    # reused the memory (tests/test_gpu_threads.py found it)
    return a.ctypes.data_as(ctypes.c_void_p)


def _fr(x, r=R_BN254):
    return ints_to_limbs([int(x) % r], 4)[0].copy()


_M256 = (1 << 256) - 1


def _pt_arrays(pts, nl=4):
    """[(x, y) | None] -> ((n, 2 nl) u64 limbs, (n,) identity flags): one bytes buffer for all points
    (per-point numpy assignments cost ~10 us per call of the IPA prover's Python mirror). nl: u64
    limbs of a coordinate (4: BN254, 6: BLS12-381)"""
    n = len(pts)
    cb = 8 * nl
    mask = (1 << (8 * cb)) - 1
    buf = bytearray(2 * cb * n)
    inf = np.zeros(n, dtype=np.uint8)
    for i, P in enumerate(pts):
        if P is None:
            inf[i] = 1
        else:
            buf[2 * cb * i:2 * cb * i + cb] = (int(P[0]) & mask).to_bytes(cb, "little")
            buf[2 * cb * i + cb:2 * cb * (i + 1)] = (int(P[1]) & mask).to_bytes(cb, "little")
    xy = np.frombuffer(buf, dtype="<u8").reshape(n, 2 * nl).astype(np.uint64)
    return xy, inf


def _pt_arrays_many(pts):
    """_pt_arrays for long lists (verify_many: n x (1 + 2 log2 N) points): one join over the
    coordinates' bytes, no per-point buffer assignment"""
    n = len(pts)
    zero = bytes(64)
    buf = b"".join(zero if P is None else (int(P[0]) & _M256).to_bytes(32, "little") + (int(P[1]) & _M256).to_bytes(32, "little")
                   for P in pts)
    inf = np.fromiter((P is None for P in pts), dtype=np.uint8, count=n)
    return np.frombuffer(buf, dtype="<u8").reshape(n, 8).astype(np.uint64), inf


def _pt(xy, inf):
    if inf:
        return None
    nl = len(xy) // 2
    return (limbs_to_int(xy[:nl]), limbs_to_int(xy[nl:2 * nl]))


# ---------------------------------------------------------------- transcript.rs
class TranscriptHasher:
    def __init__(self, label, _h=None):
        self.h = _h if _h is not None else lib().vc_transcript_new(label.encode())

    def __del__(self):
        if getattr(self, "h", None):
            lib().vc_transcript_free(self.h)
            self.h = None

    def clone(self):
        return TranscriptHasher(None, lib().vc_transcript_clone(self.h))

    def append_point(self, P, label):
        xy, inf = _pt_arrays([P])
        check(lib().vc_transcript_append_point(self.h, _p(xy), int(inf[0]), label.encode()), "append_point")

    def append_fr(self, x, label):
        check(lib().vc_transcript_append_fr(self.h, _p(_fr(x)), label.encode()), "append_fr")

    def append_usize(self, z, label):
        check(lib().vc_transcript_append_u64(self.h, int(z), label.encode()), "append_usize")

    def digest(self, label, clear=True):
        out = np.zeros(4, dtype=np.uint64)
        check(lib().vc_transcript_digest(self.h, label.encode(), _p(out)), "digest")
        return limbs_to_int(out)


def hash_to_field(msg, dst):
    m = np.frombuffer(bytes(msg) or b"\0", dtype=np.uint8).copy()
    d = np.frombuffer(bytes(dst) or b"\0", dtype=np.uint8).copy()
    out = np.zeros(4, dtype=np.uint64)
    check(lib().vc_hash_to_field(_p(m), len(msg), _p(d), len(dst), _p(out)), "hash_to_field")
    return limbs_to_int(out)


def point_compress(P):
    xy, inf = _pt_arrays([P])
    out = np.zeros(32, dtype=np.uint8)
    check(lib().vc_point_compress(_p(xy), int(inf[0]), _p(out)), "point_compress")
    return out.tobytes()


def to_data_item(engine, pts):
    """VCCommitment::to_data_item for a batch of points (device)."""
    xy, inf = _pt_arrays(pts)
    out = np.zeros((len(pts), 4), dtype=np.uint64)
    check(lib().vc_to_data_item_batch(engine.h, _p(xy), _p(inf), len(pts), _p(out)), "to_data_item")
    return [limbs_to_int(r) for r in out]


def ipa_crs(num, seed=b"eth_verkle_oct_2021", max_=256):
    """IPAPointGenerator::gen (ipa_point_generator.rs:51-67); VCError(VC_E_RANGE) = OutOfBounds."""
    s = np.frombuffer(seed, dtype=np.uint8).copy()
    out = np.zeros((max(num, 1), 8), dtype=np.uint64)
    check(lib().vc_ipa_crs(_p(s), len(seed), max_, num, _p(out)), "ipa_crs")
    return [_pt(out[i], 0) for i in range(num)]


# ---------------------------------------------------------------- lagrange_basis.rs
class LagrangeBasis:
    """Evaluations over a radix-2 domain (possibly shorter than it: `max`)."""

    def __init__(self, evals, domain_size=None, r=R_BN254):
        # a tuple: the limbs below are cached per padded length, so the values must not change
        self.evals = tuple(int(e) % r for e in evals)
        self._limbs = {}
        ds = 1
        while ds < len(self.evals):
            ds <<= 1
        self.dsize = domain_size if domain_size is not None else ds

    @classmethod
    def from_vec(cls, data):
        return cls(data)

    def __getitem__(self, i):
        return self.evals[i]

    def max(self):
        return len(self.evals) - 1

    def limbs(self, n=None):
        """(max(len, n), 4) canonical u64 limbs, converted once per n (read-only array)."""
        arr = self._limbs.get(n)
        if arr is None:
            arr = ints_to_limbs(self.evals, 4)
            if n is not None and arr.shape[0] < n:
                arr = np.vstack([arr, np.zeros((n - arr.shape[0], 4), dtype=np.uint64)])
            arr = np.ascontiguousarray(arr)
            arr.flags.writeable = False
            self._limbs[n] = arr
        return arr


# ---------------------------------------------------------------- proofs
class _ProofBuf(ctypes.Structure):
    _fields_ = [("rounds", ctypes.c_size_t), ("l_xy", _P), ("l_inf", _P), ("r_xy", _P), ("r_inf", _P),
                ("tip", ctypes.c_uint64 * 4), ("y", ctypes.c_uint64 * 4)]


class IPAProof:
    def __init__(self, l, r, tip, y):
        self.l, self.r, self.tip, self.y = l, r, tip, y

    def as_dict(self):
        return {"l": self.l, "r": self.r, "tip": self.tip, "y": self.y}

    @staticmethod
    def _alloc(rounds):
        # one buffer, four views (the caller keeps `arrs`, hence the buffer, alive while the struct's
        # raw pointers are in use): four allocations and four data_as pointers cost ~19 us a call
        k = rounds
        raw = np.zeros(128 * k + 2 * k, dtype=np.uint8)
        base = raw.ctypes.data
        arrs = {"lxy": raw[:64 * k].view(np.uint64).reshape(k, 8), "rxy": raw[64 * k:128 * k].view(np.uint64).reshape(k, 8),
                "linf": raw[128 * k:128 * k + k], "rinf": raw[128 * k + k:], "_raw": raw}
        b = _ProofBuf(k, base, base + 128 * k, base + 64 * k, base + 128 * k + k)
        return b, arrs

    @staticmethod
    def _from(b, arrs):
        k = b.rounds
        fb = int.from_bytes

        def pts(xy, inf):  # whole arrays to bytes once, then one int.from_bytes per coordinate
            raw, flags = np.ascontiguousarray(xy[:k], dtype="<u8").tobytes(), inf[:k].tolist()
            return [None if flags[i] else (fb(raw[64 * i:64 * i + 32], "little"), fb(raw[64 * i + 32:64 * i + 64], "little"))
                    for i in range(k)]
        return IPAProof(pts(arrs["lxy"], arrs["linf"]), pts(arrs["rxy"], arrs["rinf"]),
                        fb(bytes(b.tip), "little"), fb(bytes(b.y), "little"))

    def _to(self):
        k = len(self.l)
        b, arrs = IPAProof._alloc(k)
        xy, inf = _pt_arrays(self.l)
        arrs["lxy"][:] = xy
        arrs["linf"][:] = inf
        xy, inf = _pt_arrays(self.r)
        arrs["rxy"][:] = xy
        arrs["rinf"][:] = inf
        b.tip[:] = [int(v) for v in _fr(self.tip)]
        b.y[:] = [int(v) for v in _fr(self.y)]
        return b, arrs


def _log2(n):
    k = 0
    while (1 << k) < n:
        k += 1
    return k


# ---------------------------------------------------------------- ipa/mod.rs
class IPA:
    """IPA<N, G1(BN254), DefaultFieldHasher<Sha256>, GeneralEvaluationDomain>."""

    def __init__(self, engine, N, points):
        if engine.curve != "bn254":
            raise ValueError("the protocol layer is instantiated for BN254")
        assert len(points) == N + 1
        self.engine, self.N = engine, N
        self.g, self.q = points[:N], points[N]
        self.table = engine.upload_points(points)          # IPAUniversalParams::new_from_vec

    @classmethod
    def setup(cls, engine, max_items, gen_max=256, seed=b"eth_verkle_oct_2021"):
        """IPA::setup (:121-128): N + 1 generator points (fails OutOfBounds, Appendix B.1)."""
        return cls(engine, max_items, ipa_crs(max_items + 1, seed, gen_max))

    def max_size(self):
        return self.N

    def commit(self, data):
        return self.commit_batch([data])[0]

    def commit_batch(self, datas):
        sc = np.concatenate([d.limbs(self.N)[: self.N] for d in datas])
        xy, inf = self.engine.msm_batch(self.table, sc, self.N)
        return [_pt(xy[i], inf[i]) for i in range(len(datas))]

    def prove_point(self, commitment, point, data, transcript=None):
        return self.prove_batch_points([commitment], [point], [data], [transcript])[0]

    def prove_batch_points(self, commitments, points, datas, transcripts=None):
        B = len(datas)
        d = datas[0].limbs(self.N)[: self.N] if B == 1 else np.concatenate([x.limbs(self.N)[: self.N] for x in datas])
        cxy, cinf = _pt_arrays(commitments)
        pts = ints_to_limbs([int(p) % R_BN254 for p in points], 4)
        K = _log2(self.N)
        bufs = [IPAProof._alloc(K) for _ in range(B)]
        arr = (_ProofBuf * B)(*[b for b, _ in bufs])
        trs = None
        if transcripts is not None and any(t is not None for t in transcripts):
            trs = (_P * B)(*[(t.h if t is not None else None) for t in transcripts])
        check(lib().vc_ipa_prove(self.engine.h, self.table, self.N, _p(d), _p(cxy), _p(cinf), _p(pts), B,
                                 ctypes.cast(trs, _P) if trs is not None else None, ctypes.cast(arr, _P)),
              "ipa_prove")
        return [IPAProof._from(arr[i], bufs[i][1]) for i in range(B)]

    def prove_many(self, commitments, points, datas, rows=None):
        """n openings in one call, every round on the device (vc_ipa_prove_many): opening i is
        prove_point of datas[rows[i]] (rows None: datas[i], one data per point) at points[i] over a
        fresh "ipa" transcript -> list of IPAProof, equal to prove_point's. commitments: one per
        data row. VCError(VC_E_DOMAIN) for the whole call when one point makes prove_point fail."""
        n = len(points)
        if n == 0:
            return []
        if len(commitments) != len(datas):
            raise ValueError("commitments: one per data row")
        d = datas[0].limbs(self.N)[: self.N] if len(datas) == 1 else np.concatenate([x.limbs(self.N)[: self.N] for x in datas])
        d = np.ascontiguousarray(d)
        cxy, cinf = _pt_arrays_many(commitments)
        pts = ints_to_limbs([int(p) % R_BN254 for p in points], 4)
        row = np.ascontiguousarray(np.asarray(rows, dtype=np.uint32)) if rows is not None else None
        if row is not None and row.shape != (n,):
            raise ValueError("rows: one data index per point")
        K = _log2(self.N)
        lxy, rxy = np.zeros((n * K, 8), dtype=np.uint64), np.zeros((n * K, 8), dtype=np.uint64)
        linf, rinf = np.zeros(n * K, dtype=np.uint8), np.zeros(n * K, dtype=np.uint8)
        tip, y = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
        check(lib().vc_ipa_prove_many(self.engine.h, self.table, self.N, len(datas), _p(d),
                                      _p(row) if row is not None else None, _p(cxy), _p(cinf), _p(pts), n,
                                      _p(lxy), _p(linf), _p(rxy), _p(rinf), _p(tip), _p(y)), "ipa_prove_many")
        fb = int.from_bytes
        lraw, rraw, traw, yraw = lxy.tobytes(), rxy.tobytes(), tip.tobytes(), y.tobytes()
        lflag, rflag = linf.tolist(), rinf.tolist()

        def pts_of(raw, flags, i):
            return [None if flags[j] else (fb(raw[64 * j:64 * j + 32], "little"), fb(raw[64 * j + 32:64 * j + 64], "little"))
                    for j in range(i * K, (i + 1) * K)]
        return [IPAProof(pts_of(lraw, lflag, i), pts_of(rraw, rflag, i), fb(traw[32 * i:32 * i + 32], "little"),
                         fb(yraw[32 * i:32 * i + 32], "little")) for i in range(n)]

    def prove(self, commitment, index, data):
        return self.prove_point(commitment, index, data)

    def verify_point(self, commitment, point, proof, transcript=None):
        cxy, cinf = _pt_arrays([commitment])
        b, arrs = proof._to()
        res = ctypes.c_int()
        check(lib().vc_ipa_verify(self.engine.h, self.table, self.N, _p(cxy), int(cinf[0]), _p(_fr(point)),
                                  ctypes.byref(b), transcript.h if transcript is not None else None,
                                  ctypes.byref(res)), "ipa_verify")
        return bool(res.value)

    def verify(self, commitment, index, proof):
        return self.verify_point(commitment, index, proof)

    def _verify_many_arrays(self, commitments, points, proofs):
        """vc_ipa_verify_many's flat arrays (com_xy, com_inf, points, l_xy, l_inf, r_xy, r_inf, tip, y)
        and which proofs have log2 N rounds (the others go in as identities and are rejected by the
        caller). Values as given (low 256 bits): a malformed entry must reach the library unreduced."""
        K = _log2(self.N)
        good = [len(pr.l) == K and len(pr.r) == K for pr in proofs]
        none = [None] * K
        cxy, cinf = _pt_arrays_many(commitments)
        lxy, linf = _pt_arrays_many([P for pr, g in zip(proofs, good) for P in (pr.l if g else none)])
        rxy, rinf = _pt_arrays_many([P for pr, g in zip(proofs, good) for P in (pr.r if g else none)])
        pts = ints_to_limbs([int(p) & _M256 for p in points], 4)
        tips = ints_to_limbs([int(pr.tip) & _M256 for pr in proofs], 4)
        ys = ints_to_limbs([int(pr.y) & _M256 for pr in proofs], 4)
        return (cxy, cinf, pts, lxy, linf, rxy, rinf, tips, ys), good

    def verify_many(self, commitments, points, proofs, transcripts=None):
        """n openings on the GPU, one verdict each (vc_ipa_verify_many) -> list of bool; transcripts:
        None, or one TranscriptHasher (a prior state, advanced) or None per opening. VCError
        (VC_E_DOMAIN) when a point is a domain element that is not below N."""
        n = len(proofs)
        if n == 0:
            return []
        arrs, good = self._verify_many_arrays(commitments, points, proofs)
        trs = None
        if transcripts is not None and any(t is not None for t in transcripts):
            trs = (_P * n)(*[(t.h if t is not None else None) for t in transcripts])
        out = np.zeros(n, dtype=np.uint8)
        check(lib().vc_ipa_verify_many(self.engine.h, self.table, self.N, n, *[_p(a) for a in arrs],
                                       ctypes.cast(trs, _P) if trs is not None else None, _p(out)), "ipa_verify_many")
        return [bool(v) and g for v, g in zip(out, good)]

    @staticmethod
    def _handles(transcripts, n):
        if transcripts is None or not any(t is not None for t in transcripts):
            return None
        return ctypes.cast((_P * n)(*[(t.h if t is not None else None) for t in transcripts]), _P)

    def challenges_many(self, commitments, points, proofs, device=True):
        """[w, x_0 .. x_{K-1}] of every opening's fresh "ipa" transcript (vc_ipa_challenges_many) ->
        list of (w, [x_k]); device=False: the host pool instead of the device kernel."""
        n = len(proofs)
        if n == 0:
            return []
        (cxy, cinf, pts, lxy, linf, rxy, rinf, _, ys), good = self._verify_many_arrays(commitments, points, proofs)
        if not all(good):
            raise ValueError("every proof needs log2 N rounds")
        K = _log2(self.N)
        out = np.zeros((n, 1 + K, 4), dtype=np.uint64)
        check(lib().vc_ipa_challenges_many(self.engine.h if device else None, self.N, n, _p(cxy), _p(cinf), _p(pts),
                                           _p(ys), _p(lxy), _p(linf), _p(rxy), _p(rinf), _p(out)), "ipa_challenges_many")
        return [(limbs_to_int(out[i, 0]), [limbs_to_int(out[i, 1 + k]) for k in range(K)]) for i in range(n)]

    def batch_fold(self, commitments, points, proofs, rho, transcripts=None, device=True):
        """The fold of vc_ipa_verify_batch alone (vc_ipa_batch_fold): the point S for the challenge
        rho (None: the identity), or False when an entry is malformed. device=False: the host path
        over this CRS (the oracle check without a GPU, not a product path)."""
        n = len(proofs)
        arrs, good = self._verify_many_arrays(commitments, points, proofs) if n else ((None,) * 9, [])
        if not all(good):
            return False
        ptr = [_p(a) if a is not None else None for a in arrs]
        crs, _ = _pt_arrays(list(self.g) + [self.q])
        out = np.zeros(8, dtype=np.uint64)
        inf = np.zeros(1, dtype=np.uint8)
        bad = ctypes.c_int()
        check(lib().vc_ipa_batch_fold(self.engine.h if device else None, self.table, _p(crs), self.N, n, *ptr,
                                      self._handles(transcripts, n), _p(_fr_raw(rho)), _p(out), _p(inf),
                                      ctypes.byref(bad)), "ipa_batch_fold")
        if bad.value:
            return False
        return _pt(out, inf[0])

    def verify_batch(self, commitments, points, proofs, seed=None, locate=False, transcripts=None):
        """One combined check for n openings (vc_ipa_verify_batch) -> bool: are all of them valid?
        seed: 32 bytes the verifier draws after it holds the inputs (None: OS entropy). locate=True ->
        (bool, list of bool): when the combined check rejects, the per-opening verdicts of verify_many
        say which ones are bad. transcripts: as verify_many's (prior states, advanced once)."""
        n = len(proofs)
        if seed is not None and len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        arrs, good = self._verify_many_arrays(commitments, points, proofs) if n else ((None,) * 9, [])
        ptr = [_p(a) if a is not None else None for a in arrs]
        s = np.frombuffer(bytes(seed), dtype=np.uint8).copy() if seed is not None else None
        # (a proof without log2 N rounds goes in as identities: the verdicts are always wanted then)
        out = np.zeros(max(n, 1), dtype=np.uint8) if locate or not all(good) else None
        res = ctypes.c_int()
        check(lib().vc_ipa_verify_batch(self.engine.h, self.table, self.N, n, *ptr, self._handles(transcripts, n),
                                        _p(s) if s is not None else None, ctypes.byref(res),
                                        _p(out) if out is not None else None), "ipa_verify_batch")
        ok = bool(res.value) and all(good)
        if locate:
            return ok, [bool(v) and g for v, g in zip(out[:n], good)]
        return ok

    def prove_commitment(self, commitment, data):
        """:199-234 -> IPAProof with l, r, tip (y = 0)."""
        return self.prove_commitment_batch([commitment], [data])[0]

    def prove_commitment_batch(self, commitments, datas):
        n = datas[0].max() + 1
        if any(d.max() + 1 != n for d in datas):
            raise ValueError("one batch proves data of one length")
        B = len(datas)
        d = np.concatenate([x.limbs(n)[:n] for x in datas])
        cxy, cinf = _pt_arrays(commitments)
        K = _log2(n)
        bufs = [IPAProof._alloc(K) for _ in range(B)]
        arr = (_ProofBuf * B)(*[b for b, _ in bufs])
        check(lib().vc_ipa_prove_commitment(self.engine.h, self.table, n, _p(d), _p(cxy), _p(cinf), B,
                                            ctypes.cast(arr, _P)), "ipa_prove_commitment")
        return [IPAProof._from(arr[i], bufs[i][1]) for i in range(B)]

    def verify_commitment_proof(self, commitment, proof):
        """:237-265."""
        cxy, cinf = _pt_arrays([commitment])
        b, arrs = proof._to()
        res = ctypes.c_int()
        check(lib().vc_ipa_verify_commitment_proof(self.engine.h, self.table, _p(cxy), int(cinf[0]), ctypes.byref(b),
                                                   ctypes.byref(res)), "ipa_verify_commitment_proof")
        return bool(res.value)


# ---------------------------------------------------------------- kzg/mod.rs
def _fr_raw(x):
    """4 limbs of x as given (verifier inputs: a value >= r must reach the library unreduced)"""
    return ints_to_limbs([int(x) & _M256], 4)[0].copy()


def _g2_array(Q, nl=4):
    """((x0, x1), (y0, y1)) | None -> (4 nl u64 limbs, identity flag) in the ABI's G2 layout"""
    xy = np.zeros(4 * nl, dtype=np.uint64)
    if Q is None:
        return xy, 1
    (x0, x1), (y0, y1) = Q
    mask = (1 << (64 * nl)) - 1
    xy[:] = ints_to_limbs([int(v) & mask for v in (x0, x1, y0, y1)], nl).reshape(4 * nl)
    return xy, 0


def _g2_tuple(xy, nl):
    """the ABI's G2 layout -> ((x.c0, x.c1), (y.c0, y.c1))"""
    v = [limbs_to_int(xy[nl * k:nl * k + nl]) for k in range(4)]
    return ((v[0], v[1]), (v[2], v[3]))


def kzg_g2_from_secret(secret, curve="bn254"):
    """[secret]_2 = secret * H (kzg/mod.rs:122) as ((x.c0, x.c1), (y.c0, y.c1)), None = identity."""
    r, nl, cid = _curve_params(curve)
    xy = np.zeros(4 * nl, dtype=np.uint64)
    inf = np.zeros(1, dtype=np.uint8)
    check(lib().vc_kzg_g2_from_secret_curve(cid, _p(_fr(secret, r)), _p(xy), _p(inf)), "kzg_g2_from_secret")
    return None if inf[0] else _g2_tuple(xy, nl)


def pairing_check(pairs, curve="bn254"):
    """prod e(P_i, Q_i) == 1 for pairs of (G1 point | None, G2 point | None); VCError for an
    input off its curve or outside its subgroup. Host code."""
    _, nl, _ = _curve_params(curve)
    n = len(pairs)
    g1, g1inf = (_pt_arrays([a for a, _ in pairs], nl) if n
                 else (np.zeros((1, 2 * nl), dtype=np.uint64), np.zeros(1, dtype=np.uint8)))
    g2 = np.zeros((max(n, 1), 4 * nl), dtype=np.uint64)
    g2inf = np.zeros(max(n, 1), dtype=np.uint8)
    for i, (_, Q) in enumerate(pairs):
        g2[i], g2inf[i] = _g2_array(Q, nl)
    res = ctypes.c_int()
    fn = lib().vc_bn254_pairing_check if curve == "bn254" else lib().vc_bls12_381_pairing_check
    check(fn(n, _p(g1), _p(g1inf), _p(g2), _p(g2inf), ctypes.byref(res)), "pairing_check")
    return bool(res.value)


class KZGVerifyingKey:
    """[s]_2 and the domain size: all KZG::verify_point needs (no SRS, no secret). Host code
    except verify_many, and verify_batch / batch_fold when given an Engine. VCError(VC_E_INVALID)
    for a malformed [s]_2. curve: "bn254" or "bls12_381"; an Engine given to verify_many /
    verify_batch / batch_fold must be of the key's curve."""

    def __init__(self, g2, size, curve="bn254"):
        self.h = None
        self.r, self.nl, cid = _curve_params(curve)
        xy, inf = _g2_array(g2, self.nl)
        h = ctypes.c_void_p()
        check(lib().vc_kzg_vk_new_curve(cid, _p(xy), inf, size, ctypes.byref(h)), "kzg_vk_new")
        self.h, self.size, self.g2, self.curve = h, size, g2, curve

    def __del__(self):
        if getattr(self, "h", None):
            lib().vc_kzg_vk_free(self.h)
            self.h = None

    def verify_point(self, commitment, point, proof, transcript=None):
        """:165-189; proof = {"proof": point, "y": int}. The transcript is unused, as in the reference."""
        cxy, cinf = _pt_arrays([commitment], self.nl)
        pxy, pinf = _pt_arrays([proof["proof"]], self.nl)
        res = ctypes.c_int()
        check(lib().vc_kzg_verify(self.h, _p(cxy), int(cinf[0]), _p(_fr_raw(point)), _p(pxy), int(pinf[0]),
                                  _p(_fr_raw(proof["y"])), ctypes.byref(res)), "kzg_verify")
        return bool(res.value)

    def verify(self, commitment, index, proof):
        return self.verify_point(commitment, index, proof)

    def verify_many(self, engine, commitments, points, proofs):
        """n openings on the GPU, one verdict each (vc_kzg_verify_many) -> list of bool."""
        n = len(proofs)
        if n == 0:
            return []
        cxy, cinf = _pt_arrays(commitments, self.nl)
        pxy, pinf = _pt_arrays([pr["proof"] for pr in proofs], self.nl)
        pts = ints_to_limbs([int(p) & _M256 for p in points], 4)
        ys = ints_to_limbs([int(pr["y"]) & _M256 for pr in proofs], 4)
        out = np.zeros(n, dtype=np.uint8)
        check(lib().vc_kzg_verify_many(engine.h, self.h, n, _p(cxy), _p(cinf), _p(pts), _p(pxy), _p(pinf), _p(ys),
                                       _p(out)), "kzg_verify_many")
        return [bool(v) for v in out]

    def _batch_arrays(self, commitments, points, proofs):
        cxy, cinf = _pt_arrays(commitments, self.nl)
        pxy, pinf = _pt_arrays([pr["proof"] for pr in proofs], self.nl)
        pts = ints_to_limbs([int(p) & _M256 for p in points], 4)
        ys = ints_to_limbs([int(pr["y"]) & _M256 for pr in proofs], 4)
        return cxy, cinf, pts, pxy, pinf, ys

    def batch_fold(self, engine, commitments, points, proofs, rho):
        """The fold of vc_kzg_verify_batch alone (vc_kzg_batch_fold): (P1, P2) for the challenge rho,
        or None when an entry is malformed. engine None: the host path."""
        n = len(proofs)
        a = self._batch_arrays(commitments, points, proofs) if n else (None,) * 6
        ptr = [_p(x) if x is not None else None for x in a]
        out = np.zeros((2, 2 * self.nl), dtype=np.uint64)
        inf = np.zeros(2, dtype=np.uint8)
        bad = ctypes.c_int()
        check(lib().vc_kzg_batch_fold(engine.h if engine is not None else None, self.h, n, *ptr, _p(_fr_raw(rho)),
                                      _p(out[0]), _p(inf[0:1]), _p(out[1]), _p(inf[1:2]), ctypes.byref(bad)),
              "kzg_batch_fold")
        if bad.value:
            return None
        return _pt(out[0], inf[0]), _pt(out[1], inf[1])

    def verify_batch(self, engine, commitments, points, proofs, seed=None, locate=False):
        """One combined check for n openings (vc_kzg_verify_batch) -> bool: are all of them valid?
        seed: 32 bytes the verifier draws after it holds the inputs (None: OS entropy). locate=True
        (needs an Engine) -> (bool, list of bool): when the combined check rejects, the per-opening
        verdicts of verify_many say which ones are bad. engine None: the host path."""
        n = len(proofs)
        if seed is not None and len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        a = self._batch_arrays(commitments, points, proofs) if n else (None,) * 6
        ptr = [_p(x) if x is not None else None for x in a]
        s = np.frombuffer(bytes(seed), dtype=np.uint8).copy() if seed is not None else None
        out = np.zeros(max(n, 1), dtype=np.uint8) if locate else None
        res = ctypes.c_int()
        check(lib().vc_kzg_verify_batch(engine.h if engine is not None else None, self.h, n, *ptr,
                                        _p(s) if s is not None else None, ctypes.byref(res),
                                        _p(out) if locate else None), "kzg_verify_batch")
        if locate:
            return bool(res.value), [bool(v) for v in out[:n]]
        return bool(res.value)


def kzg_batch_challenge(seed, curve="bn254"):
    """rho of vc_kzg_verify_batch for a 32-byte seed: hash_to_field(seed, b"vkzg-kzg-batch") mod
    the curve's r."""
    if len(seed) != 32:
        raise ValueError("seed: 32 bytes")
    _, _, cid = _curve_params(curve)
    s = np.frombuffer(bytes(seed), dtype=np.uint8).copy()
    out = np.zeros(4, dtype=np.uint64)
    check(lib().vc_kzg_batch_challenge_curve(cid, _p(s), _p(out)), "kzg_batch_challenge")
    return limbs_to_int(out)


def kzg_subvector_weights(size, indexes, curve="bn254"):
    """The weights c_i = 1 / Z_S'(w^i) of a subvector proof over the index set (vc_kzg_subvector_weights):
    pi_S = sum c_i pi_i over the single openings' proofs. Host code."""
    _, _, cid = _curve_params(curve)
    idx = np.ascontiguousarray(np.asarray(indexes, dtype=np.uint32))
    out = np.zeros((max(len(idx), 1), 4), dtype=np.uint64)
    check(lib().vc_kzg_subvector_weights(cid, size, _p(idx), len(idx), _p(out)), "kzg_subvector_weights")
    return [limbs_to_int(out[i]) for i in range(len(idx))]


def kzg_powers_from_secret(secret, K, curve="bn254"):
    """([s^t]_1 for t < K, [s^t]_2 for t <= K) from the secret (vc_kzg_powers_from_secret): tests and
    trusted setups. Host code."""
    r, nl, cid = _curve_params(curve)
    g1 = np.zeros((K, 2 * nl), dtype=np.uint64)
    g2 = np.zeros((K + 1, 4 * nl), dtype=np.uint64)
    check(lib().vc_kzg_powers_from_secret(cid, _p(_fr(secret, r)), K, _p(g1), _p(g2)), "kzg_powers_from_secret")
    return [_pt(g1[t], 0) for t in range(K)], [_g2_tuple(g2[t], nl) for t in range(K + 1)]


class KZGSubvectorKey:
    """The verifying key of subvector proofs: [s^t]_1 for t < K and [s^t]_2 for t <= K (K =
    len(g1_powers)) and the domain size. Every point is checked (VCError(VC_E_INVALID) otherwise);
    that the powers belong to one s is not: the key is trusted input. Host code, no Engine, except
    verify_batch / batch_fold when given one (of the key's curve)."""

    def __init__(self, g1_powers, g2_powers, size, curve="bn254"):
        self.h = None
        self.r, self.nl, cid = _curve_params(curve)
        K = len(g1_powers)
        if len(g2_powers) != K + 1 or any(P is None for P in g1_powers) or any(Q is None for Q in g2_powers):
            raise ValueError("K powers in G1 and K + 1 in G2, none the identity")
        g1, _ = _pt_arrays(g1_powers, self.nl)
        g2 = np.stack([_g2_array(Q, self.nl)[0] for Q in g2_powers])
        h = ctypes.c_void_p()
        check(lib().vc_kzg_svk_new(cid, size, K, _p(np.ascontiguousarray(g1)), _p(np.ascontiguousarray(g2)),
                                   ctypes.byref(h)), "kzg_svk_new")
        self.h, self.size, self.K, self.curve = h, size, K, curve

    def __del__(self):
        if getattr(self, "h", None):
            lib().vc_kzg_svk_free(self.h)
            self.h = None

    def verify(self, commitment, indexes, ys, proof):
        """One proof (a point | None) that positions `indexes` of the vector committed to hold `ys`
        (vc_kzg_verify_subvector) -> bool. VCError(VC_E_RANGE) above K indices, VCError(VC_E_INVALID)
        for a repeated index or one outside the domain."""
        cxy, cinf = _pt_arrays([commitment], self.nl)
        pxy, pinf = _pt_arrays([proof], self.nl)
        idx = np.ascontiguousarray(np.asarray(indexes, dtype=np.uint32))
        y = ints_to_limbs([int(v) & _M256 for v in ys], 4) if len(ys) else np.zeros((1, 4), dtype=np.uint64)
        if len(ys) != len(idx):
            raise ValueError("one y per index")
        res = ctypes.c_int()
        check(lib().vc_kzg_verify_subvector(self.h, _p(cxy), int(cinf[0]), _p(idx), len(idx), _p(np.ascontiguousarray(y)),
                                            _p(pxy), int(pinf[0]), ctypes.byref(res)), "kzg_verify_subvector")
        return bool(res.value)


    def _subv_arrays(self, commitments, index_sets, ys, proofs):
        n = len(proofs)
        if not (len(commitments) == len(index_sets) == len(ys) == n):
            raise ValueError("one commitment, index set and list of ys per proof")
        if any(len(S) != len(v) for S, v in zip(index_sets, ys)):
            raise ValueError("one y per index")
        cxy, cinf = _pt_arrays(commitments, self.nl)
        pxy, pinf = _pt_arrays(proofs, self.nl)
        off = np.zeros(n + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(S) for S in index_sets])
        idx = np.ascontiguousarray(np.asarray([i for S in index_sets for i in S], dtype=np.uint32))
        flat = [int(v) & _M256 for yv in ys for v in yv]
        if idx.size == 0:
            idx = np.zeros(1, dtype=np.uint32)
        y = np.ascontiguousarray(ints_to_limbs(flat, 4)) if flat else np.zeros((1, 4), dtype=np.uint64)
        return cxy, cinf, off, idx, y, pxy, pinf

    def batch_fold(self, engine, commitments, index_sets, ys, proofs, rho):
        """The fold of verify_batch alone (vc_kzg_subvector_batch_fold): [P_H, P_1 .. P_Kmax] for the
        challenge rho (Kmax the largest set), or None when an entry is malformed. engine None: the
        host path."""
        n = len(proofs)
        a = self._subv_arrays(commitments, index_sets, ys, proofs) if n else (None,) * 7
        ptr = [_p(x) if x is not None else None for x in a]
        out = np.zeros((self.K + 1, 2 * self.nl), dtype=np.uint64)
        inf = np.zeros(self.K + 1, dtype=np.uint8)
        bad, kmax = ctypes.c_int(), ctypes.c_size_t()
        check(lib().vc_kzg_subvector_batch_fold(engine.h if engine is not None else None, self.h, n, *ptr,
                                                _p(_fr_raw(rho)), ctypes.byref(kmax), _p(out), _p(inf),
                                                ctypes.byref(bad)), "kzg_subvector_batch_fold")
        if bad.value:
            return None
        return [_pt(out[t], inf[t]) for t in range(kmax.value + 1)]

    def verify_batch(self, engine, commitments, index_sets, ys, proofs, seed=None, locate=False):
        """One combined check for n subvector proofs (vc_kzg_verify_subvector_batch) -> bool: are all
        of them valid? proofs: points | None. seed: 32 bytes the verifier draws after it holds the
        inputs (None: OS entropy). locate=True -> (bool, list of bool): when the combined check
        rejects, verify's verdicts say which ones are bad. engine None: the host path."""
        n = len(proofs)
        if seed is not None and len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        a = self._subv_arrays(commitments, index_sets, ys, proofs) if n else (None,) * 7
        ptr = [_p(x) if x is not None else None for x in a]
        s = np.frombuffer(bytes(seed), dtype=np.uint8).copy() if seed is not None else None
        out = np.zeros(max(n, 1), dtype=np.uint8) if locate else None
        res = ctypes.c_int()
        check(lib().vc_kzg_verify_subvector_batch(engine.h if engine is not None else None, self.h, n, *ptr,
                                                  _p(s) if s is not None else None, ctypes.byref(res),
                                                  _p(out) if locate else None), "kzg_verify_subvector_batch")
        if locate:
            return bool(res.value), [bool(v) for v in out[:n]]
        return bool(res.value)


def kzg_subvector_batch_challenge(seed, curve="bn254"):
    """rho of KZGSubvectorKey.verify_batch for a 32-byte seed: hash_to_field(seed,
    b"vkzg-kzg-subv-batch") mod the curve's r."""
    if len(seed) != 32:
        raise ValueError("seed: 32 bytes")
    _, _, cid = _curve_params(curve)
    s = np.frombuffer(bytes(seed), dtype=np.uint8).copy()
    out = np.zeros(4, dtype=np.uint64)
    check(lib().vc_kzg_subvector_batch_challenge(cid, _p(s), _p(out)), "kzg_subvector_batch_challenge")
    return limbs_to_int(out)


def ipa_batch_challenge(seed):
    """rho of vc_ipa_verify_batch for a 32-byte seed: hash_to_field(seed, b"vkzg-ipa-batch")."""
    if len(seed) != 32:
        raise ValueError("seed: 32 bytes")
    s = np.frombuffer(bytes(seed), dtype=np.uint8).copy()
    out = np.zeros(4, dtype=np.uint64)
    check(lib().vc_ipa_batch_challenge(_p(s), _p(out)), "ipa_batch_challenge")
    return limbs_to_int(out)


class KZG:
    """KZG<Bn254, ...>: commit, open and (through KZGVerifyingKey) verify with pairings. On an
    Engine("bls12_381") the same over BLS12-381 (data: LagrangeBasis(evals, r=R_BLS12_381));
    prove_all_points, quotient and the multiproofs stay BN254."""

    def __init__(self, engine, max_items, secret=100):
        self.engine = engine
        self.r, self.nl, _ = _curve_params(engine.curve)
        tid = ctypes.c_int()
        size = ctypes.c_size_t()
        check(lib().vc_kzg_setup(engine.h, max_items, _p(_fr(secret, self.r)), ctypes.byref(tid), ctypes.byref(size)),
              "kzg_setup")
        self.table, self.size, self.secret = tid.value, size.value, secret

    def max_size(self):
        return self.size

    def lagrange_points(self):
        xy, inf = self.engine.download_bases(self.table)
        return [_pt(xy[i], inf[i]) for i in range(self.size)]

    def commit(self, data):
        """:126-134 inner_product(lagrange_commitments, evals) (zip-truncating)."""
        sc = data.limbs()
        xy, inf = self.engine.msm(self.table, sc)
        return _pt(xy, inf)

    def prove_point(self, commitment, point, data, transcript=None):
        """one opening (vc_kzg_prove) -> {"proof", "y"}; the point is taken mod r. VCError with
        status VC_E_DOMAIN (-8) where the reference panics: point == size, and a domain element that
        is not below size (z^size == 1, r - 1 among them). (The C call also returns VC_E_INVALID for
        a point >= r; the reduction here keeps that from happening.) A failing call proves nothing."""
        ev = data.limbs()
        pxy = np.zeros(2 * self.nl, dtype=np.uint64)
        pinf = np.zeros(1, dtype=np.uint8)
        y = np.zeros(4, dtype=np.uint64)
        check(lib().vc_kzg_prove(self.engine.h, self.table, self.size, _p(ev), len(data.evals), _p(_fr(point, self.r)),
                                 _p(pxy), _p(pinf), _p(y)), "kzg_prove")
        return {"proof": _pt(pxy, pinf[0]), "y": limbs_to_int(y)}

    def prove(self, commitment, index, data):
        return self.prove_point(commitment, index, data)

    def prove_batch_points(self, commitments, points, datas, rows=None):
        """n openings in one call (vc_kzg_prove_many): opening i is prove_point of datas[rows[i]]
        (rows None: datas[i], one data per point) at points[i] -> list of {"proof", "y"}. The datas
        have one length; the commitments are unused, as in prove_point. VCError(VC_E_DOMAIN) for the
        whole call when one point makes prove_point fail."""
        n = len(points)
        if n == 0:
            return []
        width = len(datas[0].evals)
        if any(len(d.evals) != width for d in datas):
            raise ValueError("one batch proves data of one length")
        ev = datas[0].limbs() if len(datas) == 1 else np.concatenate([d.limbs() for d in datas])
        ev = np.ascontiguousarray(ev)
        pts = ints_to_limbs([int(p) % self.r for p in points], 4)
        row = np.ascontiguousarray(np.asarray(rows, dtype=np.uint32)) if rows is not None else None
        if row is not None and row.shape != (n,):
            raise ValueError("rows: one data index per point")
        pxy = np.zeros((n, 2 * self.nl), dtype=np.uint64)
        pinf = np.zeros(n, dtype=np.uint8)
        ys = np.zeros((n, 4), dtype=np.uint64)
        check(lib().vc_kzg_prove_many(self.engine.h, self.table, self.size, len(datas), width, _p(ev),
                                      _p(row) if row is not None else None, _p(pts), n, _p(pxy), _p(pinf), _p(ys)),
              "kzg_prove_many")
        return [{"proof": _pt(pxy[i], pinf[i]), "y": limbs_to_int(ys[i])} for i in range(n)]

    def prove_subvectors(self, rows, index_sets, datas):
        """One subvector proof per index set (vc_kzg_prove_subvector_many): set s proves the positions
        index_sets[s] of datas[rows[s]] (rows None: datas[s]) -> list of {"proof", "ys"}, the ys in the
        set's own order. The reference's prove_batch (kzg/mod.rs:156-163, todo!() there)."""
        n = len(index_sets)
        if n == 0:
            return []
        width = len(datas[0].evals)
        if any(len(d.evals) != width for d in datas):
            raise ValueError("one batch proves data of one length")
        ev = datas[0].limbs() if len(datas) == 1 else np.concatenate([d.limbs() for d in datas])
        ev = np.ascontiguousarray(ev)
        row = np.ascontiguousarray(np.asarray(rows, dtype=np.uint32)) if rows is not None else None
        if row is not None and row.shape != (n,):
            raise ValueError("rows: one data index per index set")
        off = np.zeros(n + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(s) for s in index_sets])
        total = int(off[n])
        idx = np.ascontiguousarray(np.asarray([i for s in index_sets for i in s], dtype=np.uint32))
        if idx.size == 0:
            idx = np.zeros(1, dtype=np.uint32)
        pxy = np.zeros((n, 2 * self.nl), dtype=np.uint64)
        pinf = np.zeros(n, dtype=np.uint8)
        ys = np.zeros((max(total, 1), 4), dtype=np.uint64)
        check(lib().vc_kzg_prove_subvector_many(self.engine.h, self.table, self.size, len(datas), width, _p(ev),
                                                _p(row) if row is not None else None, _p(off), _p(idx), n, _p(pxy),
                                                _p(pinf), _p(ys)), "kzg_prove_subvector_many")
        return [{"proof": _pt(pxy[s], pinf[s]), "ys": [limbs_to_int(ys[p]) for p in range(int(off[s]), int(off[s + 1]))]}
                for s in range(n)]

    def prove_subvector(self, commitment, indexes, data):
        """prove_batch(key, commitment, indexes, data): one proof for the positions `indexes` of data;
        the commitment is unused, as in prove_point."""
        return self.prove_subvectors(None, [list(indexes)], [data])[0]

    def g1_powers(self, K):
        """[s^t]_1 for t < K from the Lagrange SRS (vc_kzg_g1_powers), no secret."""
        out = np.zeros((K, 2 * self.nl), dtype=np.uint64)
        check(lib().vc_kzg_g1_powers(self.engine.h, self.table, self.size, K, _p(out)), "kzg_g1_powers")
        return [_pt(out[t], 0) for t in range(K)]

    def subvector_key(self, K):
        """The KZGSubvectorKey for sets of up to K indices: G1 powers from the SRS on the GPU, G2
        powers from the setup's secret (as g2())."""
        _, g2 = kzg_powers_from_secret(self.secret, K, self.engine.curve)
        return KZGSubvectorKey(self.g1_powers(K), g2, self.size, self.engine.curve)

    def prove_all_points(self, data, mode=0):
        """KZG::prove_all_points (kzg/mod.rs:200-235) -- mode 0: the reference's computation
        exactly (its h_hat values, y = data[i]); mode 1: the FK opening proofs at every domain
        point (== prove at each index). Returns a list of {"proof", "y"}."""
        ev = data.limbs() if data.evals else np.zeros((0, 4), dtype=np.uint64)
        n_out = self.size if mode == 1 else max(1, len(data.evals))
        xy = np.zeros((n_out, 8), dtype=np.uint64)
        inf = np.zeros(n_out, dtype=np.uint8)
        ys = np.zeros((n_out, 4), dtype=np.uint64)
        cnt = ctypes.c_size_t()
        check(lib().vc_kzg_prove_all_points(self.engine.h, self.table, self.size, _p(ev), len(data.evals), mode,
                                            _p(xy), _p(inf), _p(ys), ctypes.byref(cnt)), "kzg_prove_all_points")
        return [{"proof": _pt(xy[i], inf[i]), "y": limbs_to_int(ys[i])} for i in range(cnt.value)]

    def g2(self):
        """[s]_2 of the setup (kzg/mod.rs:122)."""
        return kzg_g2_from_secret(self.secret, self.engine.curve)

    def verifying_key(self):
        if getattr(self, "_vk", None) is None:
            self._vk = KZGVerifyingKey(self.g2(), self.size, self.engine.curve)
        return self._vk

    def verify_point(self, commitment, point, proof, transcript=None):
        """KZG::verify_point (:165-189) on the host."""
        return self.verifying_key().verify_point(commitment, point, proof)

    def verify(self, commitment, index, proof):
        return self.verify_point(commitment, index, proof)

    def verify_many(self, commitments, points, proofs):
        """One verdict per opening, the batch on the GPU (test_amortized_proof's loop)."""
        return self.verifying_key().verify_many(self.engine, commitments, points, proofs)

    def verify_batch(self, commitments, points, proofs, seed=None, locate=False):
        """One verdict for the whole batch (KZGVerifyingKey.verify_batch on this engine)."""
        return self.verifying_key().verify_batch(self.engine, commitments, points, proofs, seed=seed, locate=locate)

    def quotient(self, point, data):
        ev = data.limbs()
        q = np.zeros((self.size, 4), dtype=np.uint64)
        y = np.zeros(4, dtype=np.uint64)
        check(lib().vc_kzg_quotient(self.engine.h, self.size, _p(ev), len(data.evals), _p(_fr(point)), _p(q),
                                    _p(y)), "kzg_quotient")
        return [limbs_to_int(r) for r in q], limbs_to_int(y)


# ---------------------------------------------------------------- multiproof.rs
def _queries(queries, N):
    Q = len(queries)
    data = np.concatenate([q[0].limbs(N)[:N] for q in queries])
    cxy, cinf = _pt_arrays([q[1] for q in queries])
    z = np.array([int(q[2]) for q in queries], dtype=np.uint64)
    y = ints_to_limbs([int(q[3]) % R_BN254 for q in queries], 4)
    return Q, data, cxy, cinf, z, y


def prove_multiproof(vc, queries):
    """queries: list of (LagrangeBasis data, commitment, z, y). Returns {"proof", "d"}."""
    N = vc.N if isinstance(vc, IPA) else vc.size
    Q, data, cxy, cinf, z, y = _queries(queries, N)
    dxy = np.zeros(8, dtype=np.uint64)
    dinf = np.zeros(1, dtype=np.uint8)
    if isinstance(vc, IPA):
        b, arrs = IPAProof._alloc(_log2(N))
        check(lib().vc_multiproof_prove(vc.engine.h, 0, vc.table, N, Q, _p(data), _p(cxy), _p(cinf), _p(z), _p(y),
                                        _p(dxy), _p(dinf), ctypes.byref(b), None, None, None), "multiproof_prove")
        return {"proof": IPAProof._from(b, arrs), "d": _pt(dxy, dinf[0])}
    kxy = np.zeros(8, dtype=np.uint64)
    kinf = np.zeros(1, dtype=np.uint8)
    ky = np.zeros(4, dtype=np.uint64)
    check(lib().vc_multiproof_prove(vc.engine.h, 1, vc.table, N, Q, _p(data), _p(cxy), _p(cinf), _p(z), _p(y),
                                    _p(dxy), _p(dinf), None, _p(kxy), _p(kinf), _p(ky)), "multiproof_prove")
    return {"proof": {"proof": _pt(kxy, kinf[0]), "y": limbs_to_int(ky)}, "d": _pt(dxy, dinf[0])}


def verify_multiproof(vc, vqueries, mp):
    """IPA: full verification. KZG: returns the (E - D, t) claim for an external pairing check."""
    N = vc.N if isinstance(vc, IPA) else vc.size
    Q = len(vqueries)
    cxy, cinf = _pt_arrays([q[0] for q in vqueries])
    z = np.array([int(q[1]) for q in vqueries], dtype=np.uint64)
    y = ints_to_limbs([int(q[2]) % R_BN254 for q in vqueries], 4)
    dxy, dinf = _pt_arrays([mp["d"]])
    if isinstance(vc, IPA):
        b, arrs = mp["proof"]._to()
        res = ctypes.c_int()
        check(lib().vc_multiproof_verify_ipa(vc.engine.h, vc.table, N, Q, _p(cxy), _p(cinf), _p(z), _p(y), _p(dxy),
                                             int(dinf[0]), ctypes.byref(b), ctypes.byref(res)), "multiproof_verify")
        return bool(res.value)
    oxy = np.zeros(8, dtype=np.uint64)
    oinf = np.zeros(1, dtype=np.uint8)
    t = np.zeros(4, dtype=np.uint64)
    check(lib().vc_multiproof_kzg_claim(vc.engine.h, N, Q, _p(cxy), _p(cinf), _p(z), _p(y), _p(dxy), int(dinf[0]),
                                        _p(oxy), _p(oinf), _p(t)), "multiproof_kzg_claim")
    return {"commitment": _pt(oxy, oinf[0]), "t": limbs_to_int(t)}


def verify_multiproof_kzg(vc, vqueries, mp):
    """verify_multiproof (multiproof.rs:178-215) for KZG, pairing check included -> bool.
    vc: a KZG (its verifying key is used); vqueries: (commitment, z, y); mp: {"proof", "d"}."""
    N, Q = vc.size, len(vqueries)
    cxy, cinf = _pt_arrays([q[0] for q in vqueries])
    z = np.array([int(q[1]) for q in vqueries], dtype=np.uint64)
    y = ints_to_limbs([int(q[2]) % R_BN254 for q in vqueries], 4)
    dxy, dinf = _pt_arrays([mp["d"]])
    pxy, pinf = _pt_arrays([mp["proof"]["proof"]])
    res = ctypes.c_int()
    check(lib().vc_multiproof_verify_kzg(vc.engine.h, vc.verifying_key().h, N, Q, _p(cxy), _p(cinf), _p(z), _p(y),
                                         _p(dxy), int(dinf[0]), _p(pxy), int(pinf[0]), _p(_fr_raw(mp["proof"]["y"])),
                                         ctypes.byref(res)), "multiproof_verify_kzg")
    return bool(res.value)


class MultiproofSet:
    """Output buffers of P multiproofs (vc_multiproof_prove_many / _sharded / _gather): D points,
    and P IPA proofs (scheme 0) or P KZG (proof, y) pairs (scheme 1)."""

    def __init__(self, scheme_id, N, P):
        self.scheme, self.N, self.P = scheme_id, N, P
        self.d_xy = np.zeros((max(P, 1), 8), dtype=np.uint64)
        self.d_inf = np.zeros(max(P, 1), dtype=np.uint8)
        self.bufs, self.arrs = None, []
        self.kxy = self.kinf = self.ky = None
        if scheme_id == 0:
            self.bufs = (_ProofBuf * max(P, 1))()
            for p in range(P):
                b, arrs = IPAProof._alloc(_log2(N))
                self.bufs[p] = b
                self.arrs.append(arrs)
        else:
            self.kxy = np.zeros((max(P, 1), 8), dtype=np.uint64)
            self.kinf = np.zeros(max(P, 1), dtype=np.uint8)
            self.ky = np.zeros((max(P, 1), 4), dtype=np.uint64)

    def args(self):
        """(d_xy, d_inf, ipa_proofs, kzg_xy, kzg_inf, kzg_y) pointers of the C ABI"""
        if self.scheme == 0:
            return _p(self.d_xy), _p(self.d_inf), ctypes.cast(self.bufs, ctypes.c_void_p), None, None, None
        return _p(self.d_xy), _p(self.d_inf), None, _p(self.kxy), _p(self.kinf), _p(self.ky)

    def proofs(self):
        out = []
        for p in range(self.P):
            if self.scheme == 0:
                pr = IPAProof._from(self.bufs[p], self.arrs[p])
            else:
                pr = {"proof": _pt(self.kxy[p], self.kinf[p]), "y": limbs_to_int(self.ky[p])}
            out.append({"proof": pr, "d": _pt(self.d_xy[p], self.d_inf[p])})
        return out


def prove_multiproof_many(vc, cxy, cinf, z, y, d_data_ptr):
    """P independent multiproofs at once on one GPU (vc_multiproof_prove_many): cxy [P][Q][8],
    cinf [P][Q], z [P][Q], y [P][Q][4] host arrays; d_data_ptr -> [P][Q][N] canonical evaluations
    on the device. Returns P {"proof", "d"} as prove_multiproof does."""
    ipa = isinstance(vc, IPA)
    N = vc.N if ipa else vc.size
    P, Q = z.shape
    out = MultiproofSet(0 if ipa else 1, N, P)
    cxy, cinf, z, y = (np.ascontiguousarray(a) for a in (cxy, cinf, z, y))
    check(lib().vc_multiproof_prove_many(vc.engine.h, out.scheme, vc.table, N, Q, P, ctypes.c_void_p(d_data_ptr),
                                         _p(cxy), _p(cinf), _p(z), _p(y), *out.args()), "multiproof_prove_many")
    return out.proofs()


# ---------------------------------------------------------------- P multiproofs verified in one call
MPV_Q_MAX = 4096  # VC_MPV_Q_MAX: queries per proof of the many-verifier


def _queries_many(queries_per_proof):
    """[[(commitment, z, y)]] -> (q_ptr, com_xy, com_inf, z, y) flat arrays. Values as given (low
    256 bits): a malformed entry must reach the library unreduced."""
    flat = [q for qs in queries_per_proof for q in qs]
    q_ptr = np.zeros(len(queries_per_proof) + 1, dtype=np.uint64)
    q_ptr[1:] = np.cumsum([len(qs) for qs in queries_per_proof], dtype=np.uint64)
    cxy, cinf = _pt_arrays_many([q[0] for q in flat])
    z = np.array([int(q[1]) for q in flat], dtype=np.uint64)
    y = ints_to_limbs([int(q[2]) & _M256 for q in flat], 4) if flat else np.zeros((0, 4), dtype=np.uint64)
    return q_ptr, cxy, cinf, z, y


def multiproof_claims_many(vc, queries_per_proof, ds):
    """(E - D, t) of P multiproofs in one call (vc_multiproof_claims_many): queries_per_proof P lists
    of (commitment, z, y), ds the proofs' D points -> P entries {"commitment", "t"} as
    verify_multiproof gives for KZG, or None for an entry with malformed content."""
    P = len(queries_per_proof)
    if P == 0:
        return []
    N = vc.N if isinstance(vc, IPA) else vc.size
    q_ptr, cxy, cinf, z, y = _queries_many(queries_per_proof)
    dxy, dinf = _pt_arrays_many(list(ds))
    oxy = np.zeros((P, 8), dtype=np.uint64)
    oinf = np.zeros(P, dtype=np.uint8)
    t = np.zeros((P, 4), dtype=np.uint64)
    bad = np.zeros(P, dtype=np.uint8)
    check(lib().vc_multiproof_claims_many(vc.engine.h, N, P, _p(q_ptr), 0, _p(cxy), _p(cinf), _p(z), _p(y), _p(dxy),
                                          _p(dinf), _p(oxy), _p(oinf), _p(t), _p(bad)), "multiproof_claims_many")
    return [None if bad[p] else {"commitment": _pt(oxy[p], oinf[p]), "t": limbs_to_int(t[p])} for p in range(P)]


def verify_multiproof_many(vc, queries_per_proof, mps):
    """P multiproofs on the GPU, one verdict each (vc_multiproof_verify_many_ipa / _kzg) -> list of
    bool. queries_per_proof: P lists of (commitment, z, y), ragged or not; mps: P {"proof", "d"} as
    prove_multiproof / prove_multiproof_many return them. vc: the IPA or KZG scheme object (KZG: its
    verifying key is used). VCError (VC_E_DOMAIN) when a z is not below N."""
    P = len(mps)
    if len(queries_per_proof) != P:
        raise ValueError("one query list per proof")
    if P == 0:
        return []
    q_ptr, cxy, cinf, z, y = _queries_many(queries_per_proof)
    dxy, dinf = _pt_arrays_many([mp["d"] for mp in mps])
    out = np.zeros(P, dtype=np.uint8)
    if isinstance(vc, IPA):
        proofs = [mp["proof"] for mp in mps]
        (_, _, _, lxy, linf, rxy, rinf, tips, ys), good = vc._verify_many_arrays([None] * P, [0] * P, proofs)
        check(lib().vc_multiproof_verify_many_ipa(vc.engine.h, vc.table, vc.N, P, _p(q_ptr), 0, _p(cxy), _p(cinf), _p(z),
                                                  _p(y), _p(dxy), _p(dinf), _p(lxy), _p(linf), _p(rxy), _p(rinf),
                                                  _p(tips), _p(ys), _p(out)), "multiproof_verify_many_ipa")
        return [bool(v) and g for v, g in zip(out, good)]
    kxy, kinf = _pt_arrays_many([mp["proof"]["proof"] for mp in mps])
    ky = ints_to_limbs([int(mp["proof"]["y"]) & _M256 for mp in mps], 4)
    check(lib().vc_multiproof_verify_many_kzg(vc.engine.h, vc.verifying_key().h, vc.size, P, _p(q_ptr), 0, _p(cxy),
                                              _p(cinf), _p(z), _p(y), _p(dxy), _p(dinf), _p(kxy), _p(kinf), _p(ky),
                                              _p(out)), "multiproof_verify_many_kzg")
    return [bool(v) for v in out]


# ---------------------------------------------------------------- sharded multiproof
def multiproof_begin(N, cxy, cinf, z, y):
    """Phase 1 (host, every rank): transcript over all queries -> (transcript handle, r limbs, rows)."""
    Q = len(z)
    tr = ctypes.c_void_p()
    r = np.zeros(4, dtype=np.uint64)
    rows = ctypes.c_size_t()
    check(lib().vc_multiproof_begin(N, Q, _p(cxy), _p(cinf), _p(z), _p(y), ctypes.byref(tr), _p(r),
                                    ctypes.byref(rows)), "multiproof_begin")
    return tr, r, rows.value


def multiproof_accumulate(engine, N, z, first, count, d_data_ptr, r, d_S_ptr):
    """Phase 2 (device): this shard's rows x N per-point sums into d_S (canonical u64 x 4)."""
    check(lib().vc_multiproof_accumulate(engine.h, N, len(z), _p(z), first, count, ctypes.c_void_p(d_data_ptr),
                                         _p(r), ctypes.c_void_p(d_S_ptr)), "multiproof_accumulate")


def multiproof_rows(N, z):
    """The number of distinct query points (rows of the per-point sums S)."""
    rows = ctypes.c_size_t()
    check(lib().vc_multiproof_rows(N, len(z), _p(z), ctypes.byref(rows)), "multiproof_rows")
    return rows.value


def multiproof_begin_accumulate(engine, N, cxy, cinf, z, y, first, count, d_data_ptr, d_S_ptr):
    """Phases 1 + 2 in one call (the transcript overlapped with the shard's planning and uploads)
    -> (transcript handle, r limbs); S of the shard into d_S (multiproof_rows(N, z) x N x 4 u64)."""
    tr = ctypes.c_void_p()
    r = np.zeros(4, dtype=np.uint64)
    check(lib().vc_multiproof_begin_accumulate(engine.h, N, len(z), _p(cxy), _p(cinf), _p(z), _p(y), first, count,
                                               ctypes.c_void_p(d_data_ptr), ctypes.c_void_p(d_S_ptr),
                                               ctypes.byref(tr), _p(r)), "multiproof_begin_accumulate")
    return tr, r


def multiproof_finish(vc, z, d_S_parts_ptr, G, tr):
    """Phase 3: sum the G shards' S, then D, t, E and the inner proof -- an IPA proof or the KZG
    (proof, y) of prove_point at t (multiproof.rs:129-175). Frees `tr`."""
    if isinstance(vc, IPA):
        return multiproof_finish_ipa(vc, z, d_S_parts_ptr, G, tr)
    N = vc.size
    dxy = np.zeros(8, dtype=np.uint64)
    dinf = np.zeros(1, dtype=np.uint8)
    kxy = np.zeros(8, dtype=np.uint64)
    kinf = np.zeros(1, dtype=np.uint8)
    ky = np.zeros(4, dtype=np.uint64)
    try:
        check(lib().vc_multiproof_finish(vc.engine.h, 1, vc.table, N, len(z), _p(z), ctypes.c_void_p(d_S_parts_ptr),
                                         G, tr, _p(dxy), _p(dinf), None, _p(kxy), _p(kinf), _p(ky)),
              "multiproof_finish")
    finally:
        lib().vc_transcript_free(tr)
    return {"proof": {"proof": _pt(kxy, kinf[0]), "y": limbs_to_int(ky)}, "d": _pt(dxy, dinf[0])}


def multiproof_finish_ipa(ipa, z, d_S_parts_ptr, G, tr):
    """Phase 3: sum the G shards' S, then D, t, E and the inner IPA proof. Frees `tr`."""
    N = ipa.N
    dxy = np.zeros(8, dtype=np.uint64)
    dinf = np.zeros(1, dtype=np.uint8)
    b, arrs = IPAProof._alloc(_log2(N))
    try:
        check(lib().vc_multiproof_finish(ipa.engine.h, 0, ipa.table, N, len(z), _p(z), ctypes.c_void_p(d_S_parts_ptr),
                                         G, tr, _p(dxy), _p(dinf), ctypes.byref(b), None, None, None),
              "multiproof_finish")
    finally:
        lib().vc_transcript_free(tr)
    return {"proof": IPAProof._from(b, arrs), "d": _pt(dxy, dinf[0])}

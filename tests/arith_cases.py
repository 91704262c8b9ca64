"""Test helper for the device arithmetic parity tests (tests/test_arith_host.py, test_gpu_arith.py):
one operand table, three evaluators. The tables and every expected value come from Python integers
and the oracle's curves; the other two evaluators are the host build and the device build of the
project's own headers behind lib/libvkzg_check.so (csrc/arith_check.hip), which takes and returns
plain 32-bit words. Seeded and deterministic; nothing here decides what the headers compute.

Groups: (a) ff.hpp fields, (b) the radix-2^29 / signed radix-2^30 limb engines, (c) the group law of
ec.hpp and of the Fast29 engines, (d) add_quad, (e) fb_block_sum_store."""
import ctypes
import functools
import os
import random
import subprocess

import numpy as np

import limb_bounds as lb
from pyoracle import curves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "verkle-kzg_amd")
LIB_PATH = os.path.join(PKG, "lib", "libvkzg_check.so")
VC_OK, VC_E_INVALID, VC_E_NO_DEVICE = 0, -1, -7


# ---------------------------------------------------------------- the library
def build_lib():
    """build (if needed) the check library: the Makefile's `check` target"""
    if not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-C", PKG, "check"], stdout=subprocess.DEVNULL)
    return LIB_PATH


@functools.lru_cache(maxsize=None)
def lib():
    L = ctypes.CDLL(LIB_PATH)
    P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.vkc_fe.argtypes = [I, I, Z, P, P, P, I]
    L.vkc_limb.argtypes = [I, I, Z, P, P, P, P, P, I]
    L.vkc_point.argtypes = [I, I, I, Z, P, Z, P, P, I]
    L.vkc_quad.argtypes = [I, Z, P, Z, P, P]
    L.vkc_block_sum.argtypes = [I, I, Z, P, Z, P, P]
    for f in (L.vkc_fe, L.vkc_limb, L.vkc_point, L.vkc_quad, L.vkc_block_sum):
        f.restype = I
    return L


class CheckLibError(RuntimeError):
    def __init__(self, call, status):
        super().__init__(f"{call} returned {status}")
        self.status = status


def _ptr(a):
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


# ---------------------------------------------------------------- words <-> integers
def to_words(vals, N):
    raw = b"".join(int(v).to_bytes(4 * N, "little") for v in vals)
    return np.frombuffer(raw, dtype="<u4").reshape(len(vals), N).astype(np.uint32)


def from_words(arr):
    arr = np.ascontiguousarray(arr, dtype="<u4")
    return [int.from_bytes(row.tobytes(), "little") for row in arr]


# ================================================================ (a) ff.hpp
FE_FIELDS = {  # name -> (id of vkc_fe, p, N)
    "bn254_fq": (0, lb.BN254_FQ, 8),
    "bn254_fr": (1, lb.BN254_FR, 8),
    "bls12_381_fq": (2, lb.BLS_FQ, 12),
    "bls12_381_fr": (3, lb.BLS_FR, 8),
    "band_fr": (4, curves.BAND_R, 8),
}
FE_OPS = ["mul", "sqr", "mul_body", "add", "sub", "neg", "dbl", "small3", "small5", "small8", "to_mont", "from_mont",
          "inv", "inv_bin"]
FE_BINARY = ("mul", "mul_body", "add", "sub")
FE_INVERSIONS = ("inv", "inv_bin")


def edge_values(p, N):
    """the canonical values (below p) where 32-bit limb code goes wrong"""
    R = 1 << (32 * N)
    top_shift = 32 * (N - 1)
    ptop = p >> top_shift
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, R % p, R * R % p, p - R % p]
    for k in range(1, N):  # every limb boundary
        vals += [1 << (32 * k), (1 << (32 * k)) - 1]
    low_ones = (1 << top_shift) - 1
    vals.append((ptop << top_shift | low_ones) if (ptop << top_shift | low_ones) < p else ((ptop - 1) << top_shift | low_ones))
    vals += [p - (1 << (32 * k)) for k in range(N)]  # p with one limb decremented
    for phase in (0, 1):  # alternating all-ones and zero limbs
        v = sum(0xFFFFFFFF << (32 * k) for k in range(N) if k % 2 == phase)
        if v >= p:
            v = (v & low_ones) | ((ptop - 1) << top_shift)
        vals.append(v)
    out = []
    for v in vals:
        assert 0 <= v < p
        if v not in out:
            out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def fe_table(field, kind):
    """(a values, b values): "binary" is the full cross of the edge set plus 2,000 random pairs,
    "unary" the edge set plus 2,000 random values, "inv" the edge set plus 200"""
    _, p, N = FE_FIELDS[field]
    rng = random.Random(f"fe-{field}-{kind}")
    e = edge_values(p, N)
    if kind == "binary":
        a = [x for x in e for _ in e] + [rng.randrange(p) for _ in range(2000)]
        b = [y for _ in e for y in e] + [rng.randrange(p) for _ in range(2000)]
    else:
        a = e + [rng.randrange(p) for _ in range(200 if kind == "inv" else 2000)]
        b = list(a)
    return a, b


def fe_kind(op):
    return "binary" if op in FE_BINARY else "inv" if op in FE_INVERSIONS else "unary"


def fe_ref(op, a, b, p, R):
    """the operation on integers; Montgomery form is x R mod p"""
    Ri = pow(R, -1, p)
    if op in ("mul", "mul_body"):
        return a * b * Ri % p
    if op == "sqr":
        return a * a * Ri % p
    if op == "add":
        return (a + b) % p
    if op == "sub":
        return (a - b) % p
    if op == "neg":
        return -a % p
    if op == "dbl":
        return 2 * a % p
    if op.startswith("small"):
        return int(op[5:]) * a % p
    if op == "to_mont":
        return a * R % p
    if op == "from_mont":
        return a * Ri % p
    if op in FE_INVERSIONS:  # a R -> a^-1 R; 0 -> 0 as the code states
        return pow(a, -1, p) * R * R % p if a else 0
    raise ValueError(op)


def run_fe(field, op, a, b, on_device):
    fid, _, N = FE_FIELDS[field]
    wa, wb = to_words(a, N), to_words(b, N)
    out = np.zeros_like(wa)
    st = lib().vkc_fe(fid, FE_OPS.index(op), len(a), _ptr(wa), _ptr(wb), _ptr(out), int(on_device))
    if st != VC_OK:
        raise CheckLibError("vkc_fe", st)
    return out


def check_fe(field, op, a, b, out, R=None):
    """exact equality of the canonical result words with the integers"""
    _, p, N = FE_FIELDS[field]
    R = R or 1 << (32 * N)
    got = from_words(out)
    assert len(got) == len(a)
    for x, y, g in zip(a, b, got):
        want = fe_ref(op, x, y, p, R)
        assert g == want, f"{field} {op}: a = {x:#x}, b = {y:#x}: got {g:#x}, want {want:#x}"


# ================================================================ (b) limb engines
LIMB_SETS = {  # name -> (id of vkc_limb, radix bits)
    "bls12_381_fq": (0, 29),
    "bn254_fq": (1, 29),
    "bls12_381_fr": (2, 29),
    "bn254_fr": (3, 29),
    "bls12_381_fq_s30": (4, 30),
}
LIMB_OPS = ["mul", "sqr", "mul2sum", "add", "mul_raw1", "mul_raw2", "sub4", "sub16", "sub2_8", "neg4", "canon", "pack",
            "unpack", "from_mont32", "to_mont32", "is_zero_mo"]


def limb_geometry(name):
    if LIMB_SETS[name][1] == 30:
        return lb.P30, lb.L30, lb.N30
    return lb.FIELDS29[name]


def limb_ops(name):
    _, bits = LIMB_SETS[name]
    L = limb_geometry(name)[1]
    if bits == 30:  # signed values: no K p constants, no raw sums as operands (ff30.hpp header)
        return [o for o in LIMB_OPS if o not in ("mul_raw1", "mul_raw2", "sub2_8")]
    return [o for o in LIMB_OPS if o != "mul_raw2" or L <= 9]


def limbs29(v, L):
    return [(v >> (29 * j)) & lb.M29 for j in range(L - 1)] + [v >> (29 * (L - 1))]


def limbs30(v, L=lb.L30):
    """centred limbs in [-2^29, 2^29), the top limb takes the rest (v of either sign)"""
    out = []
    for _ in range(L - 1):
        d = ((v + (1 << 29)) & ((1 << 30) - 1)) - (1 << 29)
        out.append(d)
        v = (v - d) >> 30
    return out + [v]


def ulimbs30(v, L=lb.L30):
    return [(v >> (30 * j)) & ((1 << 30) - 1) for j in range(L - 1)] + [v >> (30 * (L - 1))]


def _limb_array(rows, signed):
    a = np.array(rows, dtype=np.int64)
    if signed:
        assert a.min() >= -(1 << 31) and a.max() < (1 << 31)
        return a.astype(np.int32).view(np.uint32).copy()
    assert a.min() >= 0 and a.max() < (1 << 32)
    return a.astype(np.uint32)


def _limb_rows(arr, signed):
    a = np.ascontiguousarray(arr, dtype=np.uint32)
    return (a.view(np.int32) if signed else a).tolist()


@functools.lru_cache(maxsize=None)
def limb_operands(name):
    """operand classes of the host check programs (tests/cpp/ff29_check.cpp, ff30_check.cpp) plus the
    canonical edge values of (a) converted in: {"normal": below about p, limbs normalised,
    "stress": the extremes of the stated limb bounds, value about 4 p}"""
    p, L, N = limb_geometry(name)
    bits = LIMB_SETS[name][1]
    rng = random.Random(f"limb-{name}")
    edges = edge_values(p, N)
    if bits == 29:
        ptop = p >> (29 * (L - 1))
        normal = [limbs29(v, L) for v in edges]
        normal += [[rng.getrandbits(29) for _ in range(L - 1)] + [rng.randrange(ptop + 1)] for _ in range(120)]
        hi = lb.M29 + 8  # 2^29 + 7: the "almost normalised" limit
        stress = [[hi] * (L - 1) + [4 * ptop], [lb.M29] * (L - 1) + [4 * ptop], [hi] * (L - 1) + [0]]
        stress += [[rng.choice((hi, lb.M29, 0, hi - 1)) for _ in range(L - 1)] + [rng.choice((4 * ptop, ptop, 0))]
                   for _ in range(12)]
    else:
        ptop = p >> (30 * (L - 1))
        top = 4 * ptop
        normal = [limbs30(v) for v in edges] + [limbs30(-v) for v in edges[:12]]
        normal += [[rng.randrange(-(1 << 29), 1 << 29) for _ in range(L - 1)] + [rng.randrange(-top, top + 1)]
                   for _ in range(120)]
        lo, hi = -(1 << 29), (1 << 29) + 2  # exact minimum, near-limb stress of ff30_check.cpp
        stress = [[lo] * (L - 1) + [-top], [hi] * (L - 1) + [top], [lo] * (L - 1) + [top], [hi] * (L - 1) + [-top]]
        stress += [[rng.choice((lo, hi, 0, (1 << 29) - 1)) for _ in range(L - 1)] + [rng.choice((top, -top, 0))]
                   for _ in range(12)]
    return {"normal": normal, "stress": stress}


def _mix(rng, ops, n, stress):
    """n operands: every stress operand first, then a seeded shuffle of the rest"""
    pool = list(ops["normal"]) + (list(ops["stress"]) if stress else [])
    picks = (list(ops["stress"]) if stress else []) + [rng.choice(pool) for _ in range(n)]
    return picks[:n]


@functools.lru_cache(maxsize=None)
def limb_table(name, op):
    """operand rows (a, b, c, d) of one operation, each inside the operation's stated contract"""
    p, L, N = limb_geometry(name)
    bits = LIMB_SETS[name][1]
    ops = limb_operands(name)
    rng = random.Random(f"limb-{name}-{op}")
    n = 240
    zero = [0] * L
    stress = ops["stress"]
    if op in ("mul", "mul2sum", "add", "mul_raw1", "mul_raw2", "sqr", "to_mont32"):
        a, b, c, d = (_mix(rng, ops, n, True) for _ in range(4))
        # all four operands at the same extreme (the column bound), and crossed extremes
        for i, s in enumerate(stress[:4]):
            a[i], b[i], c[i], d[i] = s, s, s, s
        for i, s in enumerate(stress[:4]):
            a[4 + i], b[4 + i], c[4 + i], d[4 + i] = s, stress[(i + 1) % 4], stress[(i + 2) % 4], s
    elif op == "sub16":  # subtrahend below 15 p: the stress operands (about 4 p) are inside
        a, b = _mix(rng, ops, n, True), _mix(rng, ops, n, True)
        c = d = [zero] * n
    elif op in ("sub4", "sub2_8", "neg4"):  # subtrahends below 3 p (sub2_8: their sum below 7 p)
        a = _mix(rng, ops, n, True)
        b, c = _mix(rng, ops, n, False), _mix(rng, ops, n, False)
        if op == "neg4":
            a = b
        d = [zero] * n
    elif op == "canon":  # values below 4 p (radix 2^29) / |value| below 8 p (radix 2^30)
        base = edge_values(p, N) + [rng.randrange(p) for _ in range(40)]
        if bits == 29:
            a = [limbs29(v + k * p, L) for v in base for k in range(4)]
        else:
            a = [limbs30(v + k * p) for v in base for k in (-7, -4, -1, 0, 1, 3, 6)]
        a += ops["normal"]
        b = c = d = [zero] * len(a)
    elif op in ("pack", "unpack", "from_mont32"):  # canonical values
        vals = edge_values(p, N) + [rng.randrange(p) for _ in range(150)]
        if op == "pack":
            a = [limbs29(v, L) if bits == 29 else ulimbs30(v) for v in vals]
        else:
            a = [to_words([v], N)[0].tolist() + [0] * (L - N) for v in vals]
        b = c = d = [zero] * len(a)
    elif op == "is_zero_mo":  # fully normalised product outputs: below 2 p / |value| below p
        vals = edge_values(p, N) + [rng.randrange(p) for _ in range(60)]
        if bits == 29:
            a = [limbs29(v + k * p, L) for v in vals for k in (0, 1)]
        else:
            a = [limbs30(v) for v in vals] + [limbs30(-v) for v in vals]
        b = c = d = [zero] * len(a)
    else:
        raise ValueError(op)
    return a, b, c, d


def run_limb(name, op, rows, on_device):
    sid, bits = LIMB_SETS[name]
    L = limb_geometry(name)[1]
    signed_in = bits == 30 and op not in ("pack", "unpack", "from_mont32")
    arrs = [_limb_array(r, signed_in) for r in rows]
    out = np.zeros_like(arrs[0])
    st = lib().vkc_limb(sid, LIMB_OPS.index(op), len(rows[0]), *(_ptr(x) for x in arrs), _ptr(out), int(on_device))
    if st != VC_OK:
        raise CheckLibError("vkc_limb", st)
    assert out.shape[1] == L
    return out


def check_limb(name, op, rows, out, run_more):
    """congruence mod p and the limb / magnitude bounds of limb_bounds.py on every record.
    run_more(op, rows) evaluates a follow-up operation (the round trip of from_mont32)."""
    p, L, N = limb_geometry(name)
    bits = LIMB_SETS[name][1]
    a, b, c, d = rows
    s30 = bits == 30
    val = lb.val30 if s30 else lb.val29
    res = _limb_rows(out, s30 and op not in ("canon", "pack", "to_mont32", "is_zero_mo"))
    Rp, R = 1 << (bits * L), 1 << (32 * N)

    def rec(kind, i, **kw):
        dd = {"op": kind, "r": res[i]}
        dd.update(kw)
        ok = lb.check30(dd) if s30 else lb.check29(dd, p, L, N)
        assert ok, kind

    back = None
    if op == "from_mont32":
        zero = [[0] * L] * len(a)
        back = run_more("to_mont32", (res, zero, zero, zero))
    for i in range(len(a)):
        if op == "mul":
            rec("mul", i, a=a[i], b=b[i])
        elif op == "sqr":
            rec("mul", i, a=a[i], b=a[i])
        elif op == "mul2sum":
            rec("mul2", i, a=a[i], b=b[i], c=c[i], d=d[i])
        elif op == "add":
            rec("add", i, a=a[i], b=b[i])
        elif op == "mul_raw1":
            rec("mul", i, a=[x + y for x, y in zip(a[i], b[i])], b=b[i])
        elif op == "mul_raw2":
            s = [x + y for x, y in zip(a[i], b[i])]
            rec("mul", i, a=s, b=s)
        elif op in ("sub4", "sub16"):
            rec("sub" if s30 else op, i, a=a[i], b=b[i])
        elif op == "sub2_8":  # a - b - c + 8 p: the record of a sub with the subtrahend b + c (K = 8)
            assert val(res[i]) == val(a[i]) - val(b[i]) - val(c[i]) + 8 * p
            assert all(v <= lb.M29 + 7 for v in res[i][:-1])
        elif op == "neg4":
            if s30:
                assert val(res[i]) == -val(a[i]) and lb.near30(res[i])
            else:  # 4 p - a: the record of sub4 with a zero minuend
                rec("sub4", i, a=[0] * L, b=a[i])
        elif op == "canon":
            rec("canon", i, a=a[i])
            if not s30:
                assert res[i] == limbs29(val(a[i]) % p, L)
            else:
                assert res[i] == ulimbs30(val(a[i]) % p)
        elif op == "pack":
            v = lb.val29(a[i]) if not s30 else lb.val30(a[i])
            assert lb.val32(res[i][:N]) == v and not any(res[i][N:])
        elif op == "unpack":
            v = lb.val32(a[i][:N])
            if s30:
                assert val(res[i]) == v and lb.near30(res[i])
            else:
                rec("unpack", i, a=limbs29(v, L))
        elif op == "from_mont32":
            v = lb.val32(a[i][:N])
            bw = _limb_rows(back, False)[i][:N]
            if s30:
                rec("mont", i, a=a[i][:N], back=bw)
                assert lb.exact30(res[i])
            else:
                rec("mont", i, a=limbs29(v, L), back=bw)
                assert all(x <= lb.M29 for x in res[i][:-1])
        elif op == "to_mont32":  # exact: the canonical words of a R / R'
            assert lb.val32(res[i][:N]) == val(a[i]) * R * pow(Rp, -1, p) % p and not any(res[i][N:])
        elif op == "is_zero_mo":
            if s30:  # |value| < p: zero iff every limb is zero
                assert abs(val(a[i])) < p
            assert res[i][0] == (1 if val(a[i]) % p == 0 else 0) and not any(res[i][1:])
        else:
            raise ValueError(op)


# ================================================================ (c) group law
CURVE_IDS = {"bn254": 0, "bls12_381": 1, "bandersnatch": 2}
PT_OPS = ["madd", "add", "dbl", "to_aff", "to_aff_bin", "store", "pack_aff"]
ENGINES = {"ec": 0, "fast": 1}
CHAIN_MAX = 32
CASE_WORDS = 8 + 2 * CHAIN_MAX


def engine_ops(curve, engine):
    if engine == "ec":
        return PT_OPS[:6]
    return ["madd", "add", "store", "pack_aff"] + ([] if curve == "bandersnatch" else ["dbl"])


def curve_geometry(curve):
    c = curves.CURVES[curve]
    N = c.fbytes // 4
    return c, c.p, N, 1 << (32 * N)


def fast_radix(curve):
    """R' of the curve's Fast29 engine: 13 signed 30-bit limbs at BLS12-381, 29-bit limbs elsewhere"""
    return 1 << (30 * 13) if curve == "bls12_381" else 1 << (29 * 9)


def base_words(curve, pts):
    """ec.hpp affine layout in Montgomery form: x, y (and d x y on the Edwards curve)"""
    c, p, N, R = curve_geometry(curve)
    rows = []
    for (x, y) in pts:
        coords = [x * R % p, y * R % p]
        if c.kind == "te":
            coords.append(c.d * x * y * R % p)
        rows.append(np.concatenate([to_words([v], N)[0] for v in coords]))
    return _u32(np.stack(rows))


def chain_value(c, bases, chain):
    acc = c.identity()
    for idx, sign in chain:
        acc = c.add(acc, c.neg(bases[idx]) if sign else bases[idx])
    return acc


class PointTables:
    """bases and, per operation, cases with their expected affine results"""

    NRAND = 24

    def __init__(self, curve):
        self.curve = curve
        c = self.c = curves.CURVES[curve]
        rng = self.rng = random.Random(f"points-{curve}")
        self.bases = curves.random_points(c, self.NRAND, rng)
        self.order2 = self.ident = None
        if c.kind == "te":
            self.ident = self._base((0, 1))
            self.order2 = self._base((0, c.p - 1))
        self.cases = {op: [] for op in PT_OPS}
        self._build()

    def _base(self, pt):
        self.bases.append(pt)
        return len(self.bases) - 1

    def chain(self, lo=1, hi=CHAIN_MAX):
        return [(self.rng.randrange(self.NRAND), self.rng.randrange(2)) for _ in range(self.rng.randint(lo, hi))]

    def lam(self):
        return 1 + self.rng.randrange(self.NRAND)

    def value(self, chain):
        return chain_value(self.c, self.bases, chain)

    def add_case(self, kind):
        """one case of the general add (also the cases of add_quad): (label, p, plam, q, qlam)"""
        ch = self.chain()
        flip = [(i, 1 - s) for i, s in ch]
        te = self.c.kind == "te"
        table = {
            "random": (ch, 0, self.chain(), 0),
            "same_words": (ch, 0, ch, 0),
            "same_rescaled": (ch, 0, ch, self.lam()),
            "opposite": (ch, 0, flip, 0),
            "opposite_rescaled": (ch, self.lam(), flip, 0),
            "p_identity": ([], 0, ch, 0),
            "q_identity": (ch, 0, [], 0),
            "both_identity": ([], 0, [], 0),
            "cancelled_chain": (ch[:3] + flip[:3][::-1], 0, self.chain(), 0),  # an identity the adds made
            "short_chains": (self.chain(1, 1), 0, self.chain(1, 2), 0),
        }
        if te:
            table.update({
                "identity_zz": ([], self.lam(), ch, 0),           # (0 : Z : Z), Z != 1
                "identity_zz_both": ([], self.lam(), [], self.lam()),
                "order2": ([(self.order2, 0)], 0, ch, 0),
                "order2_twice": ([(self.order2, 0)], 0, [(self.order2, 1)], self.lam()),
                "order2_acc": (ch, 0, [(self.order2, 0)], 0),
                "cancellation": (ch, self.lam(), flip, self.lam()),  # P + (-P)
            })
        p, plam, q, qlam = table[kind]
        return {"label": kind, "p": p, "plam": plam, "q": q, "qlam": qlam, "aff": 0, "neg": 0,
                "want": self.c.add(self.value(p), self.value(q))}

    EXCEPTIONAL = ["same_words", "same_rescaled", "opposite", "opposite_rescaled", "p_identity", "q_identity",
                   "both_identity", "cancelled_chain"]

    def add_kinds(self):
        kinds = ["random"] * 16 + self.EXCEPTIONAL * 2 + ["short_chains"] * 4
        if self.c.kind == "te":
            kinds += ["identity_zz", "identity_zz_both", "order2", "order2_twice", "order2_acc", "cancellation"] * 2
        return kinds

    def _build(self):
        c, rng = self.c, self.rng
        te = c.kind == "te"
        I = c.identity()
        self.cases["add"] = [self.add_case(k) for k in self.add_kinds()]
        # mixed adds
        madd = []

        def m(label, p, plam, aff, neg):
            q = self.bases[aff]
            madd.append({"label": label, "p": p, "plam": plam, "q": [], "qlam": 0, "aff": aff, "neg": neg,
                         "want": c.add(self.value(p), c.neg(q) if neg else q)})

        for _ in range(16):
            m("random", self.chain(), 0, rng.randrange(self.NRAND), rng.randrange(2))
        for _ in range(4):
            m("p_identity", [], 0, rng.randrange(self.NRAND), rng.randrange(2))
            m("rescaled_acc", self.chain(), self.lam(), rng.randrange(self.NRAND), rng.randrange(2))
        for _ in range(4):  # the exceptional branches: acc's own affine point and its negation
            ch = self.chain()
            A = self.value(ch)
            if A == I:
                continue
            own, opp = self._base(A), self._base(c.neg(A))
            lam = self.lam()
            m("own_point", ch, 0, own, 0)            # doubling
            m("own_point_neg", ch, 0, own, 1)        # cancels
            m("negation", ch, 0, opp, 0)             # cancels
            m("negation_neg", ch, 0, opp, 1)         # doubling through the sign
            m("own_point_rescaled", ch, lam, own, 0)
            m("negation_rescaled", ch, lam, opp, 0)
        for i in range(3):  # a one-add accumulator (ZZ = 1) meeting its own base
            m("base_twice", [(i, 0)], 0, i, 0)
            m("base_minus_base", [(i, 1)], 0, i, 0)
        if te:
            m("identity_base", self.chain(), 0, self.ident, 0)
            m("identity_base_neg", self.chain(), 0, self.ident, 1)
            m("order2_base", self.chain(), 0, self.order2, 0)
            m("order2_base_on_identity_zz", [], self.lam(), self.order2, 1)
            m("order2_twice", [(self.order2, 0)], 0, self.order2, 0)
        self.cases["madd"] = madd
        # doublings, normalisations, stores: one operand
        single = [("random", self.chain(), 0) for _ in range(12)]
        single += [("rescaled", self.chain(), self.lam()) for _ in range(4)]
        single += [("identity", [], 0), ("cancelled_chain", [(1, 0), (2, 1), (2, 0), (1, 1)], 0), ("one_add", [(3, 1)], 0)]
        if te:
            single += [("identity_zz", [], self.lam()), ("order2", [(self.order2, 0)], 0),
                       ("order2_rescaled", [(self.order2, 1)], self.lam())]
        for op in ("dbl", "to_aff", "to_aff_bin", "store"):
            for label, ch, lam in single:
                v = self.value(ch)
                self.cases[op].append({"label": label, "p": ch, "plam": lam, "q": [], "qlam": 0, "aff": 0, "neg": 0,
                                       "want": c.add(v, v) if op == "dbl" else v})
        self.cases["pack_aff"] = [{"label": f"base{i}", "p": [], "plam": 0, "q": [], "qlam": 0, "aff": i, "neg": 0,
                                   "want": self.bases[i]} for i in range(len(self.bases))]

    def base_words(self):
        return base_words(self.curve, self.bases)


@functools.lru_cache(maxsize=None)
def point_tables(curve):
    return PointTables(curve)


def case_words(cases):
    out = np.zeros((len(cases), CASE_WORDS), dtype=np.uint32)
    for i, cs in enumerate(cases):
        assert len(cs["p"]) <= CHAIN_MAX and len(cs["q"]) <= CHAIN_MAX
        out[i, :6] = [len(cs["p"]), len(cs["q"]), cs["plam"], cs["qlam"], cs["aff"], cs["neg"]]
        for k, (idx, sign) in enumerate(cs["p"]):
            out[i, 8 + k] = idx << 1 | sign
        for k, (idx, sign) in enumerate(cs["q"]):
            out[i, 8 + CHAIN_MAX + k] = idx << 1 | sign
    return out


def run_point(curve, engine, op, cases, bases_w, on_device):
    N = curve_geometry(curve)[2]
    cw = case_words(cases)
    out = np.zeros((len(cases), 4 * N + 1), dtype=np.uint32)
    st = lib().vkc_point(CURVE_IDS[curve], ENGINES[engine], PT_OPS.index(op), len(cases), _ptr(bases_w),
                         len(bases_w), _ptr(cw), _ptr(out), int(on_device))
    if st != VC_OK:
        raise CheckLibError("vkc_point", st)
    return out


def acc_to_affine(curve, row, R=None):
    """one record (the ec.hpp accumulator in Montgomery words, then the identity flag) divided out
    on integers: x = X / ZZ, y = Y / ZZZ (XYZZ) or X / Z, Y / Z (extended Edwards); the curve's
    identity for the identity, whose flag must agree. The Montgomery factor cancels in the
    quotients; the coordinate relations are checked with it."""
    c, p, N, R0 = curve_geometry(curve)
    R = R or R0
    w = [lb.val32(row[k * N:(k + 1) * N].tolist()) for k in range(4)]
    flag = int(row[4 * N])
    assert all(v < p for v in w), "non-canonical accumulator words"
    assert flag in (0, 1)
    if c.kind == "sw":
        X, Y, ZZ, ZZZ = w
        if ZZ == 0:
            assert flag == 1, "identity words without the identity flag"
            return None
        assert flag == 0, "identity flag on a finite point"
        assert (ZZ ** 3 - ZZZ ** 2 * R) % p == 0, "ZZ^3 != ZZZ^2"
        return (X * pow(ZZ, -1, p) % p, Y * pow(ZZZ, -1, p) % p)
    X, Y, T, Z = w
    assert Z != 0 and (T * Z - X * Y) % p == 0, "T Z != X Y"
    zi = pow(Z, -1, p)
    pt = (X * zi % p, Y * zi % p)
    assert flag == (1 if pt == (0, 1) else 0), "identity flag"
    return pt


def check_point(curve, engine, op, cases, out, R=None):
    c, p, N, R0 = curve_geometry(curve)
    R = R or R0
    I = c.identity()
    for cs, row in zip(cases, out):
        tag = f"{curve} {engine} {op} [{cs['label']}]"
        want = cs["want"]
        if op == "pack_aff":  # canonical x R' in the 32-bit words of the table layout
            Rp = fast_radix(curve)
            coords = list(want) + ([c.d * want[0] * want[1] % p] if c.kind == "te" else [])
            got = [lb.val32(row[k * N:(k + 1) * N].tolist()) for k in range(len(coords))]
            assert got == [v * Rp % p for v in coords], tag
            continue
        if op in ("to_aff", "to_aff_bin"):  # affine x, y in Montgomery form, then the identity flag
            x, y = (lb.val32(row[k * N:(k + 1) * N].tolist()) for k in range(2))
            flag = int(row[4 * N])
            assert flag == (1 if want == I else 0), tag
            if c.kind == "sw" and flag:
                continue
            Ri = pow(R, -1, p)
            assert (x * Ri % p, y * Ri % p) == want, tag
            continue
        try:
            got = acc_to_affine(curve, row, R)
        except AssertionError as e:
            raise AssertionError(f"{tag}: {e}") from None
        assert got == want, f"{tag}: got {got}, want {want}"


# ================================================================ (d) add_quad
QUAD_WAVES = ["random", "exceptional", "interleaved", "partial20"]


@functools.lru_cache(maxsize=None)
def quad_wave(curve, wave):
    """the cases of one wave, one per quad"""
    t = point_tables(curve)
    exc = t.EXCEPTIONAL
    kinds = {
        "random": ["random"] * 16,
        "exceptional": exc * 2,
        "interleaved": [exc[i // 2 % len(exc)] if i % 2 == 0 else "random" for i in range(16)],
        "partial20": ["random", "same_words", "opposite_rescaled", "random", "q_identity"],
    }[wave]
    return tuple(t.add_case(k) for k in kinds)


def run_quad(curve, cases, bases_w):
    N = curve_geometry(curve)[2]
    cw = case_words(cases)
    lanes = 4 * len(cases)
    out = np.zeros((lanes, 4 * N + 1), dtype=np.uint32)
    st = lib().vkc_quad(CURVE_IDS[curve], lanes, _ptr(bases_w), len(bases_w), _ptr(cw), _ptr(out))
    if st != VC_OK:
        raise CheckLibError("vkc_quad", st)
    return out


# ================================================================ (e) fb_block_sum_store
def block_patterns(curve, nt):
    """[(label, {lane: chain})] -- lanes not named hold the identity"""
    t = point_tables(curve)
    rng = random.Random(f"blocks-{curve}-{nt}")
    P = [(0, 0)]
    nP = [(0, 1)]
    Q = [(5, 0), (7, 1)]
    pats = [("all_identity", {})]
    for lane in (0, 3, 4, 63, 64, 255):
        if lane < nt:
            pats.append((f"single_lane_{lane}", {lane: [(2, 1), (9, 0)]}))
    pats.append(("same_point_everywhere", {lane: P for lane in range(nt)}))       # every level doubles
    pats.append(("alternating_P_minus_P", {lane: (P if lane % 2 == 0 else nP) for lane in range(nt)}))
    pats.append(("pair_inside_quad", {1: P, 2: nP, nt - 1: Q}))
    for dist in (4, 8, 16, 32):
        pats.append((f"pair_xor_{dist}", {2: P, 2 ^ dist: nP, nt - 1: Q}))
    if nt > 64:
        pats.append(("pair_across_waves", {5: P, 64 + 5: nP, nt - 1: Q}))
        pats.append(("pair_across_waves_far", {70: P, 192 + 9: nP, 3: Q}))
    for k in range(2):
        lanes = {}
        for lane in range(nt):
            if rng.random() < 0.8:
                lanes[lane] = [(rng.randrange(t.NRAND), rng.randrange(2)) for _ in range(rng.randint(1, 3))]
        pats.append((f"random_with_identities_{k}", lanes))
    return pats


def run_block_sum(curve, nt, pats, bases_w):
    N = curve_geometry(curve)[2]
    spec = np.zeros((len(pats), nt, 4), dtype=np.uint32)
    for b, (_, lanes) in enumerate(pats):
        for lane, ch in lanes.items():
            spec[b, lane, 0] = len(ch)
            for k, (idx, sign) in enumerate(ch):
                spec[b, lane, 1 + k] = idx << 1 | sign
    out = np.zeros((len(pats), 4 * N), dtype=np.uint32)
    st = lib().vkc_block_sum(CURVE_IDS[curve], nt, len(pats), _ptr(bases_w), len(bases_w), _ptr(spec), _ptr(out))
    if st != VC_OK:
        raise CheckLibError("vkc_block_sum", st)
    return out


def block_sum_want(curve, lanes):
    t = point_tables(curve)
    acc = t.c.identity()
    for ch in lanes.values():
        acc = t.c.add(acc, t.value(ch))
    return acc


def block_sum_record(curve, row):
    """the stored accumulator as a record of acc_to_affine: the flag is what the words say"""
    c, p, N, _ = curve_geometry(curve)
    if c.kind == "sw":
        flag = 0 if any(row[2 * N:3 * N]) else 1
    else:
        X, Y, _, Z = (lb.val32(row[k * N:(k + 1) * N].tolist()) for k in range(4))
        flag = 1 if X == 0 and Y == Z else 0
    return np.concatenate([row, np.array([flag], dtype=np.uint32)])

"""The congruences and bounds of the limb engines (csrc/ff29.hpp, csrc/ff30.hpp) as assertions on
one record: the integer limbs of the operands ("a", "b", "c", "d") and of the result ("r") of one
operation. tests/test_ff29.py and tests/test_ff30.py feed it the lines of their host check
programs, tests/test_arith_host.py and tests/test_gpu_arith.py the words of the check library
(arith_cases.py), host and device. The bounds are the ones the kernels' bound analysis relies on
(ec29.hpp and ec30.hpp headers); every record kind asserts the same thing for every caller."""

BN254_FQ = 21888242871839275222246405745257275088696311157297823662689037894645226208583
BN254_FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BLS_FQ = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
BLS_FR = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001

# radix-2^29 sets: name -> (p, L limbs, N 32-bit words)
FIELDS29 = {
    "bls12_381_fq": (BLS_FQ, 14, 12),
    "bn254_fq": (BN254_FQ, 9, 8),
    "bls12_381_fr": (BLS_FR, 9, 8),
    "bn254_fr": (BN254_FR, 9, 8),
}
M29 = (1 << 29) - 1

# the signed radix-2^30 set (BLS12-381 Fq)
P30 = BLS_FQ
L30 = 13
N30 = 12
RP30 = 1 << (30 * L30)
R32_30 = 1 << 384
H30 = 1 << 29


def val29(limbs):
    return sum(v << (29 * j) for j, v in enumerate(limbs))


def val30(limbs):
    return sum(v << (30 * j) for j, v in enumerate(limbs))


def val32(words):
    return sum(w << (32 * k) for k, w in enumerate(words))


def check29(d, p, L, N):
    """one record of a radix-2^29 operation; returns False for a kind it does not know"""
    Rp = 1 << (29 * L)
    R = 1 << (32 * N)
    r = val29(d["r"])
    op = d["op"]
    if op == "mul":
        a, b = val29(d["a"]), val29(d["b"])
        assert (r * Rp - a * b) % p == 0
        assert r < a * b // Rp + p
        assert all(v <= M29 for v in d["r"][:-1])
    elif op == "mul2":
        s = val29(d["a"]) * val29(d["b"]) + val29(d["c"]) * val29(d["d"])
        assert (r * Rp - s) % p == 0
        assert r < s // Rp + p
        assert all(v <= M29 for v in d["r"][:-1])
    elif op == "add":
        assert r == val29(d["a"]) + val29(d["b"])
        assert all(v <= M29 + 7 for v in d["r"][:-1])
    elif op in ("sub4", "sub16"):
        k = int(op[3:])
        a, b = val29(d["a"]), val29(d["b"])
        assert r == a - b + k * p
        assert all(v <= M29 + 7 for v in d["r"][:-1])
    elif op == "canon":
        assert r < p and (r - val29(d["a"])) % p == 0
    elif op == "unpack":
        assert r == val29(d["a"])
    elif op == "mont":
        v = val29(d["a"])
        assert (r - v * Rp * pow(R, -1, p)) % p == 0
        assert val32(d["back"]) == v
    else:
        return False
    return True


def check29_zero_mo(d, p):
    """is_zero_mo29 (product outputs below 2p) agrees with the residue: "a" of a mont record is
    canon(r) of the same iteration's product"""
    assert d["zero_mo"] == (1 if val29(d["a"]) % p == 0 else 0)


def exact30(limbs):
    return all(-H30 <= v < H30 for v in limbs[:-1])


def near30(limbs):
    return all(-H30 - 2 <= v < H30 + 2 for v in limbs[:-1])


def check30(d):
    """one record of a signed radix-2^30 operation; returns False for a kind it does not know"""
    op = d["op"]
    if op == "mul":
        a, b, r = val30(d["a"]), val30(d["b"]), val30(d["r"])
        assert (r * RP30 - a * b) % P30 == 0
        assert abs(r) < abs(a * b) // RP30 + P30 // 2 + (P30 >> 29)
        assert exact30(d["r"])
    elif op == "mul2":
        s = val30(d["a"]) * val30(d["b"]) + val30(d["c"]) * val30(d["d"])
        r = val30(d["r"])
        assert (r * RP30 - s) % P30 == 0
        assert abs(r) < abs(s) // RP30 + P30 // 2 + (P30 >> 29)
        assert exact30(d["r"])
    elif op == "add" and "r" in d:
        assert val30(d["r"]) == val30(d["a"]) + val30(d["b"]) and near30(d["r"])
    elif op == "sub":
        assert val30(d["r"]) == val30(d["a"]) - val30(d["b"]) and near30(d["r"])
    elif op == "canon":
        r = val30(d["r"])
        assert 0 <= r < P30 and (r - val30(d["a"])) % P30 == 0
    elif op == "mont":
        a = val32(d["a"])
        assert val32(d["back"]) == a
        assert (val30(d["r"]) - a * RP30 * pow(R32_30, -1, P30)) % P30 == 0
    else:
        return False
    return True

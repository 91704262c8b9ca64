#!/usr/bin/env python3
"""Generate csrc/pairing_bls_consts.hpp: constants of the BLS12-381 ate pairing (pairing_bls.hpp).

Tower: Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), xi = 1 + u, Fq12 = Fq6[w]/(w^2 - v), so
1, w, .., w^5 is a basis of Fq12 over Fq2 with w^6 = xi. Everything below is derived here with
Python integers and checked by assertions; nothing is typed in except the curve's parameter x and
the two generators.

  FROB[i][k]  xi^(k (p^i - 1) / 6), i = 1..3, k = 0..5: the Frobenius p^i multiplies the
              (conjugated i times) coefficient of w^k by it
  TWIST_B     4 xi (the M-type twist y^2 = x^3 + 4 (1 + u))
  G2_X, G2_Y  the G2 generator H (on the twist, of order r)
  G1_X, G1_Y  the G1 generator G
  BETA2       the cube root of unity with (BETA2 x, y) = -[z^2] (x, y) on G1 (the subgroup test)
  Z2          z^2 = x^2, 128 bits
  X           |x|; the Miller loop and the final exponentiation's powers run over its 64 bits
Field elements are Montgomery residues a 2^384 mod p in twelve 32-bit limbs (ff.hpp BLS381Fq).
"""
import os
import sys

X = -0xd201000000010000
R = X ** 4 - X ** 2 + 1
P = (X - 1) ** 2 * R // 3 + X
XI = (1, 1)
G = (int("17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb", 16),
     int("08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1", 16))
H = ((int("024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8", 16),
      int("13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e", 16)),
     (int("0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801", 16),
      int("0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be", 16)))


def f2add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2mul(r, a)
        a = f2mul(a, a)
        e >>= 1
    return r


def f2inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * n % P, -a[1] * n % P)


def ec_add(p, q, ops):
    """affine addition on y^2 = x^3 + b over the field given by ops (None: the identity)"""
    add, sub, mul, inv, small = ops
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if p[1] != q[1] or p[1] == small(0):
            return None
        lam = mul(mul(small(3), mul(p[0], p[0])), inv(add(p[1], p[1])))
    else:
        lam = mul(sub(q[1], p[1]), inv(sub(q[0], p[0])))
    x3 = sub(sub(mul(lam, lam), p[0]), q[0])
    return (x3, sub(mul(lam, sub(p[0], x3)), p[1]))


def ec_mul(p, k, ops):
    r = None
    for b in bin(k)[2:]:
        r = ec_add(r, r, ops)
        if b == "1":
            r = ec_add(r, p, ops)
    return r


FQ = (lambda a, b: (a + b) % P, lambda a, b: (a - b) % P, lambda a, b: a * b % P, lambda a: pow(a, -1, P),
      lambda k: k % P)
FQ2 = (f2add, f2sub, f2mul, f2inv, lambda k: (k % P, 0))


def hard_part_exponent():
    """the exponent the chain of final_exp computes, in integers, step by step as the code does"""
    y0 = X - 1                      # r^x conj(r)
    y1 = y0 * (X - 1)               # y0^x conj(y0)
    y2 = y1 * X + y1 * P            # y1^x frob(y1, 1)
    y3 = y2 * X * X + y2 * P * P - y2  # (y2^x)^x frob(y2, 2) conj(y2)
    return y3 + 3                   # y3 r^2 r


def limbs(x):
    x = x * (1 << 384) % P
    return ", ".join(f"0x{(x >> (32 * i)) & 0xffffffff:08x}u" for i in range(12))


def main():
    assert X < 0 and bin(-X).count("1") == 6 and (-X).bit_length() == 64
    assert R == 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
    assert P.bit_length() == 381 and P % 4 == 3 and (X - 1) ** 2 * R % 3 == 0
    assert P & 0xffffffff == 0xffffaaab and P >> 352 == 0x1a0111ea  # ff.hpp BLS381Fq
    assert f2pow(XI, (P * P - 1) // 2) != (1, 0) and f2pow(XI, (P * P - 1) // 3) != (1, 0)  # w^6 = xi irreducible
    tb = f2mul((4, 0), XI)
    hx, hy = H
    assert f2mul(hy, hy) == f2add(f2mul(f2mul(hx, hx), hx), tb)
    assert ec_mul(H, R, FQ2) is None
    assert G[1] * G[1] % P == (G[0] ** 3 + 4) % P and ec_mul(G, R, FQ) is None
    # the subgroup test phi^2(P) + [z^2] P = O: r = z^4 - z^2 + 1, and phi^2 = (beta2 x, y) acts on G1 as -z^2
    z2 = X * X
    assert z2 * z2 - z2 + 1 == R and z2.bit_length() == 128
    zg = ec_mul(G, z2, FQ)
    beta2 = zg[0] * pow(G[0], -1, P) % P
    assert beta2 != 1 and pow(beta2, 3, P) == 1 and zg[1] == P - G[1]
    # a point of E(Fq) outside G1 fails it: x = 5 (tests use the same point)
    y5 = pow(5 ** 3 + 4, (P + 1) // 4, P)
    assert y5 * y5 % P == 129
    r5 = (5, y5)
    assert ec_mul(r5, R, FQ) is not None
    assert ec_add(ec_mul(r5, z2, FQ), (5 * beta2 % P, y5), FQ) is not None
    # the hard part's chain computes a multiple m (p^4 - p^2 + 1) / r with gcd(m, r) = 1
    cyc = P ** 4 - P ** 2 + 1
    assert cyc % R == 0
    e = hard_part_exponent()
    assert e == (X - 1) ** 2 * (X + P) * (X * X + P * P - 1) + 3
    assert e == 3 * (cyc // R)
    e %= cyc
    assert e % (cyc // R) == 0 and (e // (cyc // R)) % R != 0
    bits = [int(b) for b in bin(-X)[2:]]
    assert bits[0] == 1 and len(bits) == 64
    sq = []  # per line of the Miller loop: 1 when f is squared before it (a doubling step's line)
    for b in bits[1:]:
        sq += [1] + ([0] if b else [])
    assert len(sq) == 68 and sum(sq) == 63
    out = ["// GENERATED by tools/gen_pairing_bls.py -- constants of the BLS12-381 pairing (pairing_bls.hpp).\n",
           "#pragma once\n#include <stdint.h>\n\nnamespace vk {\n\nstruct BLS381Pairing {\n"]
    out.append(f"    static constexpr uint64_t X = {-X}ull;  // |x|; x is negative\n")
    out.append(f"    static constexpr uint64_t Z2_LO = 0x{z2 & (2 ** 64 - 1):016x}ull, Z2_HI = 0x{z2 >> 64:016x}ull;\n")
    out.append(f"    static constexpr int ATE_BITS = {len(bits) - 1};\n")
    out.append(f"    static constexpr int ATE_LINES = {len(sq)};\n")
    out.append("    VK_HD static constexpr int ate_sq(int k) { constexpr int8_t v[ATE_LINES] = {" +
               ", ".join(str(s) for s in sq) + "}; return v[k]; }\n")
    rows = []
    for i in (1, 2, 3):
        for k in range(6):
            g = f2pow(XI, k * (P ** i - 1) // 6)
            rows.append("{" + limbs(g[0]) + "}, {" + limbs(g[1]) + "}")
    out.append("    // FROB[(i - 1) * 12 + 2 k + c]: limb j of component c of xi^(k (p^i - 1) / 6)\n")
    out.append("    VK_HD static constexpr uint32_t frob(int idx, int j) { constexpr uint32_t v[36][12] = {\n        " +
               ",\n        ".join(rows) + "}; return v[idx][j]; }\n")
    consts = [tb[0], tb[1], hx[0], hx[1], hy[0], hy[1]]
    out.append("    // 0, 1: 4 xi; 2, 3: H.x; 4, 5: H.y\n")
    out.append("    VK_HD static constexpr uint32_t g2c(int idx, int j) { constexpr uint32_t v[6][12] = {\n        " +
               ",\n        ".join("{" + limbs(c) + "}" for c in consts) + "}; return v[idx][j]; }\n")
    out.append("    // 0: G.x; 1: G.y; 2: beta2, (beta2 x, y) = -[z^2] (x, y) on G1\n")
    out.append("    VK_HD static constexpr uint32_t g1c(int idx, int j) { constexpr uint32_t v[3][12] = {\n        " +
               ",\n        ".join("{" + limbs(c) + "}" for c in (G[0], G[1], beta2)) + "}; return v[idx][j]; }\n")
    out.append("};\n\n}  // namespace vk\n")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "pairing_bls_consts.hpp")
    open(path, "w").write("".join(out))


if __name__ == "__main__":
    main()

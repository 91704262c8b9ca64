// BLS12-381 ate pairing, host + gfx950 device from one source (constants: pairing_bls_consts.hpp,
// tools/gen_pairing_bls.py). The BN254 pairing is pairing.hpp; the two share no text above ff.hpp
// and ec.hpp (the field engine and the point types), so neither curve's kernels depend on the
// other's source.
//
// Field engine: the canonical 32-bit-limb Montgomery form of ff.hpp (fe<BLS381Fq>, twelve limbs;
// fe_mul_asm12 on the device). Every fe_add / fe_sub / fe_mul result is fully reduced, so the
// tower's chains of additions and subtractions need no operand-bound bookkeeping and "f == 1" at
// the end is a limb compare. An Fq12 is 144 words.
//
// Tower: Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), xi = 1 + u, Fq12 = Fq6[w]/(w^2 - v).
// G2 is the M-type twist y^2 = x^3 + 4 xi; (x, y) on it maps to (x / w^2, y / w^3) on the curve.
//
// Lines. G2 points are kept affine, so a Miller step is a slope lam (Fq2) on the twist and the
// constant c = lam xT - yT. The untwisted slope is lam / w, and the line through the untwisted T
// evaluated at a G1 point (xP, yP) is yP - (lam / w) xP + c / w^3; times w^3 (an element of Fq4,
// which the final exponentiation sends to 1):
//     c + (-lam xP) w^2 + yP w^3  =  (c + (-lam xP) v) + (yP v) w.
// This is where the M-type twist differs from BN254's D-type line yP + b w + c w^3: the Fq
// coefficient sits at w^3 and the two Fq2 coefficients at 1 and w^2. A G1 point in XYZZ
// coordinates is used scaled by ZZ ZZZ (a factor in Fq): yP' = Y ZZ, xP' = X ZZZ, zP' = ZZ ZZZ,
// and the line is c zP' + (-lam xP') w^2 + yP' w^3. The identity pairs to one: its lines are
// skipped.
//
// Miller loop: over the 64 bits of |x|, 63 doublings and 5 additions, no Frobenius end lines; x is
// negative, so f is conjugated once after the loop (f^-1 up to the easy part).
//
// G1 has a cofactor: g1_load tests the subgroup (phi^2(P) + [z^2] P = O), since a point of small
// order pairs to one with everything.
//
// Code size on the device: every multiply / square of the tower is one out-of-line function
// (VK_PFN), and the Miller loop and the powers of x are rolled loops.
#pragma once
#include "ec.hpp"
#include "pairing_bls_consts.hpp"

#ifndef VK_PFN
#ifdef __HIP_DEVICE_COMPILE__
#define VK_PFN __host__ __device__ __attribute__((noinline))
#else
#define VK_PFN __host__ __device__ inline
#endif
#endif

namespace vk {
namespace bls {

using Fq = fe<BLS381Fq>;
using FrE = fe<BLS381Fr>;
using PC = BLS381Pairing;
constexpr int NL = BLS381Fq::N;  // 12

struct Fq2 {
    Fq c0, c1;
};
struct Fq6 {
    Fq2 c0, c1, c2;
};
struct Fq12 {
    Fq6 c0, c1;
};

// ---------------------------------------------------------------- Fq
VK_PFN Fq fq_mul(const Fq& a, const Fq& b) { return fe_mul<BLS381Fq>(a, b); }
VK_PFN Fq fq_add(const Fq& a, const Fq& b) { return fe_add<BLS381Fq>(a, b); }
VK_PFN Fq fq_sub(const Fq& a, const Fq& b) { return fe_sub<BLS381Fq>(a, b); }
VK_HD Fq fq_neg(const Fq& a) { return fq_sub(fe_zero<BLS381Fq>(), a); }
VK_HD Fq fq_inv(const Fq& a) {
#ifdef __HIP_DEVICE_COMPILE__
    return fe_inv<BLS381Fq>(a);
#else
    return fe_inv_bin<BLS381Fq>(a);
#endif
}

// ---------------------------------------------------------------- Fq2
VK_HD Fq2 fq2_zero() { return Fq2{fe_zero<BLS381Fq>(), fe_zero<BLS381Fq>()}; }
VK_HD Fq2 fq2_one() { return Fq2{fe_one<BLS381Fq>(), fe_zero<BLS381Fq>()}; }
VK_HD bool fq2_is_zero(const Fq2& a) { return fe_is_zero<BLS381Fq>(a.c0) && fe_is_zero<BLS381Fq>(a.c1); }
VK_HD bool fq2_eq(const Fq2& a, const Fq2& b) { return fe_eq<BLS381Fq>(a.c0, b.c0) && fe_eq<BLS381Fq>(a.c1, b.c1); }
VK_PFN Fq2 fq2_add(const Fq2& a, const Fq2& b) { return Fq2{fq_add(a.c0, b.c0), fq_add(a.c1, b.c1)}; }
VK_PFN Fq2 fq2_sub(const Fq2& a, const Fq2& b) { return Fq2{fq_sub(a.c0, b.c0), fq_sub(a.c1, b.c1)}; }
VK_HD Fq2 fq2_dbl(const Fq2& a) { return fq2_add(a, a); }
VK_HD Fq2 fq2_neg(const Fq2& a) { return Fq2{fq_neg(a.c0), fq_neg(a.c1)}; }
VK_HD Fq2 fq2_conj(const Fq2& a) { return Fq2{a.c0, fq_neg(a.c1)}; }
VK_HD Fq2 fq2_scale(const Fq2& a, const Fq& k) { return Fq2{fq_mul(a.c0, k), fq_mul(a.c1, k)}; }
// Karatsuba: 3 Fq multiplies
VK_PFN Fq2 fq2_mul(const Fq2& a, const Fq2& b) {
    const Fq v0 = fq_mul(a.c0, b.c0), v1 = fq_mul(a.c1, b.c1);
    const Fq s = fq_mul(fq_add(a.c0, a.c1), fq_add(b.c0, b.c1));
    return Fq2{fq_sub(v0, v1), fq_sub(fq_sub(s, v0), v1)};
}
// (a0 + a1)(a0 - a1) + 2 a0 a1 u
VK_PFN Fq2 fq2_sqr(const Fq2& a) {
    const Fq t = fq_mul(a.c0, a.c1);
    return Fq2{fq_mul(fq_add(a.c0, a.c1), fq_sub(a.c0, a.c1)), fq_add(t, t)};
}
// a (1 + u) = (a0 - a1) + (a0 + a1) u
VK_HD Fq2 fq2_mul_xi(const Fq2& a) { return Fq2{fq_sub(a.c0, a.c1), fq_add(a.c0, a.c1)}; }
VK_HD Fq2 fq2_inv(const Fq2& a) {
    const Fq n = fq_inv(fq_add(fq_mul(a.c0, a.c0), fq_mul(a.c1, a.c1)));
    return Fq2{fq_mul(a.c0, n), fq_neg(fq_mul(a.c1, n))};
}

// ---------------------------------------------------------------- Fq6
VK_HD Fq6 fq6_zero() { return Fq6{fq2_zero(), fq2_zero(), fq2_zero()}; }
VK_HD Fq6 fq6_one() { return Fq6{fq2_one(), fq2_zero(), fq2_zero()}; }
VK_PFN Fq6 fq6_add(const Fq6& a, const Fq6& b) { return Fq6{fq2_add(a.c0, b.c0), fq2_add(a.c1, b.c1), fq2_add(a.c2, b.c2)}; }
VK_PFN Fq6 fq6_sub(const Fq6& a, const Fq6& b) { return Fq6{fq2_sub(a.c0, b.c0), fq2_sub(a.c1, b.c1), fq2_sub(a.c2, b.c2)}; }
VK_HD Fq6 fq6_neg(const Fq6& a) { return Fq6{fq2_neg(a.c0), fq2_neg(a.c1), fq2_neg(a.c2)}; }
// a v: (a0 + a1 v + a2 v^2) v = xi a2 + a0 v + a1 v^2
VK_HD Fq6 fq6_mul_v(const Fq6& a) { return Fq6{fq2_mul_xi(a.c2), a.c0, a.c1}; }
// Karatsuba: 6 Fq2 multiplies
VK_PFN Fq6 fq6_mul(const Fq6& a, const Fq6& b) {
    const Fq2 v0 = fq2_mul(a.c0, b.c0), v1 = fq2_mul(a.c1, b.c1), v2 = fq2_mul(a.c2, b.c2);
    const Fq2 t12 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c1, a.c2), fq2_add(b.c1, b.c2)), v1), v2);
    const Fq2 t01 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c0, a.c1), fq2_add(b.c0, b.c1)), v0), v1);
    const Fq2 t02 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c0, a.c2), fq2_add(b.c0, b.c2)), v0), v2);
    return Fq6{fq2_add(v0, fq2_mul_xi(t12)), fq2_add(t01, fq2_mul_xi(v2)), fq2_add(t02, v1)};
}
// Chung-Hasan SQR2: 2 multiplies + 3 squares
VK_PFN Fq6 fq6_sqr(const Fq6& a) {
    const Fq2 s0 = fq2_sqr(a.c0);
    const Fq2 s1 = fq2_dbl(fq2_mul(a.c0, a.c1));
    const Fq2 s2 = fq2_sqr(fq2_add(fq2_sub(a.c0, a.c1), a.c2));
    const Fq2 s3 = fq2_dbl(fq2_mul(a.c1, a.c2));
    const Fq2 s4 = fq2_sqr(a.c2);
    return Fq6{fq2_add(s0, fq2_mul_xi(s3)), fq2_add(s1, fq2_mul_xi(s4)),
               fq2_sub(fq2_sub(fq2_add(fq2_add(s1, s2), s3), s0), s4)};
}
// a (b0 + b1 v), the sparse factor of a line product
VK_PFN Fq6 fq6_mul_01(const Fq6& a, const Fq2& b0, const Fq2& b1) {
    const Fq2 a0b0 = fq2_mul(a.c0, b0), a1b1 = fq2_mul(a.c1, b1);
    const Fq2 c1 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c0, a.c1), fq2_add(b0, b1)), a0b0), a1b1);
    return Fq6{fq2_add(a0b0, fq2_mul_xi(fq2_mul(a.c2, b1))), c1, fq2_add(a1b1, fq2_mul(a.c2, b0))};
}
VK_HD Fq6 fq6_scale(const Fq6& a, const Fq& k) { return Fq6{fq2_scale(a.c0, k), fq2_scale(a.c1, k), fq2_scale(a.c2, k)}; }
VK_HD Fq6 fq6_inv(const Fq6& a) {
    const Fq2 A = fq2_sub(fq2_sqr(a.c0), fq2_mul_xi(fq2_mul(a.c1, a.c2)));
    const Fq2 B = fq2_sub(fq2_mul_xi(fq2_sqr(a.c2)), fq2_mul(a.c0, a.c1));
    const Fq2 C = fq2_sub(fq2_sqr(a.c1), fq2_mul(a.c0, a.c2));
    const Fq2 F = fq2_add(fq2_mul(a.c0, A), fq2_mul_xi(fq2_add(fq2_mul(a.c2, B), fq2_mul(a.c1, C))));
    const Fq2 Fi = fq2_inv(F);
    return Fq6{fq2_mul(A, Fi), fq2_mul(B, Fi), fq2_mul(C, Fi)};
}

// ---------------------------------------------------------------- Fq12
VK_HD Fq12 fq12_one() { return Fq12{fq6_one(), fq6_zero()}; }
VK_HD Fq12 fq12_conj(const Fq12& a) { return Fq12{a.c0, fq6_neg(a.c1)}; }
VK_HD bool fq12_eq(const Fq12& a, const Fq12& b) {
    return fq2_eq(a.c0.c0, b.c0.c0) && fq2_eq(a.c0.c1, b.c0.c1) && fq2_eq(a.c0.c2, b.c0.c2) &&
           fq2_eq(a.c1.c0, b.c1.c0) && fq2_eq(a.c1.c1, b.c1.c1) && fq2_eq(a.c1.c2, b.c1.c2);
}
// every limb is canonical (ff.hpp), so this is a plain compare with the Montgomery one
VK_HD bool fq12_is_one(const Fq12& a) { return fq12_eq(a, fq12_one()); }
// Karatsuba: 3 Fq6 multiplies
VK_PFN Fq12 fq12_mul(const Fq12& a, const Fq12& b) {
    const Fq6 v0 = fq6_mul(a.c0, b.c0), v1 = fq6_mul(a.c1, b.c1);
    const Fq6 s = fq6_mul(fq6_add(a.c0, a.c1), fq6_add(b.c0, b.c1));
    return Fq12{fq6_add(v0, fq6_mul_v(v1)), fq6_sub(fq6_sub(s, v0), v1)};
}
// complex squaring: 2 Fq6 multiplies
VK_PFN Fq12 fq12_sqr(const Fq12& a) {
    const Fq6 ab = fq6_mul(a.c0, a.c1);
    const Fq6 t = fq6_mul(fq6_add(a.c0, a.c1), fq6_add(a.c0, fq6_mul_v(a.c1)));
    return Fq12{fq6_sub(fq6_sub(t, ab), fq6_mul_v(ab)), fq6_add(ab, ab)};
}
VK_PFN Fq12 fq12_inv(const Fq12& a) {
    const Fq6 t = fq6_inv(fq6_sub(fq6_sqr(a.c0), fq6_mul_v(fq6_sqr(a.c1))));
    return Fq12{fq6_mul(a.c0, t), fq6_neg(fq6_mul(a.c1, t))};
}

// coefficient of w^k over Fq2: w^0 c0.c0, w^1 c1.c0, w^2 c0.c1, w^3 c1.c1, w^4 c0.c2, w^5 c1.c2
VK_HD const Fq2& fq12_coef(const Fq12& a, int k) {
    const Fq6& h = (k & 1) ? a.c1 : a.c0;
    return (k >> 1) == 0 ? h.c0 : (k >> 1) == 1 ? h.c1 : h.c2;
}
VK_HD Fq2& fq12_coef(Fq12& a, int k) {
    Fq6& h = (k & 1) ? a.c1 : a.c0;
    return (k >> 1) == 0 ? h.c0 : (k >> 1) == 1 ? h.c1 : h.c2;
}
VK_HD Fq2 frob_const(int i, int k) {
    Fq2 r;
    const int at = (i - 1) * 12 + 2 * k;
    for (int j = 0; j < NL; j++) {
        r.c0.v[j] = PC::frob(at, j);
        r.c1.v[j] = PC::frob(at + 1, j);
    }
    return r;
}
// a^(p^i), i = 1, 2, 3: coefficient of w^k conjugated i times, times xi^(k (p^i - 1) / 6)
VK_PFN Fq12 fq12_frob(const Fq12& a, int i) {
    Fq12 r;
    for (int k = 0; k < 6; k++) {
        const Fq2& c = fq12_coef(a, k);
        fq12_coef(r, k) = fq2_mul((i & 1) ? fq2_conj(c) : c, frob_const(i, k));
    }
    return r;
}

// ---------------------------------------------------------------- G2 (affine, on the twist)
struct G2Aff {
    Fq2 x, y;
    bool inf;
};
VK_HD Fq2 g2_const(int k) {
    Fq2 r;
    for (int j = 0; j < NL; j++) {
        r.c0.v[j] = PC::g2c(2 * k, j);
        r.c1.v[j] = PC::g2c(2 * k + 1, j);
    }
    return r;
}
VK_HD Fq g1_const(int k) {
    Fq r;
    for (int j = 0; j < NL; j++) r.v[j] = PC::g1c(k, j);
    return r;
}
VK_HD G2Aff g2_generator() { return G2Aff{g2_const(1), g2_const(2), false}; }
VK_HD G2Aff g2_neg(const G2Aff& p) { return G2Aff{p.x, fq2_neg(p.y), p.inf}; }
VK_HD bool g2_on_twist(const G2Aff& p) {
    if (p.inf) return true;
    return fq2_eq(fq2_sqr(p.y), fq2_add(fq2_mul(fq2_sqr(p.x), p.x), g2_const(0)));
}

// a Miller step: slope and lam xT - yT
struct LineCoef {
    Fq2 lam, c;
};
// tangent at T (T != O, yT != 0 for a point of odd order), T <- 2 T
VK_HD LineCoef line_dbl(G2Aff& T) {
    const Fq2 xx = fq2_sqr(T.x);
    LineCoef l;
    l.lam = fq2_mul(fq2_add(fq2_dbl(xx), xx), fq2_inv(fq2_dbl(T.y)));
    l.c = fq2_sub(fq2_mul(l.lam, T.x), T.y);
    const Fq2 x3 = fq2_sub(fq2_sqr(l.lam), fq2_dbl(T.x));
    T.y = fq2_sub(fq2_mul(l.lam, fq2_sub(T.x, x3)), T.y);
    T.x = x3;
    return l;
}
// chord through T and Q (xT != xQ), T <- T + Q
VK_HD LineCoef line_add(G2Aff& T, const G2Aff& Q) {
    LineCoef l;
    l.lam = fq2_mul(fq2_sub(Q.y, T.y), fq2_inv(fq2_sub(Q.x, T.x)));
    l.c = fq2_sub(fq2_mul(l.lam, T.x), T.y);
    const Fq2 x3 = fq2_sub(fq2_sub(fq2_sqr(l.lam), T.x), Q.x);
    T.y = fq2_sub(fq2_mul(l.lam, fq2_sub(T.x, x3)), T.y);
    T.x = x3;
    return l;
}
// general group law (setup-time work: [s] H, the subgroup check)
VK_HD G2Aff g2_add(const G2Aff& a, const G2Aff& b) {
    if (a.inf) return b;
    if (b.inf) return a;
    G2Aff t = a;
    if (fq2_eq(a.x, b.x)) {
        if (!fq2_eq(a.y, b.y) || fq2_is_zero(a.y)) return G2Aff{fq2_zero(), fq2_zero(), true};
        line_dbl(t);
        return t;
    }
    line_add(t, b);
    return t;
}
// k Q for k given as canonical little-endian 32-bit words
VK_HD G2Aff g2_mul(const G2Aff& q, const uint32_t* k, int words) {
    G2Aff r{fq2_zero(), fq2_zero(), true};
    for (int i = words - 1; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            r = g2_add(r, r);
            if ((k[i] >> b) & 1) r = g2_add(r, q);
        }
    return r;
}
// [r] Q == O (the twist has a large cofactor)
VK_HD bool g2_in_subgroup(const G2Aff& q) {
    uint32_t r[8];
    for (int i = 0; i < 8; i++) r[i] = BLS381Fr::p(i);
    return g2_mul(q, r, 8).inf;
}

// ---------------------------------------------------------------- G1 operand of a line
struct G1Eval {
    Fq xp, yp, zp;
    bool skip;  // the identity: e(O, Q) = 1
};
VK_HD G1Eval g1_eval_aff(const Fq& x, const Fq& y, bool inf) { return G1Eval{x, y, fe_one<BLS381Fq>(), inf}; }
VK_HD G1Eval g1_eval_acc(const SWAcc<BLS381Fq>& a) {
    return G1Eval{fq_mul(a.x, a.zzz), fq_mul(a.y, a.zz), fq_mul(a.zz, a.zzz), fe_is_zero<BLS381Fq>(a.zz)};
}

// f (a + b v + yP v w), a = l.c zP, b = -lam xP: the factor is s0 + s1 w with s0 = a + b v and
// s1 = yP v (yP in Fq), so f s = (f0 s0 + v f1 s1) + ((f0 + f1)(s0 + s1) - f0 s0 - f1 s1) w with
// f1 s1 = v (yP f1) and s0 + s1 = a + (b + yP) v
VK_PFN Fq12 fq12_mul_line(const Fq12& f, const LineCoef& l, const G1Eval& P) {
    const Fq2 a = fq2_scale(l.c, P.zp), b = fq2_neg(fq2_scale(l.lam, P.xp));
    const Fq6 t0 = fq6_mul_01(f.c0, a, b);
    const Fq6 t1 = fq6_mul_v(fq6_scale(f.c1, P.yp));
    const Fq6 t2 = fq6_mul_01(fq6_add(f.c0, f.c1), a, Fq2{fq_add(b.c0, P.yp), b.c1});
    return Fq12{fq6_add(t0, fq6_mul_v(t1)), fq6_sub(fq6_sub(t2, t0), t1)};
}
// the same line as a full Fq12 element (tests: the sparse product against the plain one)
VK_HD Fq12 line_as_fq12(const LineCoef& l, const G1Eval& P) {
    Fq12 s{fq6_zero(), fq6_zero()};
    s.c0.c0 = fq2_scale(l.c, P.zp);
    s.c0.c1 = fq2_neg(fq2_scale(l.lam, P.xp));
    s.c1.c1.c0 = P.yp;
    return s;
}

// ---------------------------------------------------------------- Miller loop
// bit b of |x|
VK_HD int ate_bit(int b) { return (int)((PC::X >> b) & 1); }
// the ATE_LINES line coefficients of Q in loop order (Q of order r, not the identity)
VK_HD void ate_line_table(const G2Aff& Q, LineCoef* out) {
    G2Aff T = Q;
    int k = 0;
    for (int b = PC::ATE_BITS - 1; b >= 0; b--) {
        out[k++] = line_dbl(T);
        if (ate_bit(b)) out[k++] = line_add(T, Q);
    }
}
// f_{|x|,Q}(P) conjugated (x < 0), the lines computed on the fly
VK_HD Fq12 miller_loop(const G1Eval& P, const G2Aff& Q) {
    Fq12 f = fq12_one();
    if (P.skip || Q.inf) return f;
    G2Aff T = Q;
    for (int b = PC::ATE_BITS - 1; b >= 0; b--) {
        f = fq12_sqr(f);
        f = fq12_mul_line(f, line_dbl(T), P);
        if (ate_bit(b)) f = fq12_mul_line(f, line_add(T, Q), P);
    }
    return fq12_conj(f);
}
// the product of two Miller loops over precomputed line tables, one shared accumulator: one
// squaring per doubling step, two sparse products per line, one conjugation
VK_HD Fq12 miller_loop_tab2(const G1Eval& P0, const LineCoef* tab0, const G1Eval& P1, const LineCoef* tab1) {
    Fq12 f = fq12_one();
    for (int k = 0; k < PC::ATE_LINES; k++) {
        if (PC::ate_sq(k)) f = fq12_sqr(f);
        for (int j = 0; j < 2; j++) {
            const G1Eval& P = j ? P1 : P0;
            if (!P.skip) f = fq12_mul_line(f, (j ? tab1 : tab0)[k], P);
        }
    }
    return fq12_conj(f);
}

// ---------------------------------------------------------------- final exponentiation
// (a + b s)^2 in Fq2[s]/(s^2 - xi): (a + b)(a + xi b) - ab - xi ab, 2 ab
VK_HD void fq4_sqr(const Fq2& a, const Fq2& b, Fq2& t0, Fq2& t1) {
    const Fq2 ab = fq2_mul(a, b);
    t0 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a, b), fq2_add(fq2_mul_xi(b), a)), ab), fq2_mul_xi(ab));
    t1 = fq2_dbl(ab);
}
// squaring in the cyclotomic subgroup (Granger-Scott): only for a with a^(p^6 + 1) = 1 and
// a^(p^4 - p^2 + 1) = 1, i.e. after the easy part. 6 Fq2 multiplies against fq12_sqr's 12.
VK_PFN Fq12 fq12_cyc_sqr(const Fq12& a) {
    Fq2 t0, t1, t2, t3, t4, t5;
    fq4_sqr(a.c0.c0, a.c1.c1, t0, t1);
    fq4_sqr(a.c1.c0, a.c0.c2, t2, t3);
    fq4_sqr(a.c0.c1, a.c1.c2, t4, t5);
    Fq12 r;
    // 3 t - 2 z for the c0 half, 3 t + 2 z for the c1 half
    r.c0.c0 = fq2_add(fq2_dbl(fq2_sub(t0, a.c0.c0)), t0);
    r.c0.c1 = fq2_add(fq2_dbl(fq2_sub(t2, a.c0.c1)), t2);
    r.c0.c2 = fq2_add(fq2_dbl(fq2_sub(t4, a.c0.c2)), t4);
    const Fq2 t5x = fq2_mul_xi(t5);
    r.c1.c0 = fq2_add(fq2_dbl(fq2_add(t5x, a.c1.c0)), t5x);
    r.c1.c1 = fq2_add(fq2_dbl(fq2_add(t1, a.c1.c1)), t1);
    r.c1.c2 = fq2_add(fq2_dbl(fq2_add(t3, a.c1.c2)), t3);
    return r;
}
// a^|x| by square and multiply over the 64 bits of |x|, a in the cyclotomic subgroup
VK_HD Fq12 fq12_pow_absx(const Fq12& a) {
    Fq12 r = a;
    for (int b = PC::ATE_BITS - 1; b >= 0; b--) {
        r = fq12_cyc_sqr(r);
        if (ate_bit(b)) r = fq12_mul(r, a);
    }
    return r;
}
// a^x: x < 0 and a unitary, so the inverse is the conjugate
VK_HD Fq12 fq12_pow_x(const Fq12& a) { return fq12_conj(fq12_pow_absx(a)); }
// f^((p^12 - 1) / r) up to a power prime to r: the easy part (p^6 - 1)(p^2 + 1), then the hard
// part (x - 1)^2 (x + p)(x^2 + p^2 - 1) + 3 = 3 (p^4 - p^2 + 1) / r by five powers of x (restated
// with integers in tools/gen_pairing_bls.py). After the easy part f is unitary, so inversion is
// conjugation.
VK_HD Fq12 final_exp_easy(const Fq12& f) {
    const Fq12 r = fq12_mul(fq12_conj(f), fq12_inv(f));
    return fq12_mul(fq12_frob(r, 2), r);
}
VK_HD Fq12 final_exp(const Fq12& f) {
    const Fq12 r = final_exp_easy(f);
    Fq12 y = fq12_mul(fq12_pow_x(r), fq12_conj(r));             // r^(x - 1)
    y = fq12_mul(fq12_pow_x(y), fq12_conj(y));                  // ^(x - 1)
    y = fq12_mul(fq12_pow_x(y), fq12_frob(y, 1));               // ^(x + p)
    const Fq12 z = fq12_mul(fq12_frob(y, 2), fq12_conj(y));     // y^(p^2 - 1)
    y = fq12_mul(fq12_pow_x(fq12_pow_x(y)), z);                 // ^(x^2 + p^2 - 1)
    return fq12_mul(y, fq12_mul(fq12_cyc_sqr(r), r));           // r^3
}

// prod e(P_i, Q_i) == 1, lines on the fly
VK_HD bool pairing_product_is_one(int n, const G1Eval* P, const G2Aff* Q) {
    Fq12 f = fq12_one();
    for (int i = 0; i < n; i++) f = fq12_mul(f, miller_loop(P[i], Q[i]));
    return fq12_is_one(final_exp(f));
}

// ---------------------------------------------------------------- the KZG opening check
// e(pi, [s]_2 - p H) == e(C - y G, H)  <=>  e(pi, [s]_2) e(y G - C - p pi, H) == 1: two pairings
// against the key's two fixed G2 points, whose lines are tabulated once (ate_line_table).
using G1A = SWAcc<BLS381Fq>;
using G1P = SWAff<BLS381Fq>;
VK_HD G1A g1_zero() { return G1A{fe_one<BLS381Fq>(), fe_one<BLS381Fq>(), fe_zero<BLS381Fq>(), fe_zero<BLS381Fq>()}; }
// the XYZZ formulas of ec.hpp (dbl-2008-s-1, madd-2008-s) on the out-of-line multiply, one copy each
VK_PFN G1A g1_dbl(const G1A& p) {
    if (fe_is_zero<BLS381Fq>(p.zz)) return p;
    const Fq U = fq_add(p.y, p.y), V = fq_mul(U, U), W = fq_mul(U, V), S = fq_mul(p.x, V);
    const Fq X2 = fq_mul(p.x, p.x), M = fq_add(fq_add(X2, X2), X2);
    G1A r;
    r.x = fq_sub(fq_mul(M, M), fq_add(S, S));
    r.y = fq_sub(fq_mul(M, fq_sub(S, r.x)), fq_mul(W, p.y));
    r.zz = fq_mul(V, p.zz);
    r.zzz = fq_mul(W, p.zzz);
    return r;
}
VK_PFN G1A g1_madd(const G1A& p, const G1P& q, bool neg) {
    const Fq y2 = neg ? fq_neg(q.y) : q.y;
    if (fe_is_zero<BLS381Fq>(p.zz)) return G1A{q.x, y2, fe_one<BLS381Fq>(), fe_one<BLS381Fq>()};
    const Fq P = fq_sub(fq_mul(q.x, p.zz), p.x), R = fq_sub(fq_mul(y2, p.zzz), p.y);
    if (fe_is_zero<BLS381Fq>(P)) {
        if (fe_is_zero<BLS381Fq>(R)) return g1_dbl(G1A{q.x, y2, fe_one<BLS381Fq>(), fe_one<BLS381Fq>()});
        return g1_zero();
    }
    const Fq PP = fq_mul(P, P), PPP = fq_mul(P, PP), Q = fq_mul(p.x, PP);
    G1A r;
    r.x = fq_sub(fq_sub(fq_mul(R, R), PPP), fq_add(Q, Q));
    r.y = fq_sub(fq_mul(R, fq_sub(Q, r.x)), fq_mul(p.y, PPP));
    r.zz = fq_mul(p.zz, PP);
    r.zzz = fq_mul(p.zzz, PPP);
    return r;
}
// canonical little-endian words below the modulus?
template <class F>
VK_HD bool words_below_modulus(const uint32_t* w) {
    for (int i = F::N - 1; i >= 0; i--)
        if (w[i] != F::p(i)) return w[i] < F::p(i);
    return false;
}
// P (on the curve, Montgomery) in the subgroup of order r: phi^2(P) + [z^2] P == O, the test
// k_glv_check runs over whole tables. phi^2 = (beta2 x, y) satisfies X^2 + X + 1 = 0 on all of
// E(Fq), so a point that passes has (z^4 - z^2 + 1) P = r P = O: the test is complete.
VK_HD bool g1_in_subgroup(const G1P& P) {
    G1A acc = g1_zero();
    for (int b = 127; b >= 0; b--) {
        acc = g1_dbl(acc);
        const uint64_t w = b >= 64 ? PC::Z2_HI : PC::Z2_LO;
        if ((w >> (b & 63)) & 1) acc = g1_madd(acc, P, false);
    }
    acc = g1_madd(acc, G1P{fq_mul(P.x, g1_const(2)), P.y}, false);
    return fe_is_zero<BLS381Fq>(acc.zz);
}
// a G1 input (canonical x[12], y[12] words): false when a coordinate is >= p, the point is off
// y^2 = x^3 + 4, or it is outside the subgroup of order r; the Montgomery form in `out`.
VK_HD bool g1_load(const uint32_t* xy, G1P& out) {
    if (!words_below_modulus<BLS381Fq>(xy) || !words_below_modulus<BLS381Fq>(xy + NL)) return false;
    Fq x, y;
    for (int i = 0; i < NL; i++) {
        x.v[i] = xy[i];
        y.v[i] = xy[NL + i];
    }
    out.x = fe_to_mont<BLS381Fq>(x);
    out.y = fe_to_mont<BLS381Fq>(y);
    const Fq one = fe_one<BLS381Fq>();
    const Fq two = fq_add(one, one), four = fq_add(two, two);
    if (!fe_eq<BLS381Fq>(fq_mul(out.y, out.y), fq_add(fq_mul(fq_mul(out.x, out.x), out.x), four))) return false;
#ifdef VK_BLS_NO_SUBGROUP_TEST  // tests only: shows that the subgroup cases need the test
    return true;
#else
    return g1_in_subgroup(out);
#endif
}
VK_PFN FrE fr_mul(const FrE& a, const FrE& b) { return fe_mul<BLS381Fr>(a, b); }
// verify_point's p for a canonical point below r: omega^point when point < size (the strict `<`
// of the reference), else the point itself; canonical words out. omega: the generator of the
// domain of `size` (a power of two), Montgomery: 7^((r - 1) / size), vc_kzg_setup's.
VK_HD void kzg_eval_point(const FrE& omega, uint64_t size, const uint32_t* point, uint32_t* out) {
    uint32_t hi = 0;
    for (int k = 0; k < 8; k++) {
        out[k] = point[k];
        if (k >= 2) hi |= point[k];
    }
    uint64_t e = (uint64_t)point[0] | ((uint64_t)point[1] << 32);
    if (hi || e >= size) return;
    FrE r = fe_one<BLS381Fr>(), b = omega;
    for (; e; e >>= 1) {
        if (e & 1) r = fr_mul(r, b);
        b = fr_mul(b, b);
    }
    r = fe_from_mont<BLS381Fr>(r);
    for (int k = 0; k < 8; k++) out[k] = r.v[k];
}
// one opening: commitment C and proof pi (validated, Montgomery; *_inf: the identity), y and the
// evaluation point p as canonical words below r. A = y G - C - p pi by a joint double-and-add,
// kept in XYZZ and never normalised.
VK_HD bool kzg_check(const G1P& C, bool c_inf, const G1P& pi, bool pi_inf, const uint32_t* y, const uint32_t* p,
                     const LineCoef* tab_s, const LineCoef* tab_h) {
    const G1P G{g1_const(0), g1_const(1)};
    G1A A = g1_zero();
    for (int i = 7; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            A = g1_dbl(A);
            if ((y[i] >> b) & 1) A = g1_madd(A, G, false);
            if (!pi_inf && ((p[i] >> b) & 1)) A = g1_madd(A, pi, true);
        }
    if (!c_inf) A = g1_madd(A, C, true);
    const Fq12 f = miller_loop_tab2(g1_eval_aff(pi.x, pi.y, pi_inf), tab_s, g1_eval_acc(A), tab_h);
    return fq12_is_one(final_exp(f));
}

}  // namespace bls
}  // namespace vk

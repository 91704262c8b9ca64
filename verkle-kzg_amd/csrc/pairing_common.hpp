// What the BN254 and the BLS12-381 pairing have in common, host + gfx950 device from one source,
// as function templates over the base field's tag F: the tower Fq2 / Fq6 / Fq12, the affine G2
// law with its Miller steps, the table-driven Miller loop, the easy part of the final
// exponentiation, the G1 tail (XYZZ double and mixed add on the out-of-line multiply, the input
// checks) and the KZG opening check. pairing.hpp (BN254) and pairing_bls.hpp (BLS12-381) add what
// a curve does differently and name it for this text:
//     fq2_mul_xi                       xi of Fq6 = Fq2[v]/(v^3 - xi)
//     fq12_mul_line, line_as_fq12      the sparse line product: D-type or M-type twist
//     ate_line_table, miller_loop      the Miller schedule
//     final_exp (fq12_pow_x)           the hard part
//     g1_in_subgroup                   curves with a G1 cofactor
// The curve's constants, its G1 generator and its inlining policy are in kzg_curves.hpp.
//
// Field engine: the canonical 32-bit-limb Montgomery form of ff.hpp (fe<F>), not the loosely
// reduced radix-2^29 form of ff29.hpp. Every fe_add / fe_sub / fe_mul result is fully reduced, so
// the tower's long chains of additions and subtractions (Karatsuba at three levels, the sparse
// line products, the Frobenius maps) need no operand-bound bookkeeping, and "f == 1" at the end is
// a limb compare. An Fq12 is 96 words on BN254 and 144 on BLS12-381.
//
// Tower: Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v).
//
// Lines. G2 points are kept affine (they are fixed per key, or host-side inputs), so a Miller step
// is a slope lam (Fq2) on the twist and the constant c = lam xT - yT. A G1 point in XYZZ
// coordinates (x = X / ZZ, y = Y / ZZZ) is used scaled by ZZ ZZZ -- a factor in Fq, which the final
// exponentiation sends to 1: yP' = Y ZZ, xP' = X ZZZ, zP' = ZZ ZZZ. No per-proof inversion. The
// identity (zP' = 0) pairs to one: its lines are skipped.
//
// Code size on the device: every multiply / square of the tower is one out-of-line function
// (VK_PFN), and the Miller loop and the powers of x are rolled loops over tables.
#pragma once
#include "kzg_curves.hpp"

#ifdef __HIP_DEVICE_COMPILE__
#define VK_PFN __host__ __device__ __attribute__((noinline))
#else
#define VK_PFN __host__ __device__ inline
#endif

namespace vk {
namespace ate {

template <class F>
struct Fq2T {
    fe<F> c0, c1;
};
template <class F>
struct Fq6T {
    Fq2T<F> c0, c1, c2;
};
template <class F>
struct Fq12T {
    Fq6T<F> c0, c1;
};

// name(a, b) = the expression: inline, or through one out-of-line copy on a curve with OOL_ADDS
// (the policy and its reason: kzg_curves.hpp)
#define VK_TOWER_SUM(T, name, ...)                                    \
    template <class F>                                                \
    VK_PFN T<F> name##_ool(const T<F>& a, const T<F>& b) {            \
        return __VA_ARGS__;                                           \
    }                                                                 \
    template <class F>                                                \
    VK_HD T<F> name(const T<F>& a, const T<F>& b) {                   \
        if constexpr (KzgCurve<F>::OOL_ADDS) return name##_ool(a, b); \
        else return __VA_ARGS__;                                      \
    }

// ---------------------------------------------------------------- Fq, Fr
template <class F>
VK_PFN fe<F> fq_mul(const fe<F>& a, const fe<F>& b) {
    return fe_mul<F>(a, b);
}
template <class F>
VK_PFN fe<F> fr_mul(const fe<F>& a, const fe<F>& b) {
    return fe_mul<F>(a, b);
}
VK_TOWER_SUM(fe, fq_add, fe_add<F>(a, b))
VK_TOWER_SUM(fe, fq_sub, fe_sub<F>(a, b))
template <class F>
VK_HD fe<F> fq_neg(const fe<F>& a) {
    if constexpr (KzgCurve<F>::OOL_ADDS) return fq_sub(fe_zero<F>(), a);
    else return fe_neg<F>(a);
}
template <class F>
VK_HD fe<F> fq_inv(const fe<F>& a) {
#ifdef __HIP_DEVICE_COMPILE__
    return fe_inv<F>(a);
#else
    return fe_inv_bin<F>(a);
#endif
}
// the small integer K >= 1 by doubling and adding one over K's bits
template <class F, int K>
VK_HD fe<F> fq_small() {
    int top = 30;
    while (!((K >> top) & 1)) top--;
    fe<F> r = fe_one<F>();
    for (int b = top - 1; b >= 0; b--) {
        r = fq_add(r, r);
        if ((K >> b) & 1) r = fq_add(r, fe_one<F>());
    }
    return r;
}

// ---------------------------------------------------------------- Fq2
template <class F>
VK_HD Fq2T<F> fq2_zero() {
    return Fq2T<F>{fe_zero<F>(), fe_zero<F>()};
}
template <class F>
VK_HD Fq2T<F> fq2_one() {
    return Fq2T<F>{fe_one<F>(), fe_zero<F>()};
}
template <class F>
VK_HD bool fq2_is_zero(const Fq2T<F>& a) {
    return fe_is_zero<F>(a.c0) && fe_is_zero<F>(a.c1);
}
template <class F>
VK_HD bool fq2_eq(const Fq2T<F>& a, const Fq2T<F>& b) {
    return fe_eq<F>(a.c0, b.c0) && fe_eq<F>(a.c1, b.c1);
}
VK_TOWER_SUM(Fq2T, fq2_add, Fq2T<F>{fq_add(a.c0, b.c0), fq_add(a.c1, b.c1)})
VK_TOWER_SUM(Fq2T, fq2_sub, Fq2T<F>{fq_sub(a.c0, b.c0), fq_sub(a.c1, b.c1)})
template <class F>
VK_HD Fq2T<F> fq2_dbl(const Fq2T<F>& a) {
    return fq2_add(a, a);
}
template <class F>
VK_HD Fq2T<F> fq2_neg(const Fq2T<F>& a) {
    return Fq2T<F>{fq_neg(a.c0), fq_neg(a.c1)};
}
template <class F>
VK_HD Fq2T<F> fq2_conj(const Fq2T<F>& a) {
    return Fq2T<F>{a.c0, fq_neg(a.c1)};
}
template <class F>
VK_HD Fq2T<F> fq2_scale(const Fq2T<F>& a, const fe<F>& k) {
    return Fq2T<F>{fq_mul(a.c0, k), fq_mul(a.c1, k)};
}
// Karatsuba: 3 Fq multiplies
template <class F>
VK_PFN Fq2T<F> fq2_mul(const Fq2T<F>& a, const Fq2T<F>& b) {
    const fe<F> v0 = fq_mul(a.c0, b.c0), v1 = fq_mul(a.c1, b.c1);
    const fe<F> s = fq_mul(fq_add(a.c0, a.c1), fq_add(b.c0, b.c1));
    return Fq2T<F>{fq_sub(v0, v1), fq_sub(fq_sub(s, v0), v1)};
}
// (a0 + a1)(a0 - a1) + 2 a0 a1 u
template <class F>
VK_PFN Fq2T<F> fq2_sqr(const Fq2T<F>& a) {
    const fe<F> t = fq_mul(a.c0, a.c1);
    return Fq2T<F>{fq_mul(fq_add(a.c0, a.c1), fq_sub(a.c0, a.c1)), fq_add(t, t)};
}
template <class F>
VK_HD Fq2T<F> fq2_inv(const Fq2T<F>& a) {
    const fe<F> n = fq_inv(fq_add(fq_mul(a.c0, a.c0), fq_mul(a.c1, a.c1)));
    return Fq2T<F>{fq_mul(a.c0, n), fq_neg(fq_mul(a.c1, n))};
}

// ---------------------------------------------------------------- Fq6
template <class F>
VK_HD Fq6T<F> fq6_zero() {
    return Fq6T<F>{fq2_zero<F>(), fq2_zero<F>(), fq2_zero<F>()};
}
template <class F>
VK_HD Fq6T<F> fq6_one() {
    return Fq6T<F>{fq2_one<F>(), fq2_zero<F>(), fq2_zero<F>()};
}
VK_TOWER_SUM(Fq6T, fq6_add, Fq6T<F>{fq2_add(a.c0, b.c0), fq2_add(a.c1, b.c1), fq2_add(a.c2, b.c2)})
VK_TOWER_SUM(Fq6T, fq6_sub, Fq6T<F>{fq2_sub(a.c0, b.c0), fq2_sub(a.c1, b.c1), fq2_sub(a.c2, b.c2)})
#undef VK_TOWER_SUM
template <class F>
VK_HD Fq6T<F> fq6_neg(const Fq6T<F>& a) {
    return Fq6T<F>{fq2_neg(a.c0), fq2_neg(a.c1), fq2_neg(a.c2)};
}
// a v: (a0 + a1 v + a2 v^2) v = xi a2 + a0 v + a1 v^2
template <class F>
VK_HD Fq6T<F> fq6_mul_v(const Fq6T<F>& a) {
    return Fq6T<F>{fq2_mul_xi(a.c2), a.c0, a.c1};
}
// Karatsuba: 6 Fq2 multiplies
template <class F>
VK_PFN Fq6T<F> fq6_mul(const Fq6T<F>& a, const Fq6T<F>& b) {
    const Fq2T<F> v0 = fq2_mul(a.c0, b.c0), v1 = fq2_mul(a.c1, b.c1), v2 = fq2_mul(a.c2, b.c2);
    const Fq2T<F> t12 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c1, a.c2), fq2_add(b.c1, b.c2)), v1), v2);
    const Fq2T<F> t01 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c0, a.c1), fq2_add(b.c0, b.c1)), v0), v1);
    const Fq2T<F> t02 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c0, a.c2), fq2_add(b.c0, b.c2)), v0), v2);
    return Fq6T<F>{fq2_add(v0, fq2_mul_xi(t12)), fq2_add(t01, fq2_mul_xi(v2)), fq2_add(t02, v1)};
}
// Chung-Hasan SQR2: 2 multiplies + 3 squares
template <class F>
VK_PFN Fq6T<F> fq6_sqr(const Fq6T<F>& a) {
    const Fq2T<F> s0 = fq2_sqr(a.c0);
    const Fq2T<F> s1 = fq2_dbl(fq2_mul(a.c0, a.c1));
    const Fq2T<F> s2 = fq2_sqr(fq2_add(fq2_sub(a.c0, a.c1), a.c2));
    const Fq2T<F> s3 = fq2_dbl(fq2_mul(a.c1, a.c2));
    const Fq2T<F> s4 = fq2_sqr(a.c2);
    return Fq6T<F>{fq2_add(s0, fq2_mul_xi(s3)), fq2_add(s1, fq2_mul_xi(s4)),
                   fq2_sub(fq2_sub(fq2_add(fq2_add(s1, s2), s3), s0), s4)};
}
// a (b0 + b1 v), the sparse factor of a line product
template <class F>
VK_PFN Fq6T<F> fq6_mul_01(const Fq6T<F>& a, const Fq2T<F>& b0, const Fq2T<F>& b1) {
    const Fq2T<F> a0b0 = fq2_mul(a.c0, b0), a1b1 = fq2_mul(a.c1, b1);
    const Fq2T<F> c1 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c0, a.c1), fq2_add(b0, b1)), a0b0), a1b1);
    return Fq6T<F>{fq2_add(a0b0, fq2_mul_xi(fq2_mul(a.c2, b1))), c1, fq2_add(a1b1, fq2_mul(a.c2, b0))};
}
template <class F>
VK_HD Fq6T<F> fq6_scale(const Fq6T<F>& a, const fe<F>& k) {
    return Fq6T<F>{fq2_scale(a.c0, k), fq2_scale(a.c1, k), fq2_scale(a.c2, k)};
}
template <class F>
VK_HD Fq6T<F> fq6_inv(const Fq6T<F>& a) {
    const Fq2T<F> A = fq2_sub(fq2_sqr(a.c0), fq2_mul_xi(fq2_mul(a.c1, a.c2)));
    const Fq2T<F> B = fq2_sub(fq2_mul_xi(fq2_sqr(a.c2)), fq2_mul(a.c0, a.c1));
    const Fq2T<F> C = fq2_sub(fq2_sqr(a.c1), fq2_mul(a.c0, a.c2));
    const Fq2T<F> D = fq2_add(fq2_mul(a.c0, A), fq2_mul_xi(fq2_add(fq2_mul(a.c2, B), fq2_mul(a.c1, C))));
    const Fq2T<F> Di = fq2_inv(D);
    return Fq6T<F>{fq2_mul(A, Di), fq2_mul(B, Di), fq2_mul(C, Di)};
}

// ---------------------------------------------------------------- Fq12
template <class F>
VK_HD Fq12T<F> fq12_one() {
    return Fq12T<F>{fq6_one<F>(), fq6_zero<F>()};
}
template <class F>
VK_HD Fq12T<F> fq12_conj(const Fq12T<F>& a) {
    return Fq12T<F>{a.c0, fq6_neg(a.c1)};
}
template <class F>
VK_HD bool fq12_eq(const Fq12T<F>& a, const Fq12T<F>& b) {
    return fq2_eq(a.c0.c0, b.c0.c0) && fq2_eq(a.c0.c1, b.c0.c1) && fq2_eq(a.c0.c2, b.c0.c2) &&
           fq2_eq(a.c1.c0, b.c1.c0) && fq2_eq(a.c1.c1, b.c1.c1) && fq2_eq(a.c1.c2, b.c1.c2);
}
// every limb is canonical (ff.hpp), so this is a plain compare with the Montgomery one
template <class F>
VK_HD bool fq12_is_one(const Fq12T<F>& a) {
    return fq12_eq(a, fq12_one<F>());
}
// Karatsuba: 3 Fq6 multiplies
template <class F>
VK_PFN Fq12T<F> fq12_mul(const Fq12T<F>& a, const Fq12T<F>& b) {
    const Fq6T<F> v0 = fq6_mul(a.c0, b.c0), v1 = fq6_mul(a.c1, b.c1);
    const Fq6T<F> s = fq6_mul(fq6_add(a.c0, a.c1), fq6_add(b.c0, b.c1));
    return Fq12T<F>{fq6_add(v0, fq6_mul_v(v1)), fq6_sub(fq6_sub(s, v0), v1)};
}
// complex squaring: 2 Fq6 multiplies
template <class F>
VK_PFN Fq12T<F> fq12_sqr(const Fq12T<F>& a) {
    const Fq6T<F> ab = fq6_mul(a.c0, a.c1);
    const Fq6T<F> t = fq6_mul(fq6_add(a.c0, a.c1), fq6_add(a.c0, fq6_mul_v(a.c1)));
    return Fq12T<F>{fq6_sub(fq6_sub(t, ab), fq6_mul_v(ab)), fq6_add(ab, ab)};
}
template <class F>
VK_PFN Fq12T<F> fq12_inv(const Fq12T<F>& a) {
    const Fq6T<F> t = fq6_inv(fq6_sub(fq6_sqr(a.c0), fq6_mul_v(fq6_sqr(a.c1))));
    return Fq12T<F>{fq6_mul(a.c0, t), fq6_neg(fq6_mul(a.c1, t))};
}

// coefficient of w^k over Fq2: w^0 c0.c0, w^1 c1.c0, w^2 c0.c1, w^3 c1.c1, w^4 c0.c2, w^5 c1.c2
template <class F>
VK_HD const Fq2T<F>& fq12_coef(const Fq12T<F>& a, int k) {
    const Fq6T<F>& h = (k & 1) ? a.c1 : a.c0;
    return (k >> 1) == 0 ? h.c0 : (k >> 1) == 1 ? h.c1 : h.c2;
}
template <class F>
VK_HD Fq2T<F>& fq12_coef(Fq12T<F>& a, int k) {
    Fq6T<F>& h = (k & 1) ? a.c1 : a.c0;
    return (k >> 1) == 0 ? h.c0 : (k >> 1) == 1 ? h.c1 : h.c2;
}
template <class F>
VK_HD Fq2T<F> frob_const(int i, int k) {
    using PC = typename KzgCurve<F>::PC;
    Fq2T<F> r;
    const int at = (i - 1) * 12 + 2 * k;
    for (int j = 0; j < F::N; j++) {
        r.c0.v[j] = PC::frob(at, j);
        r.c1.v[j] = PC::frob(at + 1, j);
    }
    return r;
}
// a^(p^i), i = 1, 2, 3: coefficient of w^k conjugated i times, times xi^(k (p^i - 1) / 6)
template <class F>
VK_PFN Fq12T<F> fq12_frob(const Fq12T<F>& a, int i) {
    Fq12T<F> r;
    for (int k = 0; k < 6; k++) {
        const Fq2T<F>& c = fq12_coef(a, k);
        fq12_coef(r, k) = fq2_mul((i & 1) ? fq2_conj(c) : c, frob_const<F>(i, k));
    }
    return r;
}

// ---------------------------------------------------------------- G2 (affine, on the twist)
template <class F>
struct G2AffT {
    Fq2T<F> x, y;
    bool inf;
};
// constant k of the curve's table: 0 the twist's b, 1 and 2 the generator H
template <class F>
VK_HD Fq2T<F> g2_const(int k) {
    using PC = typename KzgCurve<F>::PC;
    Fq2T<F> r;
    for (int j = 0; j < F::N; j++) {
        r.c0.v[j] = PC::g2c(2 * k, j);
        r.c1.v[j] = PC::g2c(2 * k + 1, j);
    }
    return r;
}
template <class F>
VK_HD G2AffT<F> g2_generator() {
    return G2AffT<F>{g2_const<F>(1), g2_const<F>(2), false};
}
template <class F>
VK_HD G2AffT<F> g2_neg(const G2AffT<F>& p) {
    return G2AffT<F>{p.x, fq2_neg(p.y), p.inf};
}
template <class F>
VK_HD bool g2_on_twist(const G2AffT<F>& p) {
    if (p.inf) return true;
    return fq2_eq(fq2_sqr(p.y), fq2_add(fq2_mul(fq2_sqr(p.x), p.x), g2_const<F>(0)));
}

// a Miller step: slope and lam xT - yT
template <class F>
struct LineCoefT {
    Fq2T<F> lam, c;
};
// tangent at T (T != O, yT != 0 for a point of odd order), T <- 2 T
template <class F>
VK_HD LineCoefT<F> line_dbl(G2AffT<F>& T) {
    const Fq2T<F> xx = fq2_sqr(T.x);
    LineCoefT<F> l;
    l.lam = fq2_mul(fq2_add(fq2_dbl(xx), xx), fq2_inv(fq2_dbl(T.y)));
    l.c = fq2_sub(fq2_mul(l.lam, T.x), T.y);
    const Fq2T<F> x3 = fq2_sub(fq2_sqr(l.lam), fq2_dbl(T.x));
    T.y = fq2_sub(fq2_mul(l.lam, fq2_sub(T.x, x3)), T.y);
    T.x = x3;
    return l;
}
// chord through T and Q (xT != xQ), T <- T + Q
template <class F>
VK_HD LineCoefT<F> line_add(G2AffT<F>& T, const G2AffT<F>& Q) {
    LineCoefT<F> l;
    l.lam = fq2_mul(fq2_sub(Q.y, T.y), fq2_inv(fq2_sub(Q.x, T.x)));
    l.c = fq2_sub(fq2_mul(l.lam, T.x), T.y);
    const Fq2T<F> x3 = fq2_sub(fq2_sub(fq2_sqr(l.lam), T.x), Q.x);
    T.y = fq2_sub(fq2_mul(l.lam, fq2_sub(T.x, x3)), T.y);
    T.x = x3;
    return l;
}
// general group law (setup-time work: [s] H, the subgroup check)
template <class F>
VK_HD G2AffT<F> g2_add(const G2AffT<F>& a, const G2AffT<F>& b) {
    if (a.inf) return b;
    if (b.inf) return a;
    G2AffT<F> t = a;
    if (fq2_eq(a.x, b.x)) {
        if (!fq2_eq(a.y, b.y) || fq2_is_zero(a.y)) return G2AffT<F>{fq2_zero<F>(), fq2_zero<F>(), true};
        line_dbl(t);
        return t;
    }
    line_add(t, b);
    return t;
}
// k Q for k given as canonical little-endian 32-bit words
template <class F>
VK_HD G2AffT<F> g2_mul(const G2AffT<F>& q, const uint32_t* k, int words) {
    G2AffT<F> r{fq2_zero<F>(), fq2_zero<F>(), true};
    for (int i = words - 1; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            r = g2_add(r, r);
            if ((k[i] >> b) & 1) r = g2_add(r, q);
        }
    return r;
}
// [r] Q == O (BLS12-381's twist has a large cofactor)
template <class F>
VK_HD bool g2_in_subgroup(const G2AffT<F>& q) {
    using Fr = typename KzgCurve<F>::Fr;
    uint32_t r[Fr::N];
    for (int i = 0; i < Fr::N; i++) r[i] = Fr::p(i);
    return g2_mul(q, r, Fr::N).inf;
}

// ---------------------------------------------------------------- G1 operand of a line
template <class F>
struct G1EvalT {
    fe<F> xp, yp, zp;
    bool skip;  // the identity: e(O, Q) = 1
};
template <class F>
VK_HD G1EvalT<F> g1_eval_aff(const fe<F>& x, const fe<F>& y, bool inf) {
    return G1EvalT<F>{x, y, fe_one<F>(), inf};
}
template <class F>
VK_HD G1EvalT<F> g1_eval_acc(const SWAcc<F>& a) {
    return G1EvalT<F>{fq_mul(a.x, a.zzz), fq_mul(a.y, a.zz), fq_mul(a.zz, a.zzz), fe_is_zero<F>(a.zz)};
}

// ---------------------------------------------------------------- Miller loop, final exponentiation
// the product of two Miller loops over precomputed line tables (the curve's ate_line_table), one
// shared accumulator: one squaring per doubling step, two sparse products per line, and one
// conjugation where x < 0 (f^-1 up to the easy part)
template <class F>
VK_HD Fq12T<F> miller_loop_tab2(const G1EvalT<F>& P0, const LineCoefT<F>* tab0, const G1EvalT<F>& P1,
                                const LineCoefT<F>* tab1) {
    using C = KzgCurve<F>;
    Fq12T<F> f = fq12_one<F>();
    for (int k = 0; k < C::PC::ATE_LINES; k++) {
        if (C::PC::ate_sq(k)) f = fq12_sqr(f);
        for (int j = 0; j < 2; j++) {
            const G1EvalT<F>& P = j ? P1 : P0;
            if (!P.skip) f = fq12_mul_line(f, (j ? tab1 : tab0)[k], P);
        }
    }
    if constexpr (C::X_NEGATIVE) return fq12_conj(f);
    else return f;
}
// the same for m tables: prod_j of the Miller loops of P[j] over tab[j], one squaring chain for all
// of them, identities skipped (m = 2 is miller_loop_tab2 step for step). The conjugation is a ring
// automorphism, so the products of several calls multiply to the product over all their tables.
template <class F>
VK_HD Fq12T<F> miller_loop_tabn(int m, const G1EvalT<F>* P, const LineCoefT<F>* const* tab) {
    using C = KzgCurve<F>;
    Fq12T<F> f = fq12_one<F>();
    for (int k = 0; k < C::PC::ATE_LINES; k++) {
        if (C::PC::ate_sq(k)) f = fq12_sqr(f);
        for (int j = 0; j < m; j++)
            if (!P[j].skip) f = fq12_mul_line(f, tab[j][k], P[j]);
    }
    if constexpr (C::X_NEGATIVE) return fq12_conj(f);
    else return f;
}
// (a + b s)^2 in Fq2[s]/(s^2 - xi): (a + b)(a + xi b) - ab - xi ab, 2 ab
template <class F>
VK_HD void fq4_sqr(const Fq2T<F>& a, const Fq2T<F>& b, Fq2T<F>& t0, Fq2T<F>& t1) {
    const Fq2T<F> ab = fq2_mul(a, b);
    t0 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a, b), fq2_add(fq2_mul_xi(b), a)), ab), fq2_mul_xi(ab));
    t1 = fq2_dbl(ab);
}
// squaring in the cyclotomic subgroup (Granger-Scott): only for a with a^(p^6 + 1) = 1 and
// a^(p^4 - p^2 + 1) = 1, i.e. after the easy part. 6 Fq2 multiplies against fq12_sqr's 12.
template <class F>
VK_PFN Fq12T<F> fq12_cyc_sqr(const Fq12T<F>& a) {
    Fq2T<F> t0, t1, t2, t3, t4, t5;
    fq4_sqr(a.c0.c0, a.c1.c1, t0, t1);
    fq4_sqr(a.c1.c0, a.c0.c2, t2, t3);
    fq4_sqr(a.c0.c1, a.c1.c2, t4, t5);
    Fq12T<F> r;
    // 3 t - 2 z for the c0 half, 3 t + 2 z for the c1 half
    r.c0.c0 = fq2_add(fq2_dbl(fq2_sub(t0, a.c0.c0)), t0);
    r.c0.c1 = fq2_add(fq2_dbl(fq2_sub(t2, a.c0.c1)), t2);
    r.c0.c2 = fq2_add(fq2_dbl(fq2_sub(t4, a.c0.c2)), t4);
    const Fq2T<F> t5x = fq2_mul_xi(t5);
    r.c1.c0 = fq2_add(fq2_dbl(fq2_add(t5x, a.c1.c0)), t5x);
    r.c1.c1 = fq2_add(fq2_dbl(fq2_add(t1, a.c1.c1)), t1);
    r.c1.c2 = fq2_add(fq2_dbl(fq2_add(t3, a.c1.c2)), t3);
    return r;
}
// the easy part (p^6 - 1)(p^2 + 1) of f^((p^12 - 1) / r); after it f is unitary, so inversion is
// conjugation, and the curve's final_exp goes on with its hard part
template <class F>
VK_HD Fq12T<F> final_exp_easy(const Fq12T<F>& f) {
    const Fq12T<F> r = fq12_mul(fq12_conj(f), fq12_inv(f));
    return fq12_mul(fq12_frob(r, 2), r);
}
// prod e(P_i, Q_i) == 1, lines on the fly (the curve's miller_loop)
template <class F>
VK_HD bool pairing_product_is_one(int n, const G1EvalT<F>* P, const G2AffT<F>* Q) {
    Fq12T<F> f = fq12_one<F>();
    for (int i = 0; i < n; i++) f = fq12_mul(f, miller_loop(P[i], Q[i]));
    return fq12_is_one(final_exp(f));
}

// ---------------------------------------------------------------- G1
// the XYZZ formulas of ec.hpp (dbl-2008-s-1, madd-2008-s) on the out-of-line multiply, one copy each
template <class F>
VK_PFN SWAcc<F> g1_dbl(const SWAcc<F>& p) {
    if (fe_is_zero<F>(p.zz)) return p;
    const fe<F> U = fq_add(p.y, p.y), V = fq_mul(U, U), W = fq_mul(U, V), S = fq_mul(p.x, V);
    const fe<F> X2 = fq_mul(p.x, p.x), M = fq_add(fq_add(X2, X2), X2);
    SWAcc<F> r;
    r.x = fq_sub(fq_mul(M, M), fq_add(S, S));
    r.y = fq_sub(fq_mul(M, fq_sub(S, r.x)), fq_mul(W, p.y));
    r.zz = fq_mul(V, p.zz);
    r.zzz = fq_mul(W, p.zzz);
    return r;
}
template <class F>
VK_PFN SWAcc<F> g1_madd(const SWAcc<F>& p, const SWAff<F>& q, bool neg) {
    const fe<F> y2 = neg ? fq_neg(q.y) : q.y;
    if (fe_is_zero<F>(p.zz)) return SWAcc<F>{q.x, y2, fe_one<F>(), fe_one<F>()};
    const fe<F> P = fq_sub(fq_mul(q.x, p.zz), p.x), R = fq_sub(fq_mul(y2, p.zzz), p.y);
    if (fe_is_zero<F>(P)) {
        if (fe_is_zero<F>(R)) return g1_dbl(SWAcc<F>{q.x, y2, fe_one<F>(), fe_one<F>()});
        return SWAcc<F>{fe_one<F>(), fe_one<F>(), fe_zero<F>(), fe_zero<F>()};
    }
    const fe<F> PP = fq_mul(P, P), PPP = fq_mul(P, PP), Q = fq_mul(p.x, PP);
    SWAcc<F> r;
    r.x = fq_sub(fq_sub(fq_mul(R, R), PPP), fq_add(Q, Q));
    r.y = fq_sub(fq_mul(R, fq_sub(Q, r.x)), fq_mul(p.y, PPP));
    r.zz = fq_mul(p.zz, PP);
    r.zzz = fq_mul(p.zzz, PPP);
    return r;
}
// canonical little-endian words below the modulus of F (a base or a scalar field)?
template <class F>
VK_HD bool words_below_modulus(const uint32_t* w) {
    for (int i = F::N - 1; i >= 0; i--)
        if (w[i] != F::p(i)) return w[i] < F::p(i);
    return false;
}
// P (on the curve, Montgomery) in the subgroup of order r, for a curve with a G1 cofactor
// (pairing_bls.hpp)
template <class F>
VK_HD bool g1_in_subgroup(const SWAff<F>& P);
// a G1 input (canonical x[F::N], y[F::N] words): false when a coordinate is >= p, the point is off
// y^2 = x^3 + b or, on a curve with a cofactor, outside the subgroup of order r (a point of small
// order pairs to one with everything); the Montgomery form in `out`.
template <class F>
VK_HD bool g1_load(const uint32_t* xy, SWAff<F>& out) {
    using C = KzgCurve<F>;
    if (!words_below_modulus<F>(xy) || !words_below_modulus<F>(xy + F::N)) return false;
    fe<F> x, y;
    for (int i = 0; i < F::N; i++) {
        x.v[i] = xy[i];
        y.v[i] = xy[F::N + i];
    }
    out.x = fe_to_mont<F>(x);
    out.y = fe_to_mont<F>(y);
    const fe<F> b = fq_small<F, C::G1::COEFF_B>();
    if (!fe_eq<F>(fq_mul(out.y, out.y), fq_add(fq_mul(fq_mul(out.x, out.x), out.x), b))) return false;
#ifdef VK_BLS_NO_SUBGROUP_TEST  // tests only: shows that the subgroup cases need the test
    return true;
#else
    if constexpr (C::G1_COFACTOR) return g1_in_subgroup(out);
    else return true;
#endif
}

// ---------------------------------------------------------------- the KZG opening check
// e(pi, [s]_2 - p H) == e(C - y G, H)  <=>  e(pi, [s]_2) e(y G - C - p pi, H) == 1: two pairings
// against the key's two fixed G2 points, whose lines are tabulated once (ate_line_table).
//
// verify_point's p (kzg/mod.rs:172-179) for a canonical point below r: omega^point when
// point < size (the strict `<` of the reference), else the point itself; canonical words out.
// omega: the generator of the domain of `size` (a power of two), Montgomery.
template <class Fr>
VK_HD void kzg_eval_point(const fe<Fr>& omega, uint64_t size, const uint32_t* point, uint32_t* out) {
    uint32_t hi = 0;
    for (int k = 0; k < 8; k++) {
        out[k] = point[k];
        if (k >= 2) hi |= point[k];
    }
    uint64_t e = (uint64_t)point[0] | ((uint64_t)point[1] << 32);
    if (hi || e >= size) return;
    fe<Fr> r = fe_one<Fr>(), b = omega;
    for (; e; e >>= 1) {
        if (e & 1) r = fr_mul(r, b);
        b = fr_mul(b, b);
    }
    r = fe_from_mont<Fr>(r);
    for (int k = 0; k < 8; k++) out[k] = r.v[k];
}
// one opening: commitment C and proof pi (validated, Montgomery; *_inf: the identity), y and the
// evaluation point p as canonical words below r. A = y G - C - p pi by a joint double-and-add,
// kept in XYZZ and never normalised.
template <class F>
VK_HD bool kzg_check(const SWAff<F>& C, bool c_inf, const SWAff<F>& pi, bool pi_inf, const uint32_t* y,
                     const uint32_t* p, const LineCoefT<F>* tab_s, const LineCoefT<F>* tab_h) {
    const SWAff<F> G = KzgCurve<F>::g1_generator();
    SWAcc<F> A = KzgCurve<F>::G1::zero();
    for (int i = 7; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            A = g1_dbl(A);
            if ((y[i] >> b) & 1) A = g1_madd(A, G, false);
            if (!pi_inf && ((p[i] >> b) & 1)) A = g1_madd(A, pi, true);
        }
    if (!c_inf) A = g1_madd(A, C, true);
    const Fq12T<F> f = miller_loop_tab2(g1_eval_aff(pi.x, pi.y, pi_inf), tab_s, g1_eval_acc(A), tab_h);
    return fq12_is_one(final_exp(f));
}

}  // namespace ate
}  // namespace vk

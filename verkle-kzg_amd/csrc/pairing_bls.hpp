// BLS12-381 ate pairing: what is this curve's own (constants: pairing_bls_consts.hpp,
// tools/gen_pairing_bls.py). The tower, the G2 law, the table-driven Miller loop, the G1 tail and
// the KZG opening check are pairing_common.hpp's text over fe<BLS381Fq> (twelve limbs;
// fe_mul_asm12 on the device); vk::bls names its types without the tag and adds the pieces below.
//
// Tower: xi = 1 + u. G2 is the M-type twist y^2 = x^3 + 4 xi; (x, y) on it maps to
// (x / w^2, y / w^3) on the curve.
//
// Lines. The untwisted slope is lam / w, and the line through the untwisted T evaluated at a G1
// point (xP, yP) is yP - (lam / w) xP + c / w^3; times w^3 (an element of Fq4, which the final
// exponentiation sends to 1):
//     c + (-lam xP) w^2 + yP w^3  =  (c + (-lam xP) v) + (yP v) w.
// This is where the M-type twist differs from BN254's D-type line yP + b w + c w^3: the Fq
// coefficient sits at w^3 and the two Fq2 coefficients at 1 and w^2. For an XYZZ point scaled by
// ZZ ZZZ the line is c zP' + (-lam xP') w^2 + yP' w^3.
//
// Miller loop: over the 64 bits of |x|, 63 doublings and 5 additions, no Frobenius end lines; x is
// negative, so f is conjugated once after the loop (f^-1 up to the easy part).
//
// G1 has a cofactor: g1_load tests the subgroup (phi^2(P) + [z^2] P = O), since a point of small
// order pairs to one with everything.
#pragma once
#include "pairing_common.hpp"

namespace vk {
namespace bls {

using namespace ate;
using Fq = fe<BLS381Fq>;
using FrE = fe<BLS381Fr>;
using PC = BLS381Pairing;
constexpr int NL = BLS381Fq::N;  // 12
using Fq2 = Fq2T<BLS381Fq>;
using Fq6 = Fq6T<BLS381Fq>;
using Fq12 = Fq12T<BLS381Fq>;
using G2Aff = G2AffT<BLS381Fq>;
using LineCoef = LineCoefT<BLS381Fq>;
using G1Eval = G1EvalT<BLS381Fq>;
using G1A = SWAcc<BLS381Fq>;
using G1P = SWAff<BLS381Fq>;
// the shared constructors that no argument selects, for this curve
VK_HD Fq2 fq2_zero() { return ate::fq2_zero<BLS381Fq>(); }
VK_HD Fq2 fq2_one() { return ate::fq2_one<BLS381Fq>(); }
VK_HD Fq6 fq6_zero() { return ate::fq6_zero<BLS381Fq>(); }
VK_HD Fq6 fq6_one() { return ate::fq6_one<BLS381Fq>(); }
VK_HD Fq12 fq12_one() { return ate::fq12_one<BLS381Fq>(); }
VK_HD G2Aff g2_generator() { return ate::g2_generator<BLS381Fq>(); }
// constant k of G1's table: 0 and 1 the generator, 2 beta2 of phi^2
VK_HD Fq g1_const(int k) {
    Fq r;
    for (int j = 0; j < NL; j++) r.v[j] = PC::g1c(k, j);
    return r;
}

// a (1 + u) = (a0 - a1) + (a0 + a1) u
VK_HD Fq2 fq2_mul_xi(const Fq2& a) { return Fq2{fq_sub(a.c0, a.c1), fq_add(a.c0, a.c1)}; }
}  // namespace bls
namespace ate {
using bls::fq2_mul_xi;  // where pairing_common.hpp's templates look it up; the tower is usable from here on
}
namespace bls {

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

// ---------------------------------------------------------------- final exponentiation
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
VK_HD Fq12 final_exp(const Fq12& f) {
    const Fq12 r = final_exp_easy(f);
    Fq12 y = fq12_mul(fq12_pow_x(r), fq12_conj(r));             // r^(x - 1)
    y = fq12_mul(fq12_pow_x(y), fq12_conj(y));                  // ^(x - 1)
    y = fq12_mul(fq12_pow_x(y), fq12_frob(y, 1));               // ^(x + p)
    const Fq12 z = fq12_mul(fq12_frob(y, 2), fq12_conj(y));     // y^(p^2 - 1)
    y = fq12_mul(fq12_pow_x(fq12_pow_x(y)), z);                 // ^(x^2 + p^2 - 1)
    return fq12_mul(y, fq12_mul(fq12_cyc_sqr(r), r));           // r^3
}

}  // namespace bls
namespace ate {
// the rest of what pairing_common.hpp asks of a curve, where its templates look names up
using bls::ate_line_table;
using bls::final_exp;
using bls::fq12_mul_line;
using bls::miller_loop;

// phi^2(P) + [z^2] P == O, the test k_glv_check runs over whole tables. phi^2 = (beta2 x, y)
// satisfies X^2 + X + 1 = 0 on all of E(Fq), so a point that passes has (z^4 - z^2 + 1) P = r P = O:
// the test is complete.
template <>
VK_HD bool g1_in_subgroup(const bls::G1P& P) {
    bls::G1A acc = BLS381G1::zero();
    for (int b = 127; b >= 0; b--) {
        acc = g1_dbl(acc);
        const uint64_t w = b >= 64 ? bls::PC::Z2_HI : bls::PC::Z2_LO;
        if ((w >> (b & 63)) & 1) acc = g1_madd(acc, P, false);
    }
    acc = g1_madd(acc, bls::G1P{fq_mul(P.x, bls::g1_const(2)), P.y}, false);
    return fe_is_zero<BLS381Fq>(acc.zz);
}
}  // namespace ate
}  // namespace vk

// BN254 optimal-ate pairing: what is this curve's own (constants: pairing_consts.hpp,
// tools/gen_pairing.py). The tower, the G2 law, the table-driven Miller loop, the G1 tail and the
// KZG opening check are pairing_common.hpp's text over fe<BN254Fq>; vk::bn names its types without
// the tag and adds the pieces below.
//
// Tower: xi = 9 + u. G2 is the D-type twist y^2 = x^3 + 3 / xi; (x, y) on it maps to
// (x w^2, y w^3) on the curve.
//
// Lines. The line through the untwisted T with slope lam w evaluated at a G1 point (xP, yP) is
//     yP + (-lam xP) w + c w^3,
// and for an XYZZ point scaled by ZZ ZZZ it is yP' + (-lam xP') w + (c zP') w^3.
//
// Miller loop: over the NAF digits of 6x + 2, then the two Frobenius end lines.
#pragma once
#include "pairing_common.hpp"

namespace vk {
namespace bn {

using namespace ate;
using Fq = fe<BN254Fq>;
using PC = BN254Pairing;
using Fq2 = Fq2T<BN254Fq>;
using Fq6 = Fq6T<BN254Fq>;
using Fq12 = Fq12T<BN254Fq>;
using G2Aff = G2AffT<BN254Fq>;
using LineCoef = LineCoefT<BN254Fq>;
using G1Eval = G1EvalT<BN254Fq>;
using G1A = SWAcc<BN254Fq>;
using G1P = SWAff<BN254Fq>;
// the shared constructors that no argument selects, for this curve
VK_HD Fq2 fq2_zero() { return ate::fq2_zero<BN254Fq>(); }
VK_HD Fq2 fq2_one() { return ate::fq2_one<BN254Fq>(); }
VK_HD Fq6 fq6_zero() { return ate::fq6_zero<BN254Fq>(); }
VK_HD Fq6 fq6_one() { return ate::fq6_one<BN254Fq>(); }
VK_HD Fq12 fq12_one() { return ate::fq12_one<BN254Fq>(); }
VK_HD Fq2 frob_const(int i, int k) { return ate::frob_const<BN254Fq>(i, k); }
VK_HD G2Aff g2_generator() { return ate::g2_generator<BN254Fq>(); }

// a (9 + u) = (9 a0 - a1) + (9 a1 + a0) u
VK_HD Fq2 fq2_mul_xi(const Fq2& a) {
    const Fq2 a8 = fq2_dbl(fq2_dbl(fq2_dbl(a)));
    return Fq2{fq_sub(fq_add(a8.c0, a.c0), a.c1), fq_add(fq_add(a8.c1, a.c1), a.c0)};
}
}  // namespace bn
namespace ate {
using bn::fq2_mul_xi;  // where pairing_common.hpp's templates look it up; the tower is usable from here on
}
namespace bn {

// pi(Q) and -pi^2(Q) on the twist: (conj(x) g12, conj(y) g13) and (x g22, -y g23)
VK_HD G2Aff g2_frob1(const G2Aff& q) {
    return G2Aff{fq2_mul(fq2_conj(q.x), frob_const(1, 2)), fq2_mul(fq2_conj(q.y), frob_const(1, 3)), q.inf};
}
VK_HD G2Aff g2_neg_frob2(const G2Aff& q) {
    return G2Aff{fq2_mul(q.x, frob_const(2, 2)), fq2_neg(fq2_mul(q.y, frob_const(2, 3))), q.inf};
}

// f (yP + b w + c w^3), b = -lam xP, c = l.c zP: the factor is s0 + s1 w with s0 = yP in Fq and
// s1 = b + c v, so f s = (f0 s0 + v f1 s1) + ((f0 + f1)(s0 + s1) - f0 s0 - f1 s1) w
VK_PFN Fq12 fq12_mul_line(const Fq12& f, const LineCoef& l, const G1Eval& P) {
    const Fq2 b = fq2_neg(fq2_scale(l.lam, P.xp)), c = fq2_scale(l.c, P.zp);
    const Fq6 t0 = fq6_scale(f.c0, P.yp);
    const Fq6 t1 = fq6_mul_01(f.c1, b, c);
    const Fq6 t2 = fq6_mul_01(fq6_add(f.c0, f.c1), Fq2{fq_add(b.c0, P.yp), b.c1}, c);
    return Fq12{fq6_add(t0, fq6_mul_v(t1)), fq6_sub(fq6_sub(t2, t0), t1)};
}
// the same line as a full Fq12 element (tests: the sparse product against the plain one)
VK_HD Fq12 line_as_fq12(const LineCoef& l, const G1Eval& P) {
    Fq12 s{fq6_zero(), fq6_zero()};
    s.c0.c0.c0 = P.yp;
    s.c1.c0 = fq2_neg(fq2_scale(l.lam, P.xp));
    s.c1.c1 = fq2_scale(l.c, P.zp);
    return s;
}

// ---------------------------------------------------------------- Miller loop
// the ATE_LINES line coefficients of Q in loop order (Q of order r, not the identity)
VK_HD void ate_line_table(const G2Aff& Q, LineCoef* out) {
    G2Aff T = Q;
    const G2Aff nQ = g2_neg(Q);
    int k = 0;
    for (int i = 0; i < PC::ATE_DIGITS; i++) {
        out[k++] = line_dbl(T);
        const int d = PC::ate_naf(i);
        if (d) out[k++] = line_add(T, d > 0 ? Q : nQ);
    }
    out[k++] = line_add(T, g2_frob1(Q));
    out[k++] = line_add(T, g2_neg_frob2(Q));
}
// f_{6x+2,Q}(P) l_{T,pi(Q)}(P) l_{T+pi(Q),-pi^2(Q)}(P) with the lines computed on the fly
VK_HD Fq12 miller_loop(const G1Eval& P, const G2Aff& Q) {
    Fq12 f = fq12_one();
    if (P.skip || Q.inf) return f;
    G2Aff T = Q;
    const G2Aff nQ = g2_neg(Q);
    for (int i = 0; i < PC::ATE_DIGITS; i++) {
        f = fq12_sqr(f);
        f = fq12_mul_line(f, line_dbl(T), P);
        const int d = PC::ate_naf(i);
        if (d) f = fq12_mul_line(f, line_add(T, d > 0 ? Q : nQ), P);
    }
    f = fq12_mul_line(f, line_add(T, g2_frob1(Q)), P);
    return fq12_mul_line(f, line_add(T, g2_neg_frob2(Q)), P);
}

// ---------------------------------------------------------------- final exponentiation
// a^x by square and multiply over the 63 bits of x, a in the cyclotomic subgroup
VK_HD Fq12 fq12_pow_x(const Fq12& a) {
    Fq12 r = a;
    for (int b = 61; b >= 0; b--) {
        r = fq12_cyc_sqr(r);
        if ((PC::X >> b) & 1) r = fq12_mul(r, a);
    }
    return r;
}
// f^((p^12 - 1) / r) up to a power prime to r: the easy part (p^6 - 1)(p^2 + 1), then the hard
// part by three powers of x (Fuentes-Castaneda et al.; the exponent is restated with integers in
// tools/gen_pairing.py). After the easy part f is unitary, so inversion is conjugation.
VK_HD Fq12 final_exp(const Fq12& f) {
    const Fq12 r = final_exp_easy(f);
    const Fq12 y0 = fq12_conj(fq12_pow_x(r));  // r^-x
    const Fq12 y1 = fq12_cyc_sqr(y0);
    const Fq12 y3 = fq12_mul(fq12_cyc_sqr(y1), y1);
    const Fq12 y4 = fq12_conj(fq12_pow_x(y3));
    const Fq12 y6 = fq12_conj(fq12_pow_x(fq12_cyc_sqr(y4)));
    const Fq12 y8 = fq12_mul(fq12_mul(fq12_conj(y6), y4), fq12_conj(y3));
    const Fq12 y9 = fq12_mul(y8, y1);
    const Fq12 y11 = fq12_mul(fq12_mul(y8, y4), r);
    const Fq12 y13 = fq12_mul(fq12_frob(y9, 1), y11);
    const Fq12 y14 = fq12_mul(fq12_frob(y8, 2), y13);
    const Fq12 y15 = fq12_frob(fq12_mul(fq12_conj(r), y9), 3);
    return fq12_mul(y15, y14);
}

}  // namespace bn
namespace ate {
// the rest of what pairing_common.hpp asks of a curve, where its templates look names up
using bn::ate_line_table;
using bn::final_exp;
using bn::fq12_mul_line;
using bn::miller_loop;
}  // namespace ate
}  // namespace vk

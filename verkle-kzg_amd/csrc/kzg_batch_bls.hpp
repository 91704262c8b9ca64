// Per-entry arithmetic of KZG batch verification on BLS12-381 (vc_kzg_verify_batch with a
// BLS12-381 key), host + gfx950 device from one source: k_kzg_bls_batch_prep (kzg_batch_bls.hip)
// wraps entry_check / entry_scalars, and the host path of vc_kzg_batch_fold runs fold_range over
// the host pool. The fold is kzg_batch.hpp's, over this curve's fields:
//   P1 = sum_i rho^i pi_i
//   P2 = (sum_i rho^i y_i) G - sum_i rho^i C_i - sum_i (rho^i p_i) pi_i
//   accept  <=>  e(P1, [s]_2) e(P2, H) == 1
// with p_i = omega^{z_i} for z_i < size and z_i itself otherwise. Malformed includes a point of
// E(Fq) outside the subgroup of order r (pairing_bls.hpp's g1_load).
#pragma once
#include "pairing_bls.hpp"

namespace vk {
namespace kzgb_bls {

using FrE = bls::FrE;
using G1A = bls::G1A;
using G1P = bls::G1P;
constexpr int NL = bls::NL;

VK_HD FrE fr_words(const uint32_t* w) {  // 8 words as they are (no conversion)
    FrE r;
    for (int i = 0; i < 8; i++) r.v[i] = w[i];
    return r;
}

// rho^e by square-and-multiply on the index (Montgomery in and out)
VK_HD FrE pow_index(const FrE& rho, uint64_t e) {
    FrE acc = fe_one<BLS381Fr>(), b = rho;
    while (e) {
        if (e & 1) acc = bls::fr_mul(acc, b);
        e >>= 1;
        if (e) b = bls::fr_mul(b, b);
    }
    return acc;
}

// One entry's validation, vc_kzg_verify_many's sense of malformed: y or point >= r, a coordinate of
// C or pi >= p, such a point off the curve or outside the subgroup (the identity flag is a valid
// input; its coordinates are not read). C and pi come back in Montgomery form, zero for the identity.
VK_HD bool entry_check(const uint32_t* com_xy, bool c_inf, const uint32_t* proof_xy, bool pi_inf, const uint32_t* y,
                       const uint32_t* point, G1P& C, G1P& pi) {
    C = G1P{fe_zero<BLS381Fq>(), fe_zero<BLS381Fq>()};
    pi = C;
    if (!bls::words_below_modulus<BLS381Fr>(y) || !bls::words_below_modulus<BLS381Fr>(point)) return false;
    if (!c_inf && !bls::g1_load(com_xy, C)) return false;
    if (!pi_inf && !bls::g1_load(proof_xy, pi)) return false;
    return true;
}

// the scalars of entry i given w = rho^i: w p_i and w y_i (all Montgomery); y and point canonical
// words below r
VK_HD void entry_scalars(const FrE& w, const FrE& omega, uint64_t size, const uint32_t* y, const uint32_t* point,
                         FrE& wp, FrE& wy) {
    uint32_t pw[8];
    bls::kzg_eval_point(omega, size, point, pw);
    wp = bls::fr_mul(w, fe_to_mont<BLS381Fr>(fr_words(pw)));
    wy = bls::fr_mul(w, fe_to_mont<BLS381Fr>(fr_words(y)));
}

// k P for a Montgomery scalar, plain double-and-add (the host path and (sum rho^i y_i) G)
VK_HD G1A scalar_mul(const G1P& P, const FrE& k_mont) {
    const FrE k = fe_from_mont<BLS381Fr>(k_mont);
    G1A r = BLS381G1::zero();
    for (int b = BLS381Fr::BITS - 1; b >= 0; b--) {
        r = bls::g1_dbl(r);
        if ((k.v[b >> 5] >> (b & 31)) & 1u) r = bls::g1_madd(r, P, false);
    }
    return r;
}

// the three sums of a range of entries
struct Sums {
    G1A p1;   // sum rho^i pi_i
    G1A var;  // sum rho^i C_i + (rho^i p_i) pi_i
    FrE sy;   // sum rho^i y_i (Montgomery)
};
VK_HD Sums sums_zero() { return Sums{BLS381G1::zero(), BLS381G1::zero(), fe_zero<BLS381Fr>()}; }
VK_HD Sums sums_add(const Sums& a, const Sums& b) {
    return Sums{BLS381G1::add(a.p1, b.p1), BLS381G1::add(a.var, b.var), fe_add<BLS381Fr>(a.sy, b.sy)};
}

// entries [lo, hi) of the ABI's arrays (as 32-bit words: com_xy / proof_xy 24 per entry, points / y
// 8 per entry); false when one of them is malformed (out unspecified)
VK_HD bool fold_range(size_t lo, size_t hi, const uint32_t* com_xy, const uint8_t* com_inf, const uint32_t* points,
                      const uint32_t* proof_xy, const uint8_t* proof_inf, const uint32_t* y, const FrE& rho,
                      const FrE& omega, uint64_t size, Sums& out) {
    out = sums_zero();
    FrE w = pow_index(rho, lo);
    for (size_t i = lo; i < hi; i++) {
        G1P C, pi;
        const bool c_inf = com_inf[i] != 0, pi_inf = proof_inf[i] != 0;
        if (!entry_check(com_xy + 2 * NL * i, c_inf, proof_xy + 2 * NL * i, pi_inf, y + 8 * i, points + 8 * i, C, pi))
            return false;
        FrE wp, wy;
        entry_scalars(w, omega, size, y + 8 * i, points + 8 * i, wp, wy);
        if (!c_inf) out.var = BLS381G1::add(out.var, scalar_mul(C, w));
        if (!pi_inf) {
            out.var = BLS381G1::add(out.var, scalar_mul(pi, wp));
            out.p1 = BLS381G1::add(out.p1, scalar_mul(pi, w));
        }
        out.sy = fe_add<BLS381Fr>(out.sy, wy);
        w = bls::fr_mul(w, rho);
    }
    return true;
}

// P1 and P2 of the whole batch from its sums: P2 = sy G - var
VK_HD void fold_finish(const Sums& s, G1A& P1, G1A& P2) {
    const G1P G{bls::g1_const(0), bls::g1_const(1)};
    P1 = s.p1;
    P2 = BLS381G1::add(scalar_mul(G, s.sy), BLS381G1::neg(s.var));
}

// e(P1, [s]_2) e(P2, H) == 1 over the key's line tables; either point may be the identity
VK_HD bool pair_check(const G1A& P1, const G1A& P2, const bls::LineCoef* tab_s, const bls::LineCoef* tab_h) {
    const bls::Fq12 f = bls::miller_loop_tab2(bls::g1_eval_acc(P1), tab_s, bls::g1_eval_acc(P2), tab_h);
    return bls::fq12_is_one(bls::final_exp(f));
}

}  // namespace kzgb_bls
}  // namespace vk

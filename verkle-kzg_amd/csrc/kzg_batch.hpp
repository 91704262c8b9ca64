// Per-entry arithmetic of KZG batch verification (vc_kzg_verify_batch), host + gfx950 device from
// one source and one text for both curves (C: a curve of kzg_curves.hpp): k_kzg_batch_prep
// (kzg_batch.hip) wraps entry_check / entry_scalars, the host path of vc_kzg_batch_fold runs
// fold_range over the host pool, and tests/cpp/kzg_batch_check.cpp runs the same text under the
// sanitizers.
//
// n openings (C_i, z_i, pi_i, y_i) fold with the weights rho^i into one two-pairing check:
//   P1 = sum_i rho^i pi_i
//   P2 = (sum_i rho^i y_i) G - sum_i rho^i C_i - sum_i (rho^i p_i) pi_i
//   accept  <=>  e(P1, [s]_2) e(P2, H) == 1
// with p_i = omega^{z_i} for z_i < size and z_i itself otherwise (kzg_eval_point). An entry gives
// three scalars: rho^i (over C_i and, for P1, over pi_i), rho^i p_i (over pi_i) and rho^i y_i
// (summed in Fr). The rows are positive: the variable sum is subtracted once, as a point.
#pragma once
#include "pairing.hpp"
#include "pairing_bls.hpp"

namespace vk {
namespace kzgb {

template <class C>
using FrOf = fe<typename C::Fr>;
template <class C>
using G1AOf = SWAcc<typename C::Fq>;
template <class C>
using G1POf = SWAff<typename C::Fq>;

template <class Fr>
VK_HD fe<Fr> fr_words(const uint32_t* w) {  // 8 words as they are (no conversion)
    fe<Fr> r;
    for (int i = 0; i < 8; i++) r.v[i] = w[i];
    return r;
}

// rho^e by square-and-multiply on the index (Montgomery in and out)
template <class Fr>
VK_HD fe<Fr> pow_index(const fe<Fr>& rho, uint64_t e) {
    fe<Fr> acc = fe_one<Fr>(), b = rho;
    while (e) {
        if (e & 1) acc = ate::fr_mul(acc, b);
        e >>= 1;
        if (e) b = ate::fr_mul(b, b);
    }
    return acc;
}

// One entry's validation, vc_kzg_verify_many's sense of malformed: y or point >= r, a coordinate of
// C or pi >= p, such a point off the curve or (BLS12-381) outside the subgroup of order r: g1_load
// (the identity flag is a valid input; its coordinates are not read). C and pi come back in
// Montgomery form, zero for the identity.
template <class C>
VK_HD bool entry_check(const uint32_t* com_xy, bool c_inf, const uint32_t* proof_xy, bool pi_inf, const uint32_t* y,
                       const uint32_t* point, G1POf<C>& Cm, G1POf<C>& pi) {
    Cm = G1POf<C>{fe_zero<typename C::Fq>(), fe_zero<typename C::Fq>()};
    pi = Cm;
    if (!ate::words_below_modulus<typename C::Fr>(y) || !ate::words_below_modulus<typename C::Fr>(point))
        return false;
    if (!c_inf && !ate::g1_load(com_xy, Cm)) return false;
    if (!pi_inf && !ate::g1_load(proof_xy, pi)) return false;
    return true;
}

// the scalars of entry i given w = rho^i: w p_i and w y_i (all Montgomery); y and point canonical
// words below r
template <class Fr>
VK_HD void entry_scalars(const fe<Fr>& w, const fe<Fr>& omega, uint64_t size, const uint32_t* y,
                         const uint32_t* point, fe<Fr>& wp, fe<Fr>& wy) {
    uint32_t pw[8];
    ate::kzg_eval_point(omega, size, point, pw);
    wp = ate::fr_mul(w, fe_to_mont<Fr>(fr_words<Fr>(pw)));
    wy = ate::fr_mul(w, fe_to_mont<Fr>(fr_words<Fr>(y)));
}

// k P for a Montgomery scalar, plain double-and-add (the host path and (sum rho^i y_i) G)
template <class C>
VK_HD G1AOf<C> scalar_mul(const G1POf<C>& P, const FrOf<C>& k_mont) {
    using Fr = typename C::Fr;
    const fe<Fr> k = fe_from_mont<Fr>(k_mont);
    G1AOf<C> r = C::G1::zero();
    for (int b = Fr::BITS - 1; b >= 0; b--) {
        r = ate::g1_dbl(r);
        if ((k.v[b >> 5] >> (b & 31)) & 1u) r = ate::g1_madd(r, P, false);
    }
    return r;
}

// the three sums of a range of entries
template <class C>
struct Sums {
    G1AOf<C> p1;   // sum rho^i pi_i
    G1AOf<C> var;  // sum rho^i C_i + (rho^i p_i) pi_i
    FrOf<C> sy;    // sum rho^i y_i (Montgomery)
};
template <class C>
VK_HD Sums<C> sums_zero() {
    return Sums<C>{C::G1::zero(), C::G1::zero(), fe_zero<typename C::Fr>()};
}
template <class C>
VK_HD Sums<C> sums_add(const Sums<C>& a, const Sums<C>& b) {
    return Sums<C>{C::G1::add(a.p1, b.p1), C::G1::add(a.var, b.var), fe_add<typename C::Fr>(a.sy, b.sy)};
}

// entries [lo, hi) of the ABI's arrays (as 32-bit words: com_xy / proof_xy C::PW per entry, points
// / y 8 per entry); false when one of them is malformed (out unspecified)
template <class C>
VK_HD bool fold_range(size_t lo, size_t hi, const uint32_t* com_xy, const uint8_t* com_inf, const uint32_t* points,
                      const uint32_t* proof_xy, const uint8_t* proof_inf, const uint32_t* y, const FrOf<C>& rho,
                      const FrOf<C>& omega, uint64_t size, Sums<C>& out) {
    using G1 = typename C::G1;
    out = sums_zero<C>();
    FrOf<C> w = pow_index(rho, lo);
    for (size_t i = lo; i < hi; i++) {
        G1POf<C> Cm, pi;
        const bool c_inf = com_inf[i] != 0, pi_inf = proof_inf[i] != 0;
        if (!entry_check<C>(com_xy + C::PW * i, c_inf, proof_xy + C::PW * i, pi_inf, y + 8 * i, points + 8 * i, Cm, pi))
            return false;
        FrOf<C> wp, wy;
        entry_scalars(w, omega, size, y + 8 * i, points + 8 * i, wp, wy);
        if (!c_inf) out.var = G1::add(out.var, scalar_mul<C>(Cm, w));
        if (!pi_inf) {
            out.var = G1::add(out.var, scalar_mul<C>(pi, wp));
            out.p1 = G1::add(out.p1, scalar_mul<C>(pi, w));
        }
        out.sy = fe_add<typename C::Fr>(out.sy, wy);
        w = ate::fr_mul(w, rho);
    }
    return true;
}

// P1 and P2 of the whole batch from its sums: P2 = sy G - var
template <class C>
VK_HD void fold_finish(const Sums<C>& s, G1AOf<C>& P1, G1AOf<C>& P2) {
    P1 = s.p1;
    P2 = C::G1::add(scalar_mul<C>(C::g1_generator(), s.sy), C::G1::neg(s.var));
}

// e(P1, [s]_2) e(P2, H) == 1 over the key's line tables; either point may be the identity
template <class F>
VK_HD bool pair_check(const SWAcc<F>& P1, const SWAcc<F>& P2, const ate::LineCoefT<F>* tab_s,
                      const ate::LineCoefT<F>* tab_h) {
    return ate::fq12_is_one(ate::final_exp(
        ate::miller_loop_tab2(ate::g1_eval_acc(P1), tab_s, ate::g1_eval_acc(P2), tab_h)));
}

}  // namespace kzgb
}  // namespace vk

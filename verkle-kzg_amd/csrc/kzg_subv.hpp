// Per-proof arithmetic of KZG subvector batch verification (vc_kzg_verify_subvector_batch), host +
// gfx950 device from one source and one text for both curves (C: a curve of kzg_curves.hpp):
// k_kzg_subv_fold (kzg_subv.hip) wraps the lane functions below with the cross-lane steps (the
// same-wave fence, xor shuffles), the host path of vc_kzg_subvector_batch_fold runs coeffs_serial
// over the host pool, and tests/cpp/kzg_subv_check.cpp runs both on the host under the sanitizers,
// a wave as 64 lanes in a loop.
//
// Proof j is (C_j, S_j, y_j, pi_j), k_j = |S_j|, Z_j = prod_{i in S_j} (X - w^i) = sum_t z_{j,t} X^t,
// I_j = sum_i y_i c_i Z_j / (X - w^i) = sum_t a_{j,t} X^t, valid when
//   e(pi_j, [Z_j(s)]_2) e([I_j(s)]_1 - C_j, H) == 1.
// With the weights rho^j the coefficients move onto the G1 side (z_{j,t} = 0 above k_j):
//   P_t = sum_j rho^j z_{j,t} pi_j   (t = 0 .. Kmax),   a_t = sum_j rho^j a_{j,t}   (t < Kmax)
//   P_H = P_0 + sum_t a_t [s^t]_1 - sum_j rho^j C_j
//   accept  <=>  e(P_H, H) prod_{t = 1 .. Kmax} e(P_t, [s^t]_2) == 1,
// every G2 point a point of the key. Per proof this text makes z_{j,.} and rho^j a_{j,.}:
//   weights   x_i = w^i and u_i = rho^j y_i c_i, c_i = cw_i w^i from kzg_sub.hpp's tables (no
//             inversion) or, on the host path, from one inversion (weights_inv);
//   Z         z <- z (X - x_i), i = 0 .. k - 1; z is monic, so its k low coefficients are kept and
//             the leading one is implied. Step i makes z_t = z_{t-1} - x_i z_t for t <= i, every t
//             from the old row: lanes over t, 64 at a time from the top, each reading its
//             neighbour's z_{t-1} before anyone writes;
//   division  b^(i) = Z / (X - x_i) by synthetic division, b_{k-1} = 1, b_{t-1} = z_t + x_i b_t:
//             lanes over i in lockstep over t = k - 1 .. 0, a_t += sum_i u_i b^(i)_t (a wave sum
//             per t). Sets above 64 indices take ceil(k / 64) such passes.
#pragma once
#include "kzg_batch.hpp"
#include "kzg_sub.hpp"

namespace vk {
namespace kzgv {

using kzgb::fr_words;
using kzgb::FrOf;
using kzgb::G1AOf;
using kzgb::G1POf;

// One entry's validation, vc_kzg_verify_subvector's sense of malformed: a y >= r, a coordinate of C
// or pi >= p, such a point off the curve or (BLS12-381) outside the subgroup of order r (kzgb::
// entry_check's pieces; the identity flag is a valid input whose coordinates are not read). C and pi
// come back in Montgomery form, zero for the identity. y: k values of 8 canonical words.
template <class C>
VK_HD bool entry_check(const uint32_t* com_xy, bool c_inf, const uint32_t* proof_xy, bool pi_inf, const uint32_t* y,
                       uint32_t k, G1POf<C>& Cm, G1POf<C>& pi) {
    Cm = G1POf<C>{fe_zero<typename C::Fq>(), fe_zero<typename C::Fq>()};
    pi = Cm;
    for (uint32_t t = 0; t < k; t++)
        if (!ate::words_below_modulus<typename C::Fr>(y + 8 * (size_t)t)) return false;
    if (!c_inf && !ate::g1_load(com_xy, Cm)) return false;
    if (!pi_inf && !ate::g1_load(proof_xy, pi)) return false;
    return true;
}

// the set's t-th index: x = w^i and u = wgt y c_i, from the tables (y: 8 canonical words below r)
template <class F>
VK_HD void lane_weight(const uint32_t* S, uint32_t k, const fe<F>* pw, const fe<F>* inv1, uint32_t N, uint32_t t,
                       const fe<F>& wsum, const uint32_t* y, const fe<F>& wgt, fe<F>& x, fe<F>& u) {
    const fe<F> cw = kzgs::sub_weight<F>(S, k, inv1, N, t, wsum);
    x = pw[S[t]];
    u = fe_mul<F>(wgt, fe_mul<F>(fe_to_mont<F>(fr_words<F>(y)), kzgs::sub_weight_full<F>(cw, pw, S[t])));
}
// step i of the Z recurrence at t <= i: the new z_t from the old row (z: the low coefficients, the
// leading one of the degree-i polynomial implied)
template <class F>
VK_HD fe<F> z_step(const fe<F>* z, uint32_t i, uint32_t t, const fe<F>& x) {
    const fe<F> zt = t == i ? fe_one<F>() : z[t];
    const fe<F> zl = t ? z[t - 1] : fe_zero<F>();
    return fe_sub<F>(zl, fe_mul<F>(x, zt));
}
// the division's step: the coefficient b_t of Z / (X - x) from b_{t+1} (k: the degree of Z;
// b_{k-1} = 1 whatever comes in)
template <class F>
VK_HD fe<F> div_step(const fe<F>* z, uint32_t k, uint32_t t, const fe<F>& x, const fe<F>& b_above) {
    if (t + 1 == k) return fe_one<F>();
    return fe_add<F>(z[t + 1], fe_mul<F>(x, b_above));
}
// the scalar of row t of a proof with weight wgt: wgt z_t, zero above the degree
template <class F>
VK_HD fe<F> row_scalar(const fe<F>* z, uint32_t k, uint32_t t, const fe<F>& wgt) {
    if (t < k) return fe_mul<F>(wgt, z[t]);
    return t == k ? wgt : fe_zero<F>();
}

// One proof, one thread: z[0 .. k) and a[0 .. k) += wgt a_{j,.} from x_i and c_i (Montgomery), the
// single verifier's order of operations with the steps above. b: k values of scratch.
template <class F>
VK_HD void coeffs_serial(const fe<F>* x, const fe<F>* c, const uint32_t* y, uint32_t k, const fe<F>& wgt, fe<F>* z,
                         fe<F>* b, fe<F>* a) {
    for (uint32_t i = 0; i < k; i++)
        for (uint32_t t = i + 1; t-- > 0;) z[t] = z_step<F>(z, i, t, x[i]);  // from the top: z[t - 1] is still old
    for (uint32_t i = 0; i < k; i++) {
        const fe<F> u = fe_mul<F>(wgt, fe_mul<F>(fe_to_mont<F>(fr_words<F>(y + 8 * (size_t)i)), c[i]));
        for (uint32_t t = k; t-- > 0;) {
            b[t] = div_step<F>(z, k, t, x[i], t + 1 < k ? b[t + 1] : fe_zero<F>());
            a[t] = fe_add<F>(a[t], fe_mul<F>(u, b[t]));
        }
    }
}

}  // namespace kzgv
}  // namespace vk

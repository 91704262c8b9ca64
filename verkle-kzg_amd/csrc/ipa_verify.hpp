// Per-proof arithmetic of batched IPA verification (vc_ipa_verify_many), host + gfx950 device from
// one source: the kernels of ipa_verify.hip are thin wrappers over it, and tests/cpp/
// ipa_verify_check.cpp runs the same text on the host.
//
// low_level_verify_ipa (ipa/mod.rs:321-360) as one identity, the one ipa_verify_impl (ipa.hip)
// checks: with challenges w and x_0..x_{K-1}, s = points_coeffs, b = the barycentric weights of
// the point and P_k = prod_{j>k} x_j,
//   (prod x) C + sum_k (P_k L_k + P_k x_k^2 R_k) + sum_i (-tip s_i) g_i
//       + ((prod x) w y - w tip <b, s>) q == identity.
// The field phase builds the N + 1 scalars over (g, q) (the fixed row, Montgomery) and the 1 + 2K
// scalars over (C, L_k, R_k) (canonical words); the curve phase sums the latter's terms and adds the
// fixed row's commitment.
//
// <b, s> outside the domain is t sum_i s_i w^i / (z - w^i), t = (z^N - 1) / N. The sum is carried as
// one fraction: (A / B) + (n / d) = (A d + n B) / (B d), three multiplies per term and nothing
// stored per term, fractions of different lanes added the same way -- Montgomery's trick with the
// numerators folded in, since only the sum is wanted and never the N inverses themselves. The last
// step, the one inversion of the final denominator B, is not taken either: B is a product of
// non-zero z - w^i, the group has prime order, so the identity holds exactly when it holds with
// every scalar multiplied by B, and B <b, s> = t A needs no division. (A lone lane's Fermat
// inversion, ~380 multiplies in series, cost more than the rest of the field phase together.)
#pragma once
#include "pairing.hpp"  // the input checks: ate::words_below_modulus, ate::g1_load (also reachable as bn::)

namespace vk {
namespace ipav {

// The group law and the multiplies are the engine's inlined ones (ec.hpp BN254G1, ff.hpp): the
// kernels here hold one accumulator and one point, so unlike the pairing tower (pairing_common.hpp's
// out-of-line multiplies) they need no calls, and their operands stay in registers.
using G1A = BN254G1::Acc;
using G1P = BN254G1::Aff;
using FrE = fe<BN254Fr>;
VK_HD FrE fr_mul(const FrE& a, const FrE& b) { return fe_mul<BN254Fr>(a, b); }

template <class F>
VK_HD fe<F> words_load(const uint32_t* w) {  // 8 words as they are (no conversion)
    fe<F> r;
    for (int i = 0; i < 8; i++) r.v[i] = w[i];
    return r;
}
VK_HD FrE fr_load(const uint32_t* w) { return words_load<BN254Fr>(w); }
VK_HD void fr_store(const FrE& a, uint32_t* w) {
    for (int i = 0; i < 8; i++) w[i] = a.v[i];
}

// ---------------------------------------------------------------- field phase
// points_coeffs (ipa/mod.rs:340: [1] -> each round c -> [c x, c]): round 0 decides the most
// significant bit of i, a clear bit takes the round's challenge.
VK_HD FrE s_coeff(const FrE* xs, int K, uint32_t i) {
    FrE s = fe_one<BN254Fr>();
    for (int k = 0; k < K; k++)
        if (!((i >> (K - 1 - k)) & 1u)) s = fr_mul(s, xs[k]);
    return s;
}
// entry i < N of the fixed row: -tip s_i (outside the domain multiplied by the scale afterwards)
VK_HD FrE row_entry(const FrE& tip, const FrE& s_i) { return fe_neg<BN254Fr>(fr_mul(tip, s_i)); }

// compute_barycentric_coefficients' one-hot branch (precompute.rs:75-79): the canonical point is
// below N as an integer
VK_HD bool point_in_domain(const uint32_t* point, uint64_t N, uint64_t* idx) {
    uint32_t hi = 0;
    for (int k = 2; k < 8; k++) hi |= point[k];
    *idx = (uint64_t)point[0] | ((uint64_t)point[1] << 32);
    return hi == 0 && *idx < N;
}

struct Frac {
    FrE num, den;
};
VK_HD Frac frac_zero() { return Frac{fe_zero<BN254Fr>(), fe_one<BN254Fr>()}; }
VK_HD Frac frac_add(const Frac& a, const Frac& b) {
    return Frac{fe_add<BN254Fr>(fr_mul(a.num, b.den), fr_mul(b.num, a.den)), fr_mul(a.den, b.den)};
}
// acc + s_i w^i / (z - w^i)
VK_HD Frac frac_add_term(const Frac& acc, const FrE& s_i, const FrE& w_i, const FrE& z) {
    return frac_add(acc, Frac{fr_mul(s_i, w_i), fe_sub<BN254Fr>(z, w_i)});
}
// den <b, s> from the whole sum num / den: (z^N - 1) / N * num, N = 2^K, n_inv = 1 / N. No inversion.
VK_HD FrE bary_dot_scaled(const Frac& total, const FrE& z, int K, const FrE& n_inv) {
    FrE zn = z;
    for (int k = 0; k < K; k++) zn = fr_mul(zn, zn);
    return fr_mul(fr_mul(fe_sub<BN254Fr>(zn, fe_one<BN254Fr>()), n_inv), total.num);
}
// entry N of the fixed row (over q): scale (prod x) w y - w tip cb, cb = scale <b, s>
VK_HD FrE row_tail(const FrE& prodx, const FrE& w, const FrE& y, const FrE& tip, const FrE& cb, const FrE& scale) {
    return fe_sub<BN254Fr>(fr_mul(fr_mul(fr_mul(prodx, scale), w), y), fr_mul(fr_mul(w, tip), cb));
}
// the 1 + 2K scalars of (C, L_0, R_0, .., L_{K-1}, R_{K-1}) times `scale`, as canonical words (8
// each): prod x, then P_k and P_k x_k^2 per round; returns prod x (Montgomery, not scaled)
VK_HD FrE var_scalars(const FrE* xs, int K, const FrE& scale, uint32_t* out) {
    FrE P = fe_one<BN254Fr>();
    for (int k = K - 1; k >= 0; k--) {
        fr_store(fe_from_mont<BN254Fr>(fr_mul(P, scale)), out + 8 * (1 + 2 * k));
        fr_store(fe_from_mont<BN254Fr>(fr_mul(fr_mul(P, scale), fr_mul(xs[k], xs[k]))), out + 8 * (2 + 2 * k));
        P = fr_mul(P, xs[k]);
    }
    fr_store(fe_from_mont<BN254Fr>(fr_mul(P, scale)), out);
    return P;
}

// ---------------------------------------------------------------- curve phase
// Term t of a proof: 0 is C, 1 + 2k is L_k, 2 + 2k is R_k. A lane takes the terms first, first +
// stride, .. (count of them) and sums scalar * point over them with one shared chain of doublings
// (bit by bit from the top of the 254-bit scalars, one mixed add per set bit). `get(j, P)` gives
// the lane's j-th point in Montgomery form and returns false for the identity; `bit(j, b)` is bit
// b of its canonical scalar.
template <class GetPoint, class GetBit>
VK_HD G1A var_partial_sum(int count, GetPoint get, GetBit bit) {
    G1A A = BN254G1::zero();
    for (int b = BN254Fr::BITS - 1; b >= 0; b--) {
        A = BN254G1::dbl(A);
        for (int j = 0; j < count; j++) {
            if (!bit(j, b)) continue;
            G1P P;
            if (get(j, P)) A = BN254G1::madd(A, P, false);
        }
    }
    return A;
}
// the verdict: variable part + the fixed row's commitment (canonical affine words, as the commit
// engine writes them) is the identity
VK_HD bool sum_is_identity(const G1A& var, const uint32_t* fixed_xy, bool fixed_inf) {
    if (fixed_inf) return fe_is_zero<BN254Fq>(var.zz);
    G1P F;
    F.x = fe_to_mont<BN254Fq>(words_load<BN254Fq>(fixed_xy));
    F.y = fe_to_mont<BN254Fq>(words_load<BN254Fq>(fixed_xy + 8));
    return BN254G1::is_zero(BN254G1::madd(var, F, false));
}

}  // namespace ipav
}  // namespace vk

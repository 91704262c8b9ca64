// The field arithmetic of the IPA rounds (ipa/mod.rs:199-360), once: a round's scalar rows of L
// and R, its fold and the verifier's scalars. No HIP call, no context, no transcript: ipa.hip and
// tests/cpp/ipa_rounds_check.cpp compile the same text.
// The folded generators are kept as coefficients over the original CRS (ipa.hip): in a round of
// width m = N >> r the CRS point i belongs to the folded generator j = i mod m, with coefficient
// coeff_i (all one in round 0).
#pragma once
#include <stddef.h>

#include <vector>

#include "ff.hpp"

namespace vk {
namespace ipar {

using FrE = fe<BN254Fr>;

// (zero b entries skipped: the in-domain barycentric weights are one-hot, so the IPA prover's
// evaluation and its first round's inner products are one product instead of N and N / 2)
inline FrE inner(const FrE* a, const FrE* b, size_t n) {
    FrE s = fe_zero<BN254Fr>();
    for (size_t i = 0; i < n; i++)
        if (!fe_is_zero<BN254Fr>(b[i])) s = fe_add<BN254Fr>(s, fe_mul<BN254Fr>(a[i], b[i]));
    return s;
}

// the scalars of q in L and R: q' <a_L, b_R> = q (w <a_L, b_R>), and the mirror
inline void q_terms(const FrE* a, const FrE* b, const FrE& w, size_t half, FrE* qL, FrE* qR) {
    *qL = fe_mul<BN254Fr>(w, inner(a, b + half, half));
    *qR = fe_mul<BN254Fr>(w, inner(a + half, b, half));
}

// ---- the rows and the fold entry by entry (host and device: csrc/ipa_many.hpp's lanes take one
// entry each, the loops below take them all)
// whether CRS point i of a round of width m (half = m / 2) belongs to L's row (else to R's)
VK_HD bool row_is_left(size_t i, size_t m, size_t half) { return (i % m) >= half; }
// the entry of a that CRS point i multiplies in its row: a_L for L's bases, a_R for R's
VK_HD size_t row_source(size_t i, size_t m, size_t half) {
    const size_t j = i % m;
    return j >= half ? j - half : j + half;
}
// whether the fold of a round of width m multiplies coefficient i by the challenge
VK_HD bool coeff_folds(size_t i, size_t m, size_t half) { return (i % m) < half; }
VK_HD FrE fold_a_at(const FrE& x, const FrE& a_lo, const FrE& a_hi) {  // a_L + x a_R
    return fe_add<BN254Fr>(a_lo, fe_mul<BN254Fr>(x, a_hi));
}
VK_HD FrE fold_b_at(const FrE& x, const FrE& b_lo, const FrE& b_hi) {  // b_R + x b_L
    return fe_add<BN254Fr>(b_hi, fe_mul<BN254Fr>(x, b_lo));
}

// One round's rows of one proof, sL[0..N) and sR[0..N): L = <gens_R, a_L> takes the bases with
// i mod m >= half, R = <gens_L, a_R> the others. coeff == nullptr: every coefficient is one (round
// 0 -- the rows are a's halves as they are, no multiply). With b (and w) the q terms go to index N.
inline void round_rows(const FrE* a, const FrE* coeff, size_t N, size_t m, size_t half, FrE* sL, FrE* sR,
                       const FrE* b = nullptr, const FrE* w = nullptr) {
    for (size_t i = 0; i < N; i++) {
        const FrE& src = a[row_source(i, m, half)];
        const FrE v = coeff ? fe_mul<BN254Fr>(src, coeff[i]) : src;
        const bool left = row_is_left(i, m, half);
        sL[i] = left ? v : fe_zero<BN254Fr>();
        sR[i] = left ? fe_zero<BN254Fr>() : v;
    }
    if (b) q_terms(a, b, *w, half, &sL[N], &sR[N]);
}

// One round's fold by x: a <- a_L + x a_R; with b, b <- b_R + x b_L; with host coefficients,
// g <- g_R + x g_L, i.e. coeff_i *= x where i mod m < half.
inline void round_fold(const FrE& x, size_t N, size_t m, size_t half, std::vector<FrE>& a, std::vector<FrE>* b,
                       FrE* coeff) {
    for (size_t j = 0; j < half; j++) {
        a[j] = fold_a_at(x, a[j], a[j + half]);
        if (b) (*b)[j] = fold_b_at(x, (*b)[j], (*b)[j + half]);
    }
    a.resize(half);
    if (b) b->resize(half);
    if (coeff)
        for (size_t i = 0; i < N; i++)
            if (coeff_folds(i, m, half)) coeff[i] = fe_mul<BN254Fr>(coeff[i], x);
}

// The verifier's scalars from the challenges xs[0..K), Montgomery: s = points_coeffs ([1] -> each
// round c -> [c x, c]; 2^K entries, one multiply each) and vs, the 1 + 2K scalars of (C, L_0, R_0,
// .., L_{K-1}, R_{K-1}): prod x, then P_k and P_k x_k^2 with P_k = prod_{j>k} x_j. Returns prod x.
inline FrE verifier_scalars(const FrE* xs, size_t K, std::vector<FrE>& s, std::vector<FrE>& vs) {
    s.assign((size_t)1 << K, fe_one<BN254Fr>());
    for (size_t k = 0; k < K; k++)
        for (size_t i = (size_t)1 << k; i-- > 0;) {  // in place from the top: 2 i + 1 >= i
            s[2 * i + 1] = s[i];
            s[2 * i] = fe_mul<BN254Fr>(s[i], xs[k]);
        }
    vs.resize(1 + 2 * K);
    FrE P = fe_one<BN254Fr>();
    for (size_t k = K; k-- > 0;) {
        vs[1 + 2 * k] = P;
        vs[2 + 2 * k] = fe_mul<BN254Fr>(P, fe_sqr<BN254Fr>(xs[k]));
        P = fe_mul<BN254Fr>(P, xs[k]);
    }
    vs[0] = P;
    return P;
}

}  // namespace ipar
}  // namespace vk

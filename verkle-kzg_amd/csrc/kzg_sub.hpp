// Per-lane arithmetic of KZG subvector proving (vc_kzg_prove_subvector_many), host + gfx950 device
// from one source: the kernel of kzg_sub.hip is a wrapper that adds the cross-lane steps (xor
// shuffles, the fence between the weight pass and its readers), and tests/cpp/kzg_sub_check.cpp runs
// the same text on the host, 64 lanes in a loop.
//
// One subset S of k distinct indices below N of a row f (zero beyond `width`): the proof is the commit
// of q = (f - I) / Z_S, Z_S = prod_{i in S} (X - w^i), I the interpolant of f on S. By partial
// fractions q = sum_{i in S} c_i q^(i) with c_i = 1 / Z_S'(w^i) and q^(i) the single-point quotient of
// index i (kzg_many.hpp, in the domain). With the cached tables pw[i] = w^i and inv1[k] =
// 1 / (w^k - 1) (inv1[0] = 0), 1 / (w^a - w^b) = w^-b inv1[(a - b) mod N]:
//   c_i  = prod_{l in S, l != i} w^-l inv1[(i - l) mod N]
//        = w^(i - sum S) prod_{l != i} inv1[(i - l) mod N]
//   cw_i = c_i w^-i = w^(-sum S) prod_{l != i} inv1[(i - l) mod N]          (what the passes keep)
//   q_j  = sum_{i in S} cw_i (f_j - f_i) inv1[(j - i) mod N]                 (the term i = j is zero)
//        - [j in S] cw_j D_j,
//   D_m  = sum_{i != m} (f_i - f_m) w^i / (w^i - w^m) = sum_i (f_i - f_m) (1 + inv1[(i - m) mod N]),
// D_m being kzg_many.hpp's in-domain sum (the wave's total of in_pass, whose terms w^i w^-m
// inv1[i - m] are 1 + inv1[i - m]: one multiply per entry here, and no store into the row, which
// holds the subset's sum already), and -cw_m D_m = c_m in_qm(w^-m, D_m), the entry m of q^(m). No
// inversion. A wave takes one subset; lane l holds the subset's entries t = l, l + 64, .. < k in the
// weight pass and the row's entries j = l, l + 64, .. < N in the other two.
#pragma once
#include "kzg_many.hpp"

namespace vk {
namespace kzgs {

using kzgm::row_at;

// w^(-sum S) from the sum of the subset's indices
template <class F>
VK_HD fe<F> sub_wsum(const fe<F>* pw, uint32_t N, uint32_t sum) {
    return pw[(N - (sum & (N - 1))) & (N - 1)];
}
// cw_t of the subset's t-th index
template <class F>
VK_HD fe<F> sub_weight(const uint32_t* S, uint32_t k, const fe<F>* inv1, uint32_t N, uint32_t t, const fe<F>& wsum) {
    const uint32_t i = S[t];
    fe<F> c = wsum;
#pragma unroll 1
    for (uint32_t l = 0; l < k; l++) {
        if (l == t) continue;
        c = fe_mul<F>(c, inv1[(i + N - S[l]) & (N - 1)]);
    }
    return c;
}
// c_i from cw_i
template <class F>
VK_HD fe<F> sub_weight_full(const fe<F>& cw, const fe<F>* pw, uint32_t i) {
    return fe_mul<F>(cw, pw[i]);
}
// the row's entry j without its diagonal term
template <class F>
VK_HD fe<F> sub_row_entry(const fe<F>* f, uint32_t width, const uint32_t* S, uint32_t k, const fe<F>* cw,
                          const fe<F>* inv1, uint32_t N, uint32_t j) {
    const fe<F> fj = row_at<F>(f, width, j);
    fe<F> acc = fe_zero<F>();
#pragma unroll 1
    for (uint32_t t = 0; t < k; t++) {
        const uint32_t i = S[t];
        const fe<F> d = fe_mul<F>(fe_sub<F>(fj, row_at<F>(f, width, i)), inv1[(j + N - i) & (N - 1)]);
        acc = fe_add<F>(acc, fe_mul<F>(cw[t], d));
    }
    return acc;
}
// the lane's part of D_m
template <class F>
VK_HD fe<F> sub_diag_pass(const fe<F>* f, uint32_t width, const fe<F>* inv1, uint32_t N, uint32_t m, const fe<F>& fm,
                          uint32_t lane) {
    const fe<F> one = fe_one<F>();
    fe<F> acc = fe_zero<F>();
#pragma unroll 1
    for (uint32_t i = lane; i < N; i += 64)
        acc = fe_add<F>(acc, fe_mul<F>(fe_sub<F>(row_at<F>(f, width, i), fm), fe_add<F>(inv1[(i + N - m) & (N - 1)], one)));
    return acc;
}
// q_m from the row's entry and the wave's D_m
template <class F>
VK_HD fe<F> sub_diag(const fe<F>& qm, const fe<F>& cw, const fe<F>& total) {
    return fe_sub<F>(qm, fe_mul<F>(cw, total));
}

}  // namespace kzgs
}  // namespace vk

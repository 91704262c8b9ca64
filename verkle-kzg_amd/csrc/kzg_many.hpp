// Per-lane arithmetic of KZG batch proving (vc_kzg_prove_many), host + gfx950 device from one
// source: the kernels of kzg_many.hip are wrappers that add the cross-lane steps (xor shuffles), and
// tests/cpp/kzg_many_check.cpp runs the same text on the host, 64 lanes in a loop.
//
// One opening is KZG::prove_point (kzg/mod.rs:136-154) of a row f of `width` <= N values at a point
// z: y = f(z) and the quotient q with q_i = (f_i - y) / (w^i - z), the proof being the commit of q.
// A wave takes one opening; lane l holds the entries i = l, l + 64, .. < N (for N < 64 the upper
// lanes hold nothing: the neutral element of every fold).
//
// In the domain at m = z < N (lagrange_basis.rs:91-119): with the cached tables pw[i] = w^i and
// inv1[k] = 1 / (w^k - 1), 1 / (w^i - w^m) = w^-m inv1[(i - m) mod N] and w^-m = pw[(N - m) mod N]:
//   q_i = (f_i - f_m) w^-m inv1[(i - m) mod N]  (i != m),   q_m = -w^-m sum_{i != m} q_i w^i,
// y = f_m (0 for m >= width). No inversion.
//
// Outside the domain (lagrange_basis.rs:121-142, precompute.rs:72-90): the N inverses 1 / (w^i - z)
// share one inversion. For even N, prod_j (w^j - z) = z^N - 1 =: D, so with E_i = prod_{j != i}
// (w^j - z) the inverses are E_i / D. 1 / D comes from outside (one batch inversion for the whole
// chunk of openings); E_i is (the product of the other lanes' totals) x (the lane's own other
// entries). The latter are a prefix and a suffix product over the lane's entries: the forward pass
// leaves the exclusive prefixes in the quotient row itself, the backward pass carries the suffix and
// replaces each prefix by the finished inverse. The former is one xor butterfly over the lane
// totals: at step s a lane multiplies what it has of the others by the total of its partner's block
// of s lanes, and its own block's total likewise -- six shuffles and twelve multiplies, the prefix
// and suffix scans' result without their second shuffle. After it every lane also holds D.
//   y   = -(D / N) sum_i f_i w^i / (w^i - z)      (barycentric, precompute.rs:86 with t = D / N)
//   q_i = (f_i - y) / (w^i - z)
#pragma once
#include "ff.hpp"
#include "kzg_point.hpp"  // the point's class, z^N - 1 and the status rules, shared with the single open

namespace vk {
namespace kzgm {

constexpr uint32_t KM_MAX_N = 1024;

template <class F>
VK_HD fe<F> row_at(const fe<F>* f, uint32_t width, uint32_t i) {
    return i < width ? f[i] : fe_zero<F>();
}

// ---------------------------------------------------------------- in the domain at m
// the lane's q_i (written to q) and its part of sum_{i != m} q_i w^i
template <class F>
VK_HD fe<F> in_pass(const fe<F>* f, uint32_t width, const fe<F>* pw, const fe<F>* inv1, uint32_t N, uint32_t m,
                    const fe<F>& fm, const fe<F>& wminv, uint32_t lane, fe<F>* q) {
    fe<F> acc = fe_zero<F>();
#pragma unroll 1
    for (uint32_t i = lane; i < N; i += 64) {
        if (i == m) continue;
        const fe<F> inv = fe_mul<F>(wminv, inv1[(i + N - m) & (N - 1)]);  // 1 / (w^i - w^m)
        const fe<F> qi = fe_mul<F>(fe_sub<F>(row_at<F>(f, width, i), fm), inv);
        q[i] = qi;
        acc = fe_add<F>(acc, fe_mul<F>(qi, pw[i]));
    }
    return acc;
}
// q_m from the wave's sum
template <class F>
VK_HD fe<F> in_qm(const fe<F>& wminv, const fe<F>& total) {
    return fe_neg<F>(fe_mul<F>(wminv, total));
}

// ---------------------------------------------------------------- outside the domain
// forward: the exclusive prefix products of the lane's w^i - z into q; returns the lane's total
// (one for a lane without entries)
template <class F>
VK_HD fe<F> out_prefix_pass(const fe<F>* pw, uint32_t N, const fe<F>& z, uint32_t lane, fe<F>* q) {
    fe<F> run = fe_one<F>();
#pragma unroll 1
    for (uint32_t i = lane; i < N; i += 64) {
        q[i] = run;
        run = fe_mul<F>(run, fe_sub<F>(pw[i], z));
    }
    return run;
}
// one butterfly step: pt is the partner's `tot` (read before this lane's changes)
template <class F>
VK_HD void others_step(fe<F>& tot, fe<F>& oth, const fe<F>& pt) {
    oth = fe_mul<F>(oth, pt);
    tot = fe_mul<F>(tot, pt);
}
// backward: q_i <- 1 / (w^i - z) = prefix_i * suffix_i * oth_dinv, oth_dinv = (the other lanes'
// product) / D; returns the lane's part of sum_i f_i w^i / (w^i - z)
template <class F>
VK_HD fe<F> out_inverse_pass(const fe<F>* f, uint32_t width, const fe<F>* pw, uint32_t N, const fe<F>& z,
                             const fe<F>& oth_dinv, uint32_t lane, fe<F>* q) {
    fe<F> acc = fe_zero<F>();
    if (lane >= N) return acc;
    fe<F> suf = oth_dinv;
#pragma unroll 1
    for (uint32_t i = lane + ((N - 1 - lane) & ~63u);; i -= 64) {  // the lane's last entry first
        const fe<F> e = fe_mul<F>(q[i], suf);
        q[i] = e;
        if (i < width) acc = fe_add<F>(acc, fe_mul<F>(fe_mul<F>(f[i], pw[i]), e));
        if (i < 64) break;
        suf = fe_mul<F>(suf, fe_sub<F>(pw[i], z));
    }
    return acc;
}
// y = -(D / N) total, n_inv = 1 / N
template <class F>
VK_HD fe<F> out_y(const fe<F>& D, const fe<F>& n_inv, const fe<F>& total) {
    return fe_neg<F>(fe_mul<F>(fe_mul<F>(D, n_inv), total));
}
// q_i <- (f_i - y) q_i
template <class F>
VK_HD void out_quotient_pass(const fe<F>* f, uint32_t width, uint32_t N, const fe<F>& y, uint32_t lane, fe<F>* q) {
#pragma unroll 1
    for (uint32_t i = lane; i < N; i += 64) q[i] = fe_mul<F>(fe_sub<F>(row_at<F>(f, width, i), y), q[i]);
}

}  // namespace kzgm
}  // namespace vk

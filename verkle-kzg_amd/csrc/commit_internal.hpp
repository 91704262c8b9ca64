// What the fixed-base sources share (fb_table.hip: the window tables; commit.hip: the commits over
// them): the curve's scalar field, a scalar's signed window digits, the first-use table size.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "ctx.hpp"
#include "ec.hpp"

namespace vk {

// the scalar field of a curve's group order (signed digits need windows covering BITS + 1)
template <class C>
using ScalarOf = typename std::conditional<std::is_same<C, BN254G1>::value, BN254Fr,
                                           typename std::conditional<std::is_same<C, BLS381G1>::value, BLS381Fr,
                                                                     BandFr>::type>::type;

// signed digits of a scalar over the table's windows (widths g.width(w)): d in (-2^(cw-1), 2^(cw-1)]
template <class Fr>
struct FbDigits {
    fe<Fr> s;
    uint32_t carry = 0;
    __device__ __forceinline__ int32_t next(int cw) {
        const uint32_t mask = (1u << cw) - 1, half = 1u << (cw - 1);
        const uint32_t raw = (s.v[0] & mask) + carry;
#pragma unroll
        for (int k = 0; k < 7; k++) s.v[k] = (s.v[k] >> cw) | (s.v[k + 1] << (32 - cw));
        s.v[7] >>= cw;
        carry = raw > half ? 1u : 0u;
        return carry ? (int32_t)raw - (int32_t)(1u << cw) : (int32_t)raw;
    }
};

template <class Fr>
__device__ __forceinline__ fe<Fr> load_scalar_fb(const uint32_t* __restrict__ sc, size_t i) {
    const uint4* p = reinterpret_cast<const uint4*>(sc + 8 * i);
    uint4 a = p[0], b = p[1];
    fe<Fr> s;
    s.v[0] = a.x; s.v[1] = a.y; s.v[2] = a.z; s.v[3] = a.w;
    s.v[4] = b.x; s.v[5] = b.y; s.v[6] = b.z; s.v[7] = b.w;
    return s;
}

// window bits of the fixed-base tables a commit builds on first use (a table without
// vc_fixed_base_precompute: the IPA CRS of the prover / verifier, the multiproof's D / E): the
// widest c <= 16 whose table fits what is left of the context's budget for such tables
// (VKZG_FB_BUDGET_GB, default 20 GB of the card's 288, less the ones built before and still held)
// and into the device's free memory less a 4 GB margin (hipMemGetInfo), at least 8; a build that
// still fails for memory retries one window bit narrower, down to 8 (fb_commit_t).
// Fewer windows mean fewer table points per commit, hence fewer latency-path blocks and block
// partials: the 257-point IPA CRS at c = 16 (16 windows, 17.2 GB) proves in 0.64 ms against 0.73 at
// c = 8 (32 windows, 134 MB), the multiproof finish 0.99 against 1.15 ms (profiles/r05/fb_default_c/).
template <class Fr>
static double fb_auto_bytes(size_t n, int c) {
    const size_t W = (size_t)(Fr::BITS + 1 + c - 1) / c;
    return (double)n * (double)W * (double)(1u << (c - 1)) * 128.0;
}
template <class Fr>
static int fb_default_c(size_t n, size_t used) {
    static const double budget_gb = getenv("VKZG_FB_BUDGET_GB") ? atof(getenv("VKZG_FB_BUDGET_GB")) : 20.0;
    double limit = budget_gb * 1e9 - (double)used;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) limit = std::min(limit, (double)free_b - 4e9);
    for (int c = 16; c > 8; c--)
        if (fb_auto_bytes<Fr>(n, c) <= limit) return c;
    return 8;
}

}  // namespace vk

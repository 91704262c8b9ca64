// Scalars -> signed window digits: the digit sources the bucket sort reads (msm_sort.hpp) and the GLV
// split of BLS12-381 scalars (its fused form k_glv_radix_hist is with the sort). Templates, instantiated by msm.hip (sparse_commit.hip takes load_scalar).
#pragma once
#include <hip/hip_runtime.h>
#include "ff.hpp"

namespace vk {
template <class Fr>
__device__ __forceinline__ fe<Fr> load_scalar(const uint32_t* __restrict__ sc, size_t i) {
    const uint4* p = reinterpret_cast<const uint4*>(sc + 8 * i);
    uint4 a = p[0], b = p[1];
    fe<Fr> s;
    s.v[0] = a.x; s.v[1] = a.y; s.v[2] = a.z; s.v[3] = a.w;
    s.v[4] = b.x; s.v[5] = b.y; s.v[6] = b.z; s.v[7] = b.w;
    return s;
}

// Signed c-bit digits of one scalar, least significant window first: d_w in (-2^(c-1), 2^(c-1)],
// carry into the next window; W windows have one spare bit, so the last carry is absorbed.
template <class Fr, class Fn>
__device__ __forceinline__ void for_each_digit(fe<Fr> s, int c, int W, Fn&& f) {
    const uint32_t mask = (1u << c) - 1, half = 1u << (c - 1);
    uint32_t carry = 0;
    for (int w = 0; w < W; w++) {
        uint32_t raw = (s.v[0] & mask) + carry;
#pragma unroll
        for (int k = 0; k < 7; k++) s.v[k] = (s.v[k] >> c) | (s.v[k + 1] << (32 - c));
        s.v[7] >>= c;
        int32_t d;
        if (raw > half) {
            d = (int32_t)raw - (int32_t)(1u << c);
            carry = 1;
        } else {
            d = (int32_t)raw;
            carry = 0;
        }
        f(w, d);
    }
}

// Digits of a 4-limb magnitude (GLV halves, < 2^127), same recoding.
template <class Fn>
__device__ __forceinline__ void for_each_digit4(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, int c, int W,
                                                Fn&& f) {
    const uint32_t mask = (1u << c) - 1, half = 1u << (c - 1);
    uint32_t carry = 0;
    for (int w = 0; w < W; w++) {
        uint32_t raw = (s0 & mask) + carry;
        s0 = (s0 >> c) | (s1 << (32 - c));
        s1 = (s1 >> c) | (s2 << (32 - c));
        s2 = (s2 >> c) | (s3 << (32 - c));
        s3 >>= c;
        int32_t d;
        if (raw > half) {
            d = (int32_t)raw - (int32_t)(1u << c);
            carry = 1;
        } else {
            d = (int32_t)raw;
            carry = 0;
        }
        f(w, d);
    }
}

// Digit sources of the sort: entry i of the MSM -> its signed digits (nothing for an identity base).
// Every digit source maps its term i to the point index of the shared-window copies (Table::win,
// [w][2N] for a table of N points): the identity for a whole-table MSM; a point range [off, off + n)
// of the table (RadixDigits with half = n, gap = N - n) puts k1 term i < n at off + i and k2 term
// n + j at N + off + j.
template <class Fr>
struct ScalarDigits {  // plain scalars, canonical or Montgomery
    const uint32_t* sc;
    const uint8_t* inf;
    int mont;
    __device__ __forceinline__ uint32_t pt(uint32_t i) const { return i; }
    template <class Fn>
    __device__ __forceinline__ void operator()(uint32_t i, int c, int W, Fn&& f) const {
        if (inf != nullptr && inf[i]) return;
        fe<Fr> s = load_scalar<Fr>(sc, i);
        if (mont) s = fe_from_mont<Fr>(s);
        for_each_digit<Fr>(s, c, W, f);
    }
};
// GLV halves (k_glv_split): entry i < n is k1 of scalar i against P_i, entry n + i is k2 against
// phi(P_i); magnitude in bits 0..126, sign in bit 127 (a negative half negates every digit).
// Shared windows with a short top window (tw >= 0): its digits are scaled by 2^ts -- the window
// copy of that window holds 2^(c tw - ts) P -- so they spread over the whole bucket range
// instead of piling into the lowest 2^-ts of it.
struct GlvDigits {
    const uint4* k;
    const uint8_t* inf;
    uint32_t n;
    int tw = -1, ts = 0;
    __device__ __forceinline__ uint32_t pt(uint32_t i) const { return i; }
    template <class Fn>
    __device__ __forceinline__ void operator()(uint32_t i, int c, int W, Fn&& f) const {
        if (inf != nullptr && inf[i < n ? i : i - n]) return;
        const uint4 v = k[i];
        const bool neg = (v.w >> 31) != 0;
        for_each_digit4(v.x, v.y, v.z, v.w & 0x7fffffffu, c, W, [&](int w, int32_t d) {
            if (w == tw) d *= (1 << ts);
            f(w, neg ? -d : d);
        });
    }
};

// Radix-B digits made by k_glv_radix ([W][nv] signed, zero for identity bases): entry i of the
// (2n-term) MSM has digit dig[w * nv + i] in window w.
struct RadixDigits {
    const int32_t* dig;
    uint32_t nv;
    int w0 = 0;  // first window read (a per-set coarse pass of several bucket sets starts at its set)
    uint32_t off = 0, half = 0xffffffffu, gap = 0;  // point range of the table (see above)
    __device__ __forceinline__ uint32_t pt(uint32_t i) const { return i + off + (i >= half ? gap : 0u); }
    template <class Fn>
    __device__ __forceinline__ void operator()(uint32_t i, int, int W, Fn&& f) const {
        for (int w = w0; w < W; w++) f(w, dig[(size_t)w * nv + i]);
    }
};

// ------------------------------------------------------------------ GLV endomorphism (BLS12-381 G1)
// phi(x, y) = (beta x, y) acts on the prime-order subgroup as multiplication by
// lambda = z^2 - 1 (z = -0xd201000000010000), and r = lambda^2 + lambda + 1. A scalar splits as
// k = k1 + lambda k2 with |k1|, |k2| <= lambda/2 + 1 < 2^127, so an n-term MSM is a 2n-term MSM
// of 127-bit scalars over (P_i, phi(P_i)): the same number of accumulate entries (2n x 8
// windows instead of n x 16 at c = 16) but half the buckets, half the bucket reduction and
// half the Horner doublings. Used only when every base of the table is in the subgroup
// (checked once per table: phi^2(P) = -z^2 P, which non-subgroup points fail), so the result
// is the same group element as the reference's sum of k_i P_i for any input.
struct GlvK {
    uint64_t lam[2];
    uint64_t mu[3];  // floor(2^256 / lambda)
    uint64_t r[4];
};
constexpr size_t GLV_MIN_N = 4096;
constexpr int GLV_BITS = 128;  // |k1|, |k2| < 2^127, plus the recoding's spare bit

typedef unsigned __int128 u128;

// k = k1 + lambda k2 (k < 2^256, canonical or not): |k1| = rem (negative when nr), |k2| = q (nq)
__device__ __forceinline__ void glv_decompose(uint64_t s[4], const GlvK& K, u128& rem, bool& nr, u128& q, bool& nq) {
    // s mod r (inputs are < 2^256 < 3r)
    for (int rep = 0; rep < 2; rep++) {
        bool ge = true;
        for (int k = 3; k >= 0; k--)
            if (s[k] != K.r[k]) {
                ge = s[k] > K.r[k];
                break;
            }
        if (!ge) break;
        uint64_t br = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            u128 d = (u128)s[k] - K.r[k] - br;
            s[k] = (uint64_t)d;
            br = (uint64_t)(d >> 64) & 1;
        }
    }
    // q = floor(s mu / 2^256): floor(s / lambda) or up to 2 less
    uint64_t p[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < 4; a++) {
        uint64_t carry = 0;
#pragma unroll
        for (int b = 0; b < 3; b++) {
            u128 t = (u128)s[a] * K.mu[b] + p[a + b] + carry;
            p[a + b] = (uint64_t)t;
            carry = (uint64_t)(t >> 64);
        }
        p[a + 3] = carry;
    }
    q = ((u128)p[5] << 64) | p[4];
    const u128 lam = ((u128)K.lam[1] << 64) | K.lam[0];
    // rem = s - q lambda (< 3 lambda: 3 limbs)
    uint64_t ql[4] = {0, 0, 0, 0};
    const uint64_t qv[2] = {(uint64_t)q, (uint64_t)(q >> 64)};
#pragma unroll
    for (int a = 0; a < 2; a++) {
        uint64_t carry = 0;
#pragma unroll
        for (int b = 0; b < 2; b++) {
            u128 t = (u128)qv[a] * K.lam[b] + ql[a + b] + carry;
            ql[a + b] = (uint64_t)t;
            carry = (uint64_t)(t >> 64);
        }
        ql[a + 2] = carry;
    }
    uint64_t rm[3];
    {
        uint64_t br = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            u128 d = (u128)s[k] - ql[k] - br;
            rm[k] = (uint64_t)d;
            br = (uint64_t)(d >> 64) & 1;
        }
    }
    for (int it = 0; it < 4; it++) {  // at most 2 corrections
        const u128 lo = ((u128)rm[1] << 64) | rm[0];
        if (rm[2] == 0 && lo < lam) break;
        const u128 d = lo - lam;
        if (lo < lam) rm[2] -= 1;
        rm[0] = (uint64_t)d;
        rm[1] = (uint64_t)(d >> 64);
        q += 1;
    }
    rem = ((u128)rm[1] << 64) | rm[0];
    // balance: k = rem + lambda q with rem in [0, lambda), q in [0, lambda + 1]
    //   q > lambda/2:   (rem - 1) + lambda (q - lambda - 1)   (= k - r)
    //   rem > lambda/2: (rem - lambda) + lambda (q + 1)
    const u128 half = lam >> 1;
    nq = false;
    nr = false;
    if (q > half) {
        q = lam + 1 - q;  // magnitude of q - lambda - 1
        nq = true;
        if (rem == 0) {
            rem = 1;
            nr = true;
        } else {
            rem -= 1;
        }
    }
    if (!nr && rem > half) {
        rem = lam - rem;
        nr = true;
        if (!nq) {
            q += 1;
        } else if (q == 0) {
            q = 1;
            nq = false;
        } else {
            q -= 1;
        }
    }
}

template <class Fr>
__device__ __forceinline__ void glv_load(const uint32_t* __restrict__ sc, uint32_t i, int mont, uint64_t s[4]) {
    fe<Fr> f = load_scalar<Fr>(sc, i);
    if (mont) f = fe_from_mont<Fr>(f);
#pragma unroll
    for (int k = 0; k < 4; k++) s[k] = (uint64_t)f.v[2 * k] | ((uint64_t)f.v[2 * k + 1] << 32);
}

template <class Fr>
__global__ void __launch_bounds__(256) k_glv_split(const uint32_t* __restrict__ sc, uint32_t n, int mont, GlvK K,
                                                  uint4* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t s[4];
    glv_load<Fr>(sc, i, mont, s);
    u128 rem, q;
    bool nr, nq;
    glv_decompose(s, K, rem, nr, q, nq);
    out[i] = make_uint4((uint32_t)rem, (uint32_t)(rem >> 32), (uint32_t)(rem >> 64),
                        (uint32_t)(rem >> 96) | (nr ? 0x80000000u : 0u));
    out[n + i] = make_uint4((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)(q >> 64),
                            (uint32_t)(q >> 96) | (nq ? 0x80000000u : 0u));
}

// Mixed-radix digits of a GLV half for the radix-B shared-window MSM (B = MUL 2^C0, not a power
// of two): |k| < 2^127 = sum_w d_w B^w with signed d_w in (-B/2, B/2] (carry recoding as
// for_each_digit), W digits (B^W / 2 > 2^127: the top digit is below B/2 and never carries).
// k mod B = (k mod 2^C0) + 2^C0 ((k >> C0) mod MUL); the division by MUL runs over the four
// 32-bit limbs from the top. A negative half negates every digit.
// (rem 2^32 + x) / MUL for rem < MUL, in 32-bit steps (2^32 = MUL Q + 1 for MUL | 2^32 - 1):
// x = MUL q0 + x0 with q0 by a multiply-high, then rem + x0 < 2 MUL carries at most one
template <uint32_t MUL>
__device__ __forceinline__ uint32_t div_step(uint32_t x, uint32_t& rem) {
    static_assert(MUL == 5 || MUL == 3, "2^32 = 1 mod MUL");
    constexpr uint32_t Q = (uint32_t)(0xffffffffull / MUL);  // (2^32 - 1) / MUL
    const uint32_t q0 = MUL == 5 ? __umulhi(x, 0xCCCCCCCDu) >> 2 : __umulhi(x, 0xAAAAAAABu) >> 1;
    const uint32_t t = rem + (x - q0 * MUL);
    const uint32_t ge = t >= MUL ? 1u : 0u;
    const uint32_t q = rem * Q + q0 + ge;
    rem = t - ge * MUL;
    return q;
}

template <uint32_t MUL, int C0, class Fn>
__device__ __forceinline__ void radix_digits(u128 k, bool neg, int W, Fn&& f) {
    constexpr uint32_t B = MUL << C0, H = B / 2, LO = (1u << C0) - 1;
    uint32_t x0 = (uint32_t)k, x1 = (uint32_t)(k >> 32), x2 = (uint32_t)(k >> 64), x3 = (uint32_t)(k >> 96);
    uint32_t carry = 0;
    for (int w = 0; w < W; w++) {
        const uint32_t lo = x0 & LO;
        x0 = (x0 >> C0) | (x1 << (32 - C0));
        x1 = (x1 >> C0) | (x2 << (32 - C0));
        x2 = (x2 >> C0) | (x3 << (32 - C0));
        x3 >>= C0;
        uint32_t rem = 0;
        x3 = div_step<MUL>(x3, rem);
        x2 = div_step<MUL>(x2, rem);
        x1 = div_step<MUL>(x1, rem);
        x0 = div_step<MUL>(x0, rem);
        const uint32_t raw = lo + (rem << C0) + carry;
        int32_t d;
        if (raw > H) {
            d = (int32_t)raw - (int32_t)B;
            carry = 1;
        } else {
            d = (int32_t)raw;
            carry = 0;
        }
        f(w, neg ? -d : d);
    }
}

// GLV split straight to radix-B digits: dig[w][i] (k1 of scalar i against P_i) and dig[w][n + i]
// (k2 against phi(P_i)); identity bases get zero digits (no entries)
template <class Fr, uint32_t MUL, int C0>
__global__ void __launch_bounds__(256) k_glv_radix(const uint32_t* __restrict__ sc, const uint8_t* __restrict__ inf,
                                                  uint32_t n, int mont, GlvK K, int W, int32_t* __restrict__ dig) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t nv = 2 * (size_t)n;
    if (inf != nullptr && inf[i]) {
        for (int w = 0; w < W; w++) dig[(size_t)w * nv + i] = dig[(size_t)w * nv + n + i] = 0;
        return;
    }
    uint64_t s[4];
    glv_load<Fr>(sc, i, mont, s);
    u128 rem, q;
    bool nr, nq;
    glv_decompose(s, K, rem, nr, q, nq);
    radix_digits<MUL, C0>(rem, nr, W, [&](int w, int32_t d) { dig[(size_t)w * nv + i] = d; });
    radix_digits<MUL, C0>(q, nq, W, [&](int w, int32_t d) { dig[(size_t)w * nv + n + i] = d; });
}
}  // namespace vk

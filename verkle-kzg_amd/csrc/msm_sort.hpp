// The bucket sort of the Pippenger MSM (msm.hip): kernels and their launcher sort_entries,
// templates over the digit source (msm_digits.hpp), instantiated by msm.hip; and the GLV split
// that writes the sort's histogram itself (k_glv_radix_hist).
#pragma once
#include <hipcub/hipcub.hpp>
#include <mutex>
#include <set>
#include <utility>
#include "msm_accumulate.hpp"  // AccStart
#include "msm_digits.hpp"      // RadixDigits

namespace vk {
// Two-pass MSD counting sort of the n*W (window, bucket) keys, all in LDS -- no global atomics
// (global atomics execute memory-side on CDNA4, ~26 G/s for scattered words, which made the
// one-pass global-histogram sort cost 2.2 ms at 2^20 x 16 windows).
//   coarse bin g = w * NBC + (b >> FB)          (NBC = NB >> FB coarse bins per window)
//   k_sort_hist     block = CHUNK entries: LDS histogram of coarse bins -> counts[g][block]
//   hipcub scan     counts -> base[g][block] (global position of the block's run in bin g)
//   k_sort_coarse   same digits again, LDS cursors from base: tmp[pos] = fine<<32 | i | sign<<31
//   k_sort_fine     block = coarse bin: LDS histogram of the 2^FB fine buckets -> bucket
//                   offsets (written directly), then scatter into sorted[]
// Order inside a bucket is arbitrary (EC addition is commutative and exact).
// Shared windows (stride != 0): every window's digits go to ONE set of buckets and the entry
// names the point 2^(c w) P_i by its index w * stride + i in the window copies (Table::win).
#ifndef VK_SORT_CHUNK
#define VK_SORT_CHUNK 1024
#endif
constexpr uint32_t SORT_CHUNK = VK_SORT_CHUNK;

// XCD-aware run order: blocks are dispatched round-robin over the 8 XCDs (block b on XCD b % 8),
// each with its own L2. A block's run inside every coarse bin sits at its slot in this order, so
// the runs of one XCD's blocks are adjacent and the partial-line writes of the scatter merge in
// ONE L2 instead of being written back as masked partial lines by several.
__device__ __forceinline__ uint32_t sort_slot(uint32_t b, uint32_t nblk) {
    const uint32_t q = nblk / 8, rem = nblk % 8, x = b % 8;
    return x * q + min(x, rem) + b / 8;
}

template <class Src>
__global__ void __launch_bounds__(1024) k_sort_hist(Src src, uint32_t n, int c, int wb, int we, uint32_t FB,
                                                   uint32_t NBC, uint32_t nblk, uint32_t stride, uint32_t wps,
                                                   uint32_t chunk, uint32_t* __restrict__ counts) {
    extern __shared__ uint32_t hist[];
    // shared windows: windows [s wps, (s + 1) wps) fill bucket set s (several MSMs over one table)
    const uint32_t bins = (stride ? ((uint32_t)we + wps - 1) / wps : (uint32_t)(we - wb)) * NBC;
    for (uint32_t k = threadIdx.x; k < bins; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    const uint32_t lo = blockIdx.x * chunk, hi = min(lo + chunk, n);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        src(i, c, we, [&](int w, int32_t d) {
            if (d != 0 && w >= wb)
                atomicAdd(&hist[(stride ? (uint32_t)w / wps : (uint32_t)(w - wb)) * NBC +
                                (((uint32_t)(d < 0 ? -d : d) - 1) >> FB)],
                          1u);
        });
    }
    __syncthreads();
    const uint32_t slot = sort_slot(blockIdx.x, nblk);
    for (uint32_t k = threadIdx.x; k < bins; k += blockDim.x) counts[(size_t)k * nblk + slot] = hist[k];
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[(size_t)bins * nblk] = 0;  // the scan's terminal slot
}

// k_glv_radix fused with k_sort_hist for one shared bucket set (windows [0, W) into one set of
// m 2^(c-1) buckets): a block takes `chunk` scalars, i.e. the entries of sort blocks blockIdx.x
// (k1 terms, entries i) and n / chunk + blockIdx.x (k2 terms, entries n + i), and writes both
// blocks' coarse-bin counts where k_sort_hist would (n % chunk == 0). Saves the hist pass's
// re-read of the W x 2n digits and one launch. Several sets (several MSMs over one table): one
// launch per set, its coarse bins at [bin0, bin0 + NBC) of bins_total.
template <class Fr, uint32_t MUL, int C0>
__global__ void __launch_bounds__(1024) k_glv_radix_hist(const uint32_t* __restrict__ sc,
                                                        const uint8_t* __restrict__ inf, uint32_t n, int mont,
                                                        GlvK K, int W, int32_t* __restrict__ dig, uint32_t FB,
                                                        uint32_t NBC, uint32_t nblk, uint32_t chunk,
                                                        uint32_t* __restrict__ counts, uint32_t bin0,
                                                        uint32_t bins_total) {
    extern __shared__ uint32_t hist[];  // [2][NBC]: k1 block, k2 block
    for (uint32_t k = threadIdx.x; k < 2 * NBC; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    const size_t nv = 2 * (size_t)n;
    const uint32_t lo = blockIdx.x * chunk, hi = lo + chunk;
    // a thread's scalars are loaded up front, PRE at a time (the loads of one scalar after the
    // previous one's digits left the waves waiting on memory 52 % of their cycles:
    // profiles/r04/tail_pmc/sq_summary.txt)
    constexpr int PRE = 4;
    for (uint32_t i0 = lo + threadIdx.x; i0 < hi; i0 += PRE * blockDim.x) {
        fe<Fr> f[PRE];
        bool skip[PRE];
#pragma unroll
        for (int k = 0; k < PRE; k++) {
            const uint32_t i = i0 + (uint32_t)k * blockDim.x;
            skip[k] = i >= hi || (inf != nullptr && inf[i]);
            f[k] = i < hi ? load_scalar<Fr>(sc, i) : fe_zero<Fr>();
        }
        // unrolled (no break): f[k] / skip[k] stay in registers -- a rolled loop indexed them
        // dynamically, i.e. through scratch memory
#pragma unroll
        for (int k = 0; k < PRE; k++) {
            const uint32_t i = i0 + (uint32_t)k * blockDim.x;
            if (i >= hi) continue;
            if (skip[k]) {
                for (int w = 0; w < W; w++) dig[(size_t)w * nv + i] = dig[(size_t)w * nv + n + i] = 0;
                continue;
            }
            if (mont) f[k] = fe_from_mont<Fr>(f[k]);
            uint64_t s[4];
#pragma unroll
            for (int j = 0; j < 4; j++) s[j] = (uint64_t)f[k].v[2 * j] | ((uint64_t)f[k].v[2 * j + 1] << 32);
            u128 rem, q;
            bool nr, nq;
            glv_decompose(s, K, rem, nr, q, nq);
            radix_digits<MUL, C0>(rem, nr, W, [&](int w, int32_t d) {
                dig[(size_t)w * nv + i] = d;
                if (d != 0) atomicAdd(&hist[((uint32_t)(d < 0 ? -d : d) - 1) >> FB], 1u);
            });
            radix_digits<MUL, C0>(q, nq, W, [&](int w, int32_t d) {
                dig[(size_t)w * nv + n + i] = d;
                if (d != 0) atomicAdd(&hist[NBC + (((uint32_t)(d < 0 ? -d : d) - 1) >> FB)], 1u);
            });
        }
    }
    __syncthreads();
    const uint32_t s1 = sort_slot(blockIdx.x, nblk), s2 = sort_slot(blockIdx.x + n / chunk, nblk);
    for (uint32_t k = threadIdx.x; k < NBC; k += blockDim.x) {
        counts[(size_t)(bin0 + k) * nblk + s1] = hist[k];
        counts[(size_t)(bin0 + k) * nblk + s2] = hist[NBC + k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[(size_t)bins_total * nblk] = 0;  // the scan's terminal slot
}

// Coarse entries: u64 = fine << 32 | e | sign << 31, or -- when e < 2^(31 - FB), e.g. the
// shared-window 2^20 MSM (e < 2^24, FB = 5) -- u32 = fine << (31 - FB) | e | sign << 31, which
// halves the scatter's and the fine pass's traffic.
template <class T>
__device__ __forceinline__ T sort_pack(uint32_t fine, uint32_t e, bool neg, uint32_t FB) {
    if constexpr (sizeof(T) == 8) return ((uint64_t)fine << 32) | e | (neg ? 0x80000000u : 0u);
    else return (fine << (31 - FB)) | e | (neg ? 0x80000000u : 0u);
}
template <class T>
__device__ __forceinline__ uint32_t sort_fine_of(T x, uint32_t FB) {
    if constexpr (sizeof(T) == 8) return (uint32_t)(x >> 32);
    else return (x & 0x7fffffffu) >> (31 - FB);
}
template <class T>
__device__ __forceinline__ uint32_t sort_entry_of(T x, uint32_t FB) {
    if constexpr (sizeof(T) == 8) return (uint32_t)x;
    else return x & (0x80000000u | ((1u << (31 - FB)) - 1));
}

template <class Src, class T>
__global__ void __launch_bounds__(1024) k_sort_coarse(Src src, uint32_t n, int c, int wb, int we, uint32_t FB,
                                                     uint32_t NBC, uint32_t nblk, uint32_t stride, uint32_t wps,
                                                     uint32_t chunk, const uint32_t* __restrict__ base,
                                                     T* __restrict__ tmp) {
    extern __shared__ uint32_t cur[];
    const uint32_t bins = (stride ? ((uint32_t)we + wps - 1) / wps : (uint32_t)(we - wb)) * NBC;
    const uint32_t slot = sort_slot(blockIdx.x, nblk);
    for (uint32_t k = threadIdx.x; k < bins; k += blockDim.x) cur[k] = base[(size_t)k * nblk + slot];
    __syncthreads();
    const uint32_t fmask = (1u << FB) - 1;
    const uint32_t lo = blockIdx.x * chunk, hi = min(lo + chunk, n);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        src(i, c, we, [&](int w, int32_t d) {
            if (d != 0 && w >= wb) {
                uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1;
                uint32_t pos = atomicAdd(&cur[(stride ? (uint32_t)w / wps : (uint32_t)(w - wb)) * NBC + (b >> FB)], 1u);
                const uint32_t e = stride ? src.pt(i) + ((uint32_t)w % wps) * stride : i;
                tmp[pos] = sort_pack<T>(b & fmask, e, d < 0, FB);
            }
        });
    }
}

// Staged coarse scatter over precomputed radix digits (RadixDigits, narrow entries): the block's
// entries are counting-sorted by coarse bin in LDS (local offsets from its own per-bin counts,
// written by k_sort_hist), then every bin's run is written in one burst by one wave. The direct
// scatter wrote each run one 4-B entry at a time over the block's whole life; with 1280 bins x 32
// blocks per XCD of open runs the partly written lines left L2 repeatedly (PMC WRITE_SIZE ~6x
// the entries). LDS: 2 bins + 1 + chunk * we words (<= 160 KB: chunk 4096 at 7 windows).
template <class Src>
__global__ void __launch_bounds__(1024) k_sort_coarse_st(Src src, uint32_t n, int c, int wb, int we, uint32_t FB,
                                                        uint32_t NBC, uint32_t nblk, uint32_t stride, uint32_t wps,
                                                        uint32_t chunk, const uint32_t* __restrict__ counts,
                                                        const uint32_t* __restrict__ base,
                                                        uint32_t* __restrict__ tmp, uint32_t bin0, uint32_t bins) {
    extern __shared__ uint32_t sm[];
    __shared__ uint32_t part[1024];
    // this launch's coarse bins [bin0, bin0 + bins): all of them, or one bucket set's (windows
    // [wb, we) of a several-set sort, one launch per set so a block's entries fit LDS)
    uint32_t* loff = sm;             // bins + 1 local run starts
    uint32_t* lcur = sm + bins + 1;  // bins cursors
    uint32_t* stage = lcur + bins;   // the block's entries, bin-major
    const uint32_t t = threadIdx.x, slot = sort_slot(blockIdx.x, nblk);
    // local exclusive scan of the block's per-bin counts: ceil(bins / 1024) bins per thread
    const uint32_t per = (bins + blockDim.x - 1) / blockDim.x, b0 = t * per;
    uint32_t s = 0;
    for (uint32_t k = 0; k < per; k++)
        if (b0 + k < bins) s += counts[(size_t)(bin0 + b0 + k) * nblk + slot];
    part[t] = s;
    __syncthreads();
    for (uint32_t o = 1; o < blockDim.x; o <<= 1) {
        const uint32_t a = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += a;
        __syncthreads();
    }
    uint32_t run = part[t] - s;  // exclusive prefix of this thread's first bin
    for (uint32_t k = 0; k < per; k++)
        if (b0 + k < bins) {
            loff[b0 + k] = run;
            lcur[b0 + k] = run;
            run += counts[(size_t)(bin0 + b0 + k) * nblk + slot];
        }
    if (t == blockDim.x - 1) loff[bins] = part[t];
    __syncthreads();
    const uint32_t fmask = (1u << FB) - 1;
    const uint32_t lo = blockIdx.x * chunk, hi = min(lo + chunk, n);
    auto put = [&](uint32_t i, int w, int32_t d) {
        if (d != 0 && w >= wb) {
            const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1;
            const uint32_t p = atomicAdd(
                &lcur[(stride ? (uint32_t)w / wps : (uint32_t)(w - wb)) * NBC + (b >> FB) - bin0], 1u);
            stage[p] = sort_pack<uint32_t>(b & fmask, stride ? src.pt(i) + ((uint32_t)w % wps) * stride : i, d < 0, FB);
        }
    };
    if constexpr (std::is_same<Src, RadixDigits>::value) {
        // radix digits: the digits of PRE iterations (<= 8 windows each) loaded before their LDS
        // atomics (one load, one atomic at a time left the waves waiting on memory 71 % of their
        // cycles: profiles/r04/tail_pmc/sq_summary.txt)
        constexpr int PRE = 4, WMAX = 8;
        if (we - src.w0 <= WMAX) {
            for (uint32_t i0 = lo + t; i0 < hi; i0 += PRE * blockDim.x) {
                int32_t dg[PRE][WMAX];
#pragma unroll
                for (int k = 0; k < PRE; k++) {
                    const uint32_t i = i0 + (uint32_t)k * blockDim.x;
#pragma unroll
                    for (int j = 0; j < WMAX; j++)
                        dg[k][j] = (i < hi && src.w0 + j < we) ? src.dig[(size_t)(src.w0 + j) * src.nv + i] : 0;
                }
#pragma unroll
                for (int k = 0; k < PRE; k++) {
                    const uint32_t i = i0 + (uint32_t)k * blockDim.x;
                    if (i >= hi) break;
#pragma unroll
                    for (int j = 0; j < WMAX; j++)
                        if (src.w0 + j < we) put(i, src.w0 + j, dg[k][j]);
                }
            }
        } else {
            for (uint32_t i = lo + t; i < hi; i += blockDim.x) src(i, c, we, [&](int w, int32_t d) { put(i, w, d); });
        }
    } else {
        for (uint32_t i = lo + t; i < hi; i += blockDim.x) src(i, c, we, [&](int w, int32_t d) { put(i, w, d); });
    }
    __syncthreads();
    // every bin's run in one burst: 16 lanes per bin (runs are ~10-25 entries: a whole wave per bin
    // left most lanes idle), 4 bins per wave at a time
    const uint32_t grp = t >> 4, sub = t & 15, ngrp = blockDim.x >> 4;
    for (uint32_t g = grp; g < bins; g += ngrp) {
        const uint32_t l0 = loff[g], len = loff[g + 1] - l0;
        const uint32_t gb = base[(size_t)(bin0 + g) * nblk + slot];
        for (uint32_t j = sub; j < len; j += 16) tmp[gb + j] = stage[l0 + j];
    }
}

// one block per coarse bin; offsets[g * 2^FB + f] = start of fine bucket f of bin g. Block 0
// also clears the accumulate's chain_max word (no separate memset in the pipeline). Blocks of
// 256 or 1024 threads (large bins): the 256 fine counters are scanned by the first 256.
// starts != nullptr: the block also writes the start records of the accumulate threads (M sorted
// entries each) whose first entry lies in its bin.
// cap > 0: a bin of at most cap entries is scattered into LDS (dynamic, cap words) and written
// out in one coalesced pass -- the direct scatter wrote each bucket's 4-B entries one at a time
// over the block's life, and the partly written lines left L2 several times (PMC WRITE_SIZE
// ~4x the entries); larger bins scatter directly.
template <class T>
__global__ void __launch_bounds__(1024) k_sort_fine(const T* __restrict__ tmp, const uint32_t* __restrict__ base,
                                                   uint32_t nblk, uint32_t bins, uint32_t FB,
                                                   uint32_t* __restrict__ offsets, uint32_t* __restrict__ sorted,
                                                   uint32_t* __restrict__ zero_word, uint32_t cap,
                                                   AccStart* __restrict__ starts, uint32_t M) {
    __shared__ uint32_t h[256], x[256];
    extern __shared__ uint32_t stage[];
    const uint32_t g = blockIdx.x, F = 1u << FB, t = threadIdx.x;
    const bool cnt_lane = t < 256;
    if (zero_word != nullptr && g == 0 && t == 0) *zero_word = 0;
    const uint32_t start = base[(size_t)g * nblk];
    const uint32_t end = base[(size_t)(g + 1) * nblk];  // base has bins*nblk + 1 entries
    if (cnt_lane) h[t] = 0;
    __syncthreads();
    // a staged bin of at most RMAX entries per thread keeps its entries in registers from the
    // counting pass to the scatter: the bin is read from HBM once, not twice (uniform per block)
    constexpr uint32_t RMAX = 16;
    T er[RMAX];
    const bool regs = cap != 0 && end - start <= cap && end - start <= RMAX * blockDim.x;
    if (regs) {
#pragma unroll
        for (uint32_t k = 0; k < RMAX; k++) {
            const uint32_t p = start + t + k * blockDim.x;
            er[k] = p < end ? tmp[p] : T(0);
        }
#pragma unroll
        for (uint32_t k = 0; k < RMAX; k++)
            if (start + t + k * blockDim.x < end) atomicAdd(&h[sort_fine_of<T>(er[k], FB)], 1u);
    } else {  // RH loads in flight per thread before their counter atomics
        constexpr uint32_t RH = 4;
        for (uint32_t p0 = start + t; p0 < end; p0 += RH * blockDim.x) {
            T e[RH];
#pragma unroll
            for (uint32_t k = 0; k < RH; k++) {
                const uint32_t p = p0 + k * blockDim.x;
                e[k] = p < end ? tmp[p] : T(0);
            }
#pragma unroll
            for (uint32_t k = 0; k < RH; k++)
                if (p0 + k * blockDim.x < end) atomicAdd(&h[sort_fine_of<T>(e[k], FB)], 1u);
        }
    }
    __syncthreads();
    // inclusive Hillis-Steele scan over 256 counters
    const uint32_t v = cnt_lane ? h[t] : 0u;
    if (cnt_lane) x[t] = v;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint32_t a = (cnt_lane && t >= o) ? x[t - o] : 0u;
        __syncthreads();
        if (cnt_lane) x[t] += a;
        __syncthreads();
    }
    const uint32_t excl = cnt_lane ? x[t] - v : 0u;
    if (t < F) offsets[(size_t)g * F + t] = start + excl;
    if (g == bins - 1 && t == 0) offsets[(size_t)bins * F] = end;
    // start records (AccStart) of the accumulate threads u whose first entry u M lies in this bin:
    // their bucket is the first fine bucket whose inclusive count passes u M - start (so never an
    // empty one), searched in the LDS scan -- a thread per record, whether one bucket holds many
    // thread starts (equal scalars) or runs of empty buckets lie between two of them
    if (starts != nullptr) {
        for (uint64_t u = ((uint64_t)start + M - 1) / M + t; u * M < end; u += blockDim.x) {
            const uint32_t rel = (uint32_t)(u * M) - start;
            uint32_t lo = 0, hi = F - 1;  // x[F - 1] = end - start > rel
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (x[mid] > rel) hi = mid;
                else lo = mid + 1;
            }
            AccStart r;
            r.b = g * F + lo;
            r.begin = start + (lo ? x[lo - 1] : 0u);
            r.end = start + x[lo];
            r.next_end = lo + 1 < F ? start + x[lo + 1] : 0u;
            starts[u] = r;
        }
        // the sentinel: thread T = ceil(L / M), the first one that does not run
        if (g == bins - 1 && t == 0) starts[((uint64_t)end + M - 1) / M] = AccStart{bins * F, end, end, 0u};
    }
    __syncthreads();
    if (cnt_lane) h[t] = excl;  // cursors
    __syncthreads();
    // the scatter RS entries at a time (loads, then LDS cursor atomics, then stores: RS atomics in
    // flight per thread)
    constexpr uint32_t RS = 4;
    if (regs) {
#pragma unroll
        for (uint32_t k = 0; k < RMAX; k++)
            if (start + t + k * blockDim.x < end) stage[atomicAdd(&h[sort_fine_of<T>(er[k], FB)], 1u)] = sort_entry_of<T>(er[k], FB);
        __syncthreads();
        for (uint32_t p = t; p < end - start; p += blockDim.x) sorted[start + p] = stage[p];
        return;
    }
    if (end - start <= cap) {  // uniform over the block
        for (uint32_t p0 = start + t; p0 < end; p0 += RS * blockDim.x) {
            T e[RS];
            uint32_t pos[RS];
#pragma unroll
            for (uint32_t k = 0; k < RS; k++) {
                const uint32_t p = p0 + k * blockDim.x;
                e[k] = p < end ? tmp[p] : T(0);
            }
#pragma unroll
            for (uint32_t k = 0; k < RS; k++)
                if (p0 + k * blockDim.x < end) pos[k] = atomicAdd(&h[sort_fine_of<T>(e[k], FB)], 1u);
#pragma unroll
            for (uint32_t k = 0; k < RS; k++)
                if (p0 + k * blockDim.x < end) stage[pos[k]] = sort_entry_of<T>(e[k], FB);
        }
        __syncthreads();
        for (uint32_t p = t; p < end - start; p += blockDim.x) sorted[start + p] = stage[p];
        return;
    }
    for (uint32_t p0 = start + t; p0 < end; p0 += RS * blockDim.x) {
        T e[RS];
        uint32_t pos[RS];
#pragma unroll
        for (uint32_t k = 0; k < RS; k++) {
            const uint32_t p = p0 + k * blockDim.x;
            e[k] = p < end ? tmp[p] : T(0);
        }
#pragma unroll
        for (uint32_t k = 0; k < RS; k++)
            if (p0 + k * blockDim.x < end) pos[k] = start + atomicAdd(&h[sort_fine_of<T>(e[k], FB)], 1u);
#pragma unroll
        for (uint32_t k = 0; k < RS; k++)
            if (p0 + k * blockDim.x < end) sorted[pos[k]] = sort_entry_of<T>(e[k], FB);
    }
}

// hipFuncAttributeMaxDynamicSharedMemorySize is per device: set it once per (kernel, device), so
// a process driving several GPUs (one vc_ctx each, or a vc_group) has it on every device it launches on
static int coarse_st_lds_attr(const void* fn, int device) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({fn, device})) return VC_OK;
    VK_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    done.insert({fn, device});
    return VC_OK;
}

template <class Src>
static int sort_entries(vc_ctx* ctx, Lane L, Src src, uint32_t nv, int c, int wb, int we, uint32_t FB,
                        uint32_t NBC, uint32_t nblk, uint32_t chunk, uint32_t stride, uint32_t wps, size_t ncnt,
                        uint32_t* counts, uint32_t* base, void* tmp, uint32_t* offsets, uint32_t* sorted,
                        uint32_t* zero_word, AccStart* starts, uint32_t M, bool coarse_stage = false,
                        bool counts_ready = false, uint32_t sets_split = 1) {
    hipStream_t st = L.st;
    if (stride && wps == 0) return VC_E_INVALID;
    const uint32_t bins = (stride ? ((uint32_t)we + wps - 1) / wps : (uint32_t)(we - wb)) * NBC;
    const size_t lds = (size_t)bins * 4;
    if (lds > 64 * 1024) return VC_E_INVALID;  // c <= 16 keeps bins <= W * 128
    if (ncnt != (size_t)bins * nblk + 1) return VC_E_INVALID;
    // largest entry index e: i < nv, or w * stride + i with shared windows
    const uint64_t emax = stride ? (uint64_t)std::min<uint32_t>((uint32_t)we, wps) * stride : (uint64_t)nv;
    const bool narrow = emax <= (1ull << (31 - FB));
    // scalars per hist / coarse block: runs of a block inside a coarse bin are chunk * W / bins
    // entries long, so a big bucket set (many coarse bins) takes bigger blocks to keep the
    // scatter's runs near a cache line
    const uint32_t sblk = chunk >= 4096 ? 1024 : 256;
    if (!counts_ready)  // else written by k_glv_radix_hist
        VK_LAUNCH_ON(ctx, st, "msm_sort_hist", (k_sort_hist<Src>), nblk, sblk, lds, src, nv, c, wb, we, FB, NBC,
                     nblk, stride, wps, chunk, counts);
    size_t tmp_bytes = 0;
    VK_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, counts, base, ncnt, st));
    VK_TRY(L.ws[WS_SCAN_TMP].ensure(tmp_bytes));
    {
        hipEvent_t ev = nullptr;
        if (ctx->timing) ctx->timer_begin("msm_scan", &ev, st);
        VK_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(L.ws[WS_SCAN_TMP].p, tmp_bytes, counts, base, ncnt, st));
        if (ctx->timing) ctx->timer_end("msm_scan", ev, st);
    }
    // fine-pass block: 1024 threads once bins average >= 2^15 entries (one block per bin)
    const uint64_t total = (uint64_t)nv * (uint32_t)(we - wb);
    int fblk = total / bins >= (1u << 15) ? 1024 : 256;
    // LDS staging of the fine scatter (16K entries, 64 KB: two blocks per CU, 1024 threads) when the
    // mean bin leaves it ~40 % headroom (radix 2^20: 11.5K); a bin beyond it scatters directly
    // (staged bins of <= 16 entries per thread keep their entries in registers, k_sort_fine)
    uint32_t cap = 0;
    if (total / bins <= 12000) {
        cap = 16384;
        fblk = 1024;
    }
    // staged coarse scatter (k_sort_coarse_st): narrow entries, the block's entries in LDS; with
    // several shared bucket sets (windows [s wps, (s + 1) wps) -> set s) one launch per set, so a
    // block holds one set's chunk x wps entries (the KZG commit + open's two sets keep 4096-scalar
    // blocks, as one set does)
    const uint32_t nsplit = (stride && sets_split > 1 && wb == 0 && (uint32_t)we == sets_split * wps) ? sets_split : 1;
    const uint32_t bins_l = bins / nsplit;
    const uint32_t wl = (uint32_t)(we - wb) / nsplit;
    const size_t st_lds = ((size_t)2 * bins_l + 1 + (size_t)chunk * wl) * 4;
    const bool staged = coarse_stage && narrow && st_lds <= 152 * 1024;
    if (staged) {
        VK_TRY(coarse_st_lds_attr(reinterpret_cast<const void*>(&k_sort_coarse_st<Src>), ctx->device));
        for (uint32_t s = 0; s < nsplit; s++) {
            Src ss = src;
            const int wbs = nsplit > 1 ? (int)(s * wps) : wb, wes = nsplit > 1 ? (int)((s + 1) * wps) : we;
            if constexpr (std::is_same<Src, RadixDigits>::value) ss.w0 = wbs;
            VK_LAUNCH_ON(ctx, st, "msm_sort_coarse", k_sort_coarse_st<Src>, nblk, 1024, st_lds, ss, nv, c, wbs, wes, FB,
                         NBC, nblk, stride, wps, chunk, counts, base, static_cast<uint32_t*>(tmp), s * bins_l, bins_l);
        }
        VK_LAUNCH_ON(ctx, st, "msm_sort_fine", k_sort_fine<uint32_t>, bins, fblk, cap * 4,
                     static_cast<const uint32_t*>(tmp), base, nblk, bins, FB, offsets, sorted, zero_word, cap,
                     starts, M);
    } else if (narrow) {
        VK_LAUNCH_ON(ctx, st, "msm_sort_coarse", (k_sort_coarse<Src, uint32_t>), nblk, sblk, lds, src, nv, c, wb, we,
                     FB, NBC, nblk, stride, wps, chunk, base, static_cast<uint32_t*>(tmp));
        VK_LAUNCH_ON(ctx, st, "msm_sort_fine", k_sort_fine<uint32_t>, bins, fblk, cap * 4,
                     static_cast<const uint32_t*>(tmp), base, nblk, bins, FB, offsets, sorted, zero_word, cap,
                     starts, M);
    } else {
        VK_LAUNCH_ON(ctx, st, "msm_sort_coarse", (k_sort_coarse<Src, uint64_t>), nblk, sblk, lds, src, nv, c, wb, we,
                     FB, NBC, nblk, stride, wps, chunk, base, static_cast<uint64_t*>(tmp));
        VK_LAUNCH_ON(ctx, st, "msm_sort_fine", k_sort_fine<uint64_t>, bins, fblk, cap * 4,
                     static_cast<const uint64_t*>(tmp), base, nblk, bins, FB, offsets, sorted, zero_word, cap,
                     starts, M);
    }
    return VC_OK;
}
}  // namespace vk

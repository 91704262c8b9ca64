// Sparse batched commits over the fixed-base tables (the verkle tree's levels; declared in ctx.hpp).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>
#include "host/pool.hpp"
#include "msm_accumulate.hpp"  // msm_tail.hpp: ctx.hpp, ec.hpp, ec29.hpp
#include "msm_digits.hpp"  // load_scalar

namespace vk {
// Rows of a CSR matrix (row g = commit g: non-zero (column i, scalar s) pairs) against the
// fixed-base window tables of a table: every non-zero expands to its non-zero signed window
// digits, each a table point T[i][w][|d|-1] -- so the entries of a row are contiguous and the
// rows play the buckets of the Pippenger accumulate: the same balanced k_msm_accumulate (M
// entries per thread, rows straddling threads merged by the fix-up) sums them. For verkle
// nodes (~5 non-zeros of 256 per internal node, 2 of N per extension row) this replaces
// dense width-256 rows.
// the signed digits of a scalar over a fixed-base table's windows (widths g.width(w), ctx.hpp)
template <class Fr, class Fn>
__device__ __forceinline__ void for_each_digit_fb(fe<Fr> s, const FbGeom& g, Fn&& f) {
    uint32_t carry = 0;
    for (int w = 0; w < g.W; w++) {
        const int c = g.width(w);
        const uint32_t raw = (s.v[0] & ((1u << c) - 1)) + carry;
#pragma unroll
        for (int k = 0; k < 7; k++) s.v[k] = (s.v[k] >> c) | (s.v[k + 1] << (32 - c));
        s.v[7] >>= c;
        carry = raw > (1u << (c - 1)) ? 1u : 0u;
        f(w, carry ? (int32_t)raw - (int32_t)(1u << c) : (int32_t)raw);
    }
}

template <class Fr>
__global__ void k_sparse_count(const uint32_t* __restrict__ sc, size_t nnz, int mont, FbGeom g,
                               uint32_t* __restrict__ cnt) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nnz) return;
    fe<Fr> s = load_scalar<Fr>(sc, j);
    if (mont) s = fe_from_mont<Fr>(s);
    uint32_t k = 0;
    for_each_digit_fb<Fr>(s, g, [&](int, int32_t d) { k += d != 0; });
    cnt[j] = k;
}

template <class Fr>
__global__ void k_sparse_expand(const uint32_t* __restrict__ sc, const uint32_t* __restrict__ cols, size_t nnz,
                                int mont, FbGeom g, const uint32_t* __restrict__ eoff,
                                uint32_t* __restrict__ entries) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nnz) return;
    fe<Fr> s = load_scalar<Fr>(sc, j);
    if (mont) s = fe_from_mont<Fr>(s);
    const uint32_t base = cols[j] * (uint32_t)g.stride();
    uint32_t pos = eoff[j];
    for_each_digit_fb<Fr>(s, g, [&](int w, int32_t d) {
        if (d != 0)
            entries[pos++] = (base + (uint32_t)g.off(w) + (uint32_t)(d < 0 ? -d : d) - 1) | (d < 0 ? 0x80000000u : 0u);
    });
}

// Fused form of count + scan + expand + rows (round 6): two launches instead of six (the hipcub
// scan's two, the count, the expand, the row offsets and a fill) -- each tiny launch costs ~4.5 us
// of GPU time even when the host is ahead (profiles/r06/verkle/norm_early/timeline_full_and_update.txt).
// K1: elements [256 b, 256 b + 256) of block b (j <= nnz: the grid has nnz / 256 + 1 blocks, so
// j = nnz is always some block's element, with count 0) -> local[j] = the exclusive count prefix
// inside the block, bsum[b] = its total; the last block to arrive scans the block totals into
// boff[0 .. nb] (boff[nb] = all entries) and resets the arrival counter for the next launch.
__device__ __forceinline__ uint32_t block_excl_scan256(uint32_t v, uint32_t* s_w, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t k = 0; k < wv; k++) before += s_w[k];
    *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return before + x - v;
}
template <class Fr>
__global__ void __launch_bounds__(256) k_sparse_count_scan(const uint32_t* __restrict__ sc, size_t nnz, int mont,
                                                          FbGeom g, uint32_t* __restrict__ local,
                                                          uint64_t* __restrict__ bsum, uint32_t* __restrict__ boff,
                                                          uint32_t* __restrict__ counter, uint32_t* __restrict__ chain_max,
                                                          uint32_t epoch) {
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_last;
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t k = 0;
    if (j < nnz) {
        fe<Fr> s = load_scalar<Fr>(sc, j);
        if (mont) s = fe_from_mont<Fr>(s);
        for_each_digit_fb<Fr>(s, g, [&](int, int32_t d) { k += d != 0; });
    }
    uint32_t tot;
    const uint32_t ex = block_excl_scan256(k, s_w, &tot);
    if (j <= nnz) local[j] = ex;
    if (chain_max && blockIdx.x == 0 && threadIdx.x == 0) *chain_max = 0;
    const uint32_t nb = gridDim.x;
    const uint64_t tag = (uint64_t)epoch << 32;
    // the block total as one (epoch << 32 | total) word and no fence before the arrival: the last
    // block polls the words until they carry this launch's epoch (a fence per block writes back its
    // XCD's whole L2: ~28 us for the 1,025 blocks of a 262,144-non-zero level)
    if (threadIdx.x == 0) {
        __hip_atomic_store(&bsum[blockIdx.x], tag | tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = atomicAdd(counter, 1u) == nb - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    auto total_of = [&](uint32_t b) -> uint32_t {  // (bounded: 10 ms)
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            const uint64_t w = __hip_atomic_load(&bsum[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((w & 0xffffffff00000000ull) == tag || __builtin_amdgcn_s_memrealtime() - t0 > 1000000ull)
                return (uint32_t)w;
        }
    };
    // the last block: exclusive scan of the nb block totals, ceil(nb / 256) consecutive per thread
    // (the loads of a thread's totals go out together: one after another they cost ~1-2 us each,
    // 30 us for the 1,025 blocks of a 262,144-non-zero level)
    const uint32_t per = (nb + 255) / 256, b0 = min(threadIdx.x * per, nb), b1 = min(b0 + per, nb);
    constexpr uint32_t PR = 8;
    uint32_t v[PR];
    uint32_t seg = 0;
    if (per <= PR) {
#pragma unroll
        for (uint32_t q = 0; q < PR; q++) v[q] = b0 + q < b1 ? total_of(b0 + q) : 0u;
#pragma unroll
        for (uint32_t q = 0; q < PR; q++) seg += v[q];
    } else {
        for (uint32_t b = b0; b < b1; b++) seg += total_of(b);
    }
    uint32_t all;
    uint32_t run = block_excl_scan256(seg, s_w, &all);
    if (per <= PR) {
#pragma unroll
        for (uint32_t q = 0; q < PR; q++) {
            if (b0 + q < b1) boff[b0 + q] = run;
            run += v[q];
        }
    } else {
        for (uint32_t b = b0; b < b1; b++) {
            boff[b] = run;
            run += total_of(b);
        }
    }
    if (threadIdx.x == 0) {
        boff[nb] = all;
        *counter = 0;  // for the next launch (stream-ordered after this one)
    }
}
// K2: thread i < nnz expands element i's digits at boff[i / 256] + local[i]; thread i <= nch sets
// chunk i's entry offset (rp[i] is an element index <= nnz) and, for an empty chunk, its identity
template <class Fr, class C>
__global__ void __launch_bounds__(256) k_sparse_expand_rows(const uint32_t* __restrict__ sc,
                                                           const uint32_t* __restrict__ cols, size_t nnz, int mont,
                                                           FbGeom g, const uint32_t* __restrict__ local,
                                                           const uint32_t* __restrict__ boff,
                                                           uint32_t* __restrict__ entries,
                                                           const uint64_t* __restrict__ rp, size_t nch,
                                                           uint32_t* __restrict__ offsets,
                                                           typename C::Acc* __restrict__ chunks) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nnz) {
        fe<Fr> s = load_scalar<Fr>(sc, i);
        if (mont) s = fe_from_mont<Fr>(s);
        const uint32_t base = cols[i] * (uint32_t)g.stride();
        uint32_t pos = boff[i >> 8] + local[i];
        for_each_digit_fb<Fr>(s, g, [&](int w, int32_t d) {
            if (d != 0)
                entries[pos++] = (base + (uint32_t)g.off(w) + (uint32_t)(d < 0 ? -d : d) - 1) | (d < 0 ? 0x80000000u : 0u);
        });
    }
    if (i <= nch) {
        auto at = [&](uint64_t e) { return boff[e >> 8] + local[e]; };
        const uint32_t o = at(rp[i]);
        offsets[i] = o;
        if (i < nch && at(rp[i + 1]) == o) chunks[i] = C::zero();
    }
}

// row offsets in entry space; empty rows get the identity (the accumulate never writes them)
template <class C>
__global__ void k_sparse_rows(const uint64_t* __restrict__ row_ptr, const uint32_t* __restrict__ eoff, size_t batch,
                              uint32_t* __restrict__ offsets, typename C::Acc* __restrict__ rows) {
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > batch) return;
    offsets[g] = eoff[row_ptr[g]];
    if (g < batch && eoff[row_ptr[g + 1]] == eoff[row_ptr[g]]) rows[g] = C::zero();
}

// row g = sum of its chunks [rc[g], rc[g+1]) -- one wave per row: lanes load chunk sums (a
// strided loop when a row has more than 64), then an xor butterfly over the used lanes
template <class C>
__global__ void __launch_bounds__(64) k_sparse_combine(const typename C::Acc* __restrict__ chunks,
                                                      const uint32_t* __restrict__ rc, typename C::Acc* __restrict__ rows) {
    using Acc = typename C::Acc;
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    const uint32_t b = rc[g], n = rc[g + 1] - b;
    if (n == 1) {  // uniform per wave
        if (lane == 0) rows[g] = chunks[b];
        return;
    }
    uint32_t span = 1, lg = 0;
    while (span < n && span < 64) {
        span <<= 1;
        lg++;
    }
    const uint32_t nk = (n + 63) / 64;
    Acc v = C::zero();
    for (uint32_t it = 0; it < nk + lg; it++) {  // one add call site (see msm_tail.hip)
        Acc o;
        if (it < nk) {
            const uint32_t k = lane + it * 64;
            o = k < n ? chunks[b + k] : C::zero();
        } else {
            const uint32_t m = 1u << (it - nk);
            const uint32_t* src = reinterpret_cast<const uint32_t*>(&v);
            uint32_t* dst = reinterpret_cast<uint32_t*>(&o);
#pragma unroll
            for (int k = 0; k < C::ACC_WORDS; k++) dst[k] = __shfl_xor(src[k], m, 64);
        }
        v = C::add(v, o);
    }
    if (lane == 0) rows[g] = v;
}

// Chunk lists of a CSR row structure (host): rows are cut into chunks of <= CHNZ non-zeros (the
// accumulate's buckets), so a long row (e.g. a verkle root: 256 children x W windows) does not
// become one bucket straddling hundreds of threads -- whose pieces the fix-up would add serially;
// chunk sums are folded per row by k_sparse_combine. rc[g] = first chunk of row g (an empty row
// gets one empty chunk), cptr = chunk ends. When every row has 1..CHNZ non-zeros the chunks are
// the rows (identity: rc = 0..batch, cptr = row_ptr; nothing is built).
constexpr size_t SPARSE_CHNZ = 4;
struct SparseChunks {
    const uint32_t* rc = nullptr;    // row g's chunks are [rc[g], rc[g + 1])
    const uint64_t* cptr = nullptr;  // chunk k's non-zeros are [cptr[k], cptr[k + 1])
    size_t nch = 0;
    bool identity = false;
};
// The chunk lists in one serial pass, straight into page-locked staging (one upload each): the two
// pooled passes into fresh vectors they replace cost ~0.1 ms of idle GPU on a 17k-row verkle level
// (the pool's wake-ups and page faults; profiles/r05/verkle/sparse_norm_vk/). The previous call's
// uploads from the staging have completed: every sparse commit ends in a normalisation that saw its
// first kernel finish (or waited for the stream).
static int sparse_chunks(vc_ctx* ctx, const uint64_t* row_ptr, size_t batch, bool rows_fit, SparseChunks* out) {
    const size_t CHNZ = SPARSE_CHNZ;
    if (rows_fit) {  // the caller knows every row has 1..CHNZ non-zeros
        out->identity = true;
        out->nch = batch;
        return VC_OK;
    }
    // max(1, ceil(len / CHNZ)) <= 1 + floor(len / CHNZ) chunks per row
    const size_t cap = batch + row_ptr[batch] / CHNZ;
    VK_TRY(ctx->pin_sparse_ch.ensure((cap + 1) * 8 + (batch + 1) * 4));
    uint64_t* cptr = ctx->pin_sparse_ch.as<uint64_t>();
    uint32_t* rc = reinterpret_cast<uint32_t*>(cptr + cap + 1);
    size_t run = 0;
    cptr[0] = 0;
    for (size_t g = 0; g < batch; g++) {
        rc[g] = (uint32_t)run;
        const uint64_t lo = row_ptr[g], hi = row_ptr[g + 1];
        if (lo == hi) {  // an empty row is one empty chunk (the identity)
            cptr[++run] = lo;
            continue;
        }
        for (uint64_t j = lo; j < hi; j += CHNZ) cptr[++run] = std::min<uint64_t>(j + CHNZ, hi);
    }
    rc[batch] = (uint32_t)run;
    out->rc = rc;
    out->cptr = cptr;
    out->nch = run;
    return VC_OK;
}

// The sparse commit on the device: columns d_cols (u32) and scalars d_sc (4 u64, canonical unless
// mont) already in device memory, the row structure row_ptr on the host (the chunk lists; rows_fit:
// every row has 1..CHNZ non-zeros). Outputs on the device: canonical affine rows d_xy / d_inf and,
// with d_items (BN254), their to_data_item values. Enqueued on ctx->stream; the normalisation's
// host step synchronises it once (normalize_split), nothing else waits.
// row g += the canonical affine point (cxy[id], cinf[id]) of id = add_ids[g] (none: 0xffffffff)
template <class C>
__global__ void k_rows_add_base(typename C::Acc* __restrict__ rows, size_t batch, const uint32_t* __restrict__ add_ids,
                                const uint64_t* __restrict__ cxy, const uint8_t* __restrict__ cinf) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= batch) return;
    const uint32_t id = add_ids[g];
    if (id == 0xffffffffu || cinf[id]) return;
    using F = typename C::F;
    typename C::Aff a;
    memcpy(a.x.v, cxy + (size_t)id * 2 * (F::N / 2), F::N * 4);
    memcpy(a.y.v, cxy + (size_t)id * 2 * (F::N / 2) + F::N / 2, F::N * 4);
    a.x = fe_to_mont<F>(a.x);
    a.y = fe_to_mont<F>(a.y);
    rows[g] = C::madd(rows[g], a, false);
}

template <class C, class Fr>
static int sparse_commit_dev(vc_ctx* ctx, Table* t, size_t batch, const uint64_t* row_ptr, bool rows_fit,
                             const uint32_t* d_cols_in, const void* d_sc_in, int mont, void* d_xy, uint8_t* d_inf,
                             void* d_items, const uint32_t* d_add_ids = nullptr, const uint64_t* d_add_xy = nullptr,
                             const uint8_t* d_add_inf = nullptr, const uint32_t* d_dst = nullptr,
                             const std::function<void()>* overlap = nullptr, const uint64_t* d_row_ptr = nullptr) {
    using Acc = typename C::Acc;
    if (batch == 0) return VC_OK;
    const size_t nnz = row_ptr[batch];
    auto tic = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!verbose()) return;
        (void)hipStreamSynchronize(ctx->stream);
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[sparse %zu rows %zu nnz] %s %.3f ms\n", batch, nnz, what,
                std::chrono::duration<double, std::milli>(now - tic).count());
        tic = now;
    };
    if (t->fb_c == 0) VK_TRY(fixed_base_precompute(ctx, t, 8));
    const FbGeom fg = t->fb_geom();
    const int W = fg.W;
    SparseChunks ch;
    VK_TRY(sparse_chunks(ctx, row_ptr, batch, rows_fit, &ch));
    const size_t nch = ch.nch;
    if ((uint64_t)t->n * fg.stride() >= (1ull << 31)) return VC_E_RANGE;  // entry index + sign bit
    const size_t maxL = nnz * (size_t)W;
    if (maxL >= 0xffffffffull) return VC_E_RANGE;
    hipStream_t st = ctx->stream;
    // grow-only ctx workspaces (the MSM's own slots for entries / carries / scan scratch: the
    // two paths never run concurrently on one ctx)
    DevBuf& d_rp = ctx->ws[WS_SP_RP];
    DevBuf& d_cnt = ctx->ws[WS_SP_CNT];
    DevBuf& d_eoff = ctx->ws[WS_SP_EOFF];
    DevBuf& d_ent = ctx->ws[WS_SORTED];
    DevBuf& d_off = ctx->ws[WS_SP_OFF];
    DevBuf& d_rows = ctx->ws[WS_SP_ROWS];
    DevBuf& d_carry = ctx->ws[WS_CARRY];
    DevBuf& d_thr = ctx->ws[WS_THROUGH];
    DevBuf& d_own = ctx->ws[WS_OWNER];
    DevBuf& d_ownb = ctx->ws[WS_OWNER_B];
    DevBuf& d_tmp = ctx->ws[WS_SCAN_TMP];
    const uint32_t M = msm_entries_per_thread(maxL);
    const uint32_t Tmax = (uint32_t)((maxL + M - 1) / M);
    DevBuf& d_rc = ctx->ws[WS_SP_RC];
    DevBuf& d_chunks = ctx->ws[WS_SP_CHUNKS];
    // chunk lists: cptr and rc lie back to back in the page-locked staging (sparse_chunks), so they
    // go up in one copy into d_rp (rc at the same offset); identity rows use d_rc for their iota
    const size_t rc_off = ch.identity ? 0 : (size_t)(reinterpret_cast<const uint8_t*>(ch.rc) -
                                                     reinterpret_cast<const uint8_t*>(ch.cptr));
    VK_TRY(d_rp.ensure(ch.identity ? (nch + 1) * 8 : rc_off + (batch + 1) * 4));
    VK_TRY(d_rc.ensure((batch + 1) * 4));
    VK_TRY(d_chunks.ensure(nch * sizeof(Acc)));
    VK_TRY(d_cnt.ensure((nnz + 1) * 4));
    VK_TRY(d_eoff.ensure((nnz + 1) * 4));
    VK_TRY(d_ent.ensure(std::max<size_t>(maxL, 1) * 4));
    VK_TRY(d_off.ensure((nch + 1) * 4));
    VK_TRY(d_rows.ensure(batch * sizeof(Acc)));
    VK_TRY(d_carry.ensure((size_t)(Tmax + 8) * sizeof(FAcc<C>)));
    VK_TRY(d_thr.ensure((size_t)(Tmax + 8)));
    VK_TRY(d_own.ensure((size_t)(Tmax + 8) * sizeof(FAcc<C>)));
    VK_TRY(d_ownb.ensure((size_t)(Tmax + 8) * 4));
    lap("host chunk lists");
    // rows as chunks: the row pointers are the chunk pointers -- the caller's device copy when it
    // has one (d_row_ptr: the verkle extension rows upload theirs with the rows, or make them on the
    // device), else one upload
    const uint64_t* rp_dev = d_rp.as<uint64_t>();
    const uint32_t* rc_dev = d_rc.as<uint32_t>();
    if (ch.identity) {  // (no chunk lists: the combine, their only reader, is skipped)
        if (d_row_ptr) rp_dev = d_row_ptr;
        else VK_CHECK_HIP(hipMemcpyAsync(d_rp.p, row_ptr, (batch + 1) * 8, hipMemcpyHostToDevice, st));
    } else {
        VK_CHECK_HIP(hipMemcpyAsync(d_rp.p, ch.cptr, rc_off + (batch + 1) * 4, hipMemcpyHostToDevice, st));
        rc_dev = reinterpret_cast<const uint32_t*>(d_rp.as<uint8_t>() + rc_off);
    }
    const uint32_t* d_cols = d_cols_in;
    const uint32_t* d_sc = static_cast<const uint32_t*>(d_sc_in);
    VK_TRY(ctx->ws[WS_CHAIN].ensure(4));
    uint32_t* chain_max = ctx->ws[WS_CHAIN].as<uint32_t>();
    // VKZG_SPARSE_FUSED=0 (read per call, A/B): the count, the hipcub scan, the expand and the row
    // offsets as separate launches
    const char* fe_env = getenv("VKZG_SPARSE_FUSED");
    const bool fused = !(fe_env && atoi(fe_env) == 0);
    if (fused) {
        // the arrival counter: a word of the normalisation's zeroed counter buffer (normalize.hip)
        DevBuf& cntb = ctx->ws[WS_NORM_CNT];
        if (cntb.p == nullptr) {
            VK_TRY(cntb.ensure(256));
            VK_CHECK_HIP(hipMemsetAsync(cntb.p, 0, 256, st));
        }
        const size_t nb = nnz / 256 + 1;  // elements 0 .. nnz
        VK_TRY(d_eoff.ensure(nb * 8 + (nb + 1) * 4));
        uint64_t* bsum = d_eoff.as<uint64_t>();
        uint32_t* boff = reinterpret_cast<uint32_t*>(bsum + nb);
        const uint32_t epoch = next_epoch(ctx);
        VK_LAUNCH(ctx, "sparse_count_scan", (k_sparse_count_scan<Fr>), (unsigned)nb, 256, 0, d_sc, nnz, mont, fg,
                  d_cnt.as<uint32_t>(), bsum, boff, cntb.as<uint32_t>() + 16, Tmax > 0 ? chain_max : (uint32_t*)nullptr,
                  epoch);
        VK_LAUNCH(ctx, "sparse_expand_rows", (k_sparse_expand_rows<Fr, C>), (unsigned)((std::max(nnz, nch + 1) + 255) / 256),
                  256, 0, d_sc, d_cols, nnz, mont, fg, d_cnt.as<uint32_t>(), boff, d_ent.as<uint32_t>(), rp_dev, nch,
                  d_off.as<uint32_t>(), d_chunks.as<Acc>());
    } else {
        VK_CHECK_HIP(hipMemsetAsync(d_cnt.as<uint32_t>() + nnz, 0, 4, st));
        if (nnz)
            VK_LAUNCH(ctx, "sparse_count", (k_sparse_count<Fr>), (nnz + 255) / 256, 256, 0, d_sc, nnz, mont, fg,
                      d_cnt.as<uint32_t>());
        size_t tmp_bytes = 0;
        VK_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_cnt.as<uint32_t>(), d_eoff.as<uint32_t>(),
                                                      nnz + 1, st));
        VK_TRY(d_tmp.ensure(std::max<size_t>(tmp_bytes, 1)));
        VK_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_bytes, d_cnt.as<uint32_t>(), d_eoff.as<uint32_t>(),
                                                      nnz + 1, st));
        if (nnz)
            VK_LAUNCH(ctx, "sparse_expand", (k_sparse_expand<Fr>), (nnz + 255) / 256, 256, 0, d_sc, d_cols, nnz, mont, fg,
                      d_eoff.as<uint32_t>(), d_ent.as<uint32_t>());
        VK_LAUNCH(ctx, "sparse_rows", (k_sparse_rows<C>), (nch + 1 + 255) / 256, 256, 0, rp_dev,
                  d_eoff.as<uint32_t>(), nch, d_off.as<uint32_t>(), d_chunks.as<Acc>());
        if (Tmax > 0) VK_CHECK_HIP(hipMemsetAsync(chain_max, 0, 4, st));
    }
    // the fixed-base tables hold radix-2^29 limbs in 128-B entries (ec29.hpp FbE): the accumulate
    // reads the entries' limbs (is_fbe)
    using FA = FbE<C>;
    const FA* tab = t->fb.as<FA>();
    if (Tmax > 0) {  // all-zero rows only: the row offsets already set every chunk to the identity
        using RAcc = FAcc<C>;
        DevBuf& d_raw = ctx->ws[WS_RAW_B];
        VK_TRY(d_raw.ensure(nch * sizeof(RAcc)));
        VK_LAUNCH(ctx, "sparse_accumulate", (k_msm_accumulate<C, FA>), (Tmax + 255) / 256, 256, 0, tab, tab, 0xffffffffu,
                  d_ent.as<uint32_t>(), d_off.as<uint32_t>(), (uint32_t)nch, M, d_raw.as<RAcc>(), d_carry.as<RAcc>(),
                  d_thr.as<uint8_t>(), d_own.as<RAcc>(), d_ownb.as<uint32_t>(), chain_max,
                  (unsigned long long*)nullptr, (const AccStart*)nullptr);  // rows are not sorted here: the search
        // straddling chunks merged by the serial walk of their owners, no chain limit: a chunk holds at
        // most CHNZ x W entries, so it spans at most CHNZ W / M + 2 threads. (The pointer-jumping rounds
        // used before read the longest chain back first -- a host sync per level -- and ran ~3 guarded
        // launches: 0.6 ms of the 65,536-key full commitment's kernels.)
        VK_TRY(msm_tail_fixup_walk<C>(ctx, ctx->lane(0), d_off.as<uint32_t>(), (uint32_t)nch, M, d_raw.as<RAcc>(),
                                      d_carry.as<RAcc>(), d_own.as<RAcc>(), 0xffffffffu, d_ownb.as<uint32_t>(),
                                      d_thr.as<uint8_t>(), Tmax));
        VK_LAUNCH(ctx, "sparse_store", (k_fast_store<C>), (nch + 255) / 256, 256, 0, d_raw.as<RAcc>(), (uint32_t)nch,
                  d_off.as<uint32_t>(), d_chunks.as<Acc>());
    }
    // one chunk per row (identity): the chunk sums are the rows -- no combine launch (a one-wave
    // block per row only copied them: ~60 us for the 131,072 extension c1 / c2 rows)
    Acc* rows_p = d_rows.as<Acc>();
    if (ch.identity)
        rows_p = d_chunks.as<Acc>();
    else
        VK_LAUNCH(ctx, "sparse_combine", (k_sparse_combine<typename C::Inl>), batch, 64, 0, d_chunks.as<Acc>(),
                  rc_dev, rows_p);
    if constexpr (std::is_same<C, BN254G1>::value) {
        // BN254 rows with items (the verkle levels): the old-commitment adds, the canonical points,
        // their items and the placement at d_dst in normalize_rows_items' two kernels, the block
        // products polled from page-locked memory (no copies, no stream wait, no separate item /
        // scatter launches: ~40 us of idle GPU per level before, profiles/r05/verkle/)
        if (d_items) {
            lap("kernels");
            return normalize_rows_items(ctx, rows_p, batch, d_add_ids, d_add_xy, d_add_inf, d_dst,
                                        static_cast<uint64_t*>(d_xy), d_inf, static_cast<uint64_t*>(d_items), overlap);
        }
    }
    if (d_dst || overlap) return VC_E_INVALID;  // (BN254 with items only)
    if (d_add_ids)  // rows that update a previous commitment: C_old + sum (delta_k) L_k
        VK_LAUNCH(ctx, "sparse_add_base", (k_rows_add_base<C>), (unsigned)((batch + 255) / 256), 256, 0,
                  rows_p, batch, d_add_ids, d_add_xy, d_add_inf);
    lap("kernels");
    VK_TRY(normalize_to_canon(ctx, ctx->curve, rows_p, batch, d_xy, d_inf));
    lap("normalise");
    if (d_items) VK_TRY(to_data_item_device(ctx, d_xy, d_inf, batch, d_items));
    return VC_OK;
}

template <class C, class Fr>
static int msm_batch_sparse_t(vc_ctx* ctx, Table* t, size_t batch, const uint64_t* row_ptr, const uint32_t* cols,
                              const uint64_t* scalars, int mont, uint64_t* out_xy, uint8_t* out_inf,
                              uint64_t* out_items = nullptr) {
    if (batch == 0) return VC_OK;
    const size_t nnz = row_ptr[batch];
    // argument checks on the host pool (verkle levels: 10^5 rows / non-zeros)
    std::vector<uint8_t> bad_part(host_pool().size(), 0);
    host_pool().run([&](unsigned k) {
        const unsigned T = host_pool().size();
        uint8_t b = 0;
        for (size_t g = batch * k / T; g < batch * (k + 1) / T; g++) b |= row_ptr[g + 1] < row_ptr[g] ? 1 : 0;
        for (size_t j = nnz * k / T; j < nnz * (k + 1) / T; j++) b |= cols[j] >= t->n ? 2 : 0;
        bad_part[k] = b;
    });
    uint8_t bad = 0;
    for (uint8_t b : bad_part) bad |= b;
    if (bad & 1) return VC_E_INVALID;
    if (bad & 2) return VC_E_RANGE;
    hipStream_t st = ctx->stream;
    DevBuf& d_cols = ctx->ws[WS_SP_COLS];
    DevBuf& d_sc = ctx->ws[WS_SP_SC];
    DevBuf& d_xy = ctx->ws[WS_SP_XY];
    DevBuf& d_inf = ctx->ws[WS_SP_INF];
    DevBuf& d_it = ctx->ws[WS_SP_ITEMS];
    VK_TRY(d_cols.ensure(std::max<size_t>(nnz, 1) * 4));
    VK_TRY(d_sc.ensure(std::max<size_t>(nnz, 1) * 32));
    VK_TRY(d_xy.ensure(batch * 2 * C::F::N * 4));
    VK_TRY(d_inf.ensure(batch));
    if (out_items) VK_TRY(d_it.ensure(batch * 32));
    if (nnz) {
        VK_CHECK_HIP(hipMemcpyAsync(d_cols.p, cols, nnz * 4, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_sc.p, scalars, nnz * 32, hipMemcpyHostToDevice, st));
    }
    VK_TRY((sparse_commit_dev<C, Fr>(ctx, t, batch, row_ptr, false, d_cols.as<uint32_t>(), d_sc.p, mont, d_xy.p,
                                     d_inf.as<uint8_t>(), out_items ? d_it.p : nullptr)));
    VK_CHECK_HIP(hipMemcpyAsync(out_xy, d_xy.p, batch * 2 * C::F::N * 4, hipMemcpyDeviceToHost, st));
    VK_CHECK_HIP(hipMemcpyAsync(out_inf, d_inf.p, batch, hipMemcpyDeviceToHost, st));
    if (out_items) VK_CHECK_HIP(hipMemcpyAsync(out_items, d_it.p, batch * 32, hipMemcpyDeviceToHost, st));
    VK_CHECK_HIP(hipStreamSynchronize(st));  // host staging vectors die on return
    return VC_OK;
}

// ---- latency path of the sparse commits (verkle levels of a few thousand non-zeros). The
// sort-based path above is a chain of ~10 launches whose accumulate runs M = 16 serial mixed adds
// per thread and whose fix-up walks straddles serially: ~0.2 ms of kernels for a level of 1,000
// non-zeros, whatever its size (profiles/r05/verkle/). Here a wave takes a chunk of <= 64 of a
// row's (non-zero, window) pairs -- two non-zeros at W = 32 --, every lane adds its one table
// point (a load: the accumulator starts at the identity) and the wave folds on quad-cooperative
// adds (7 dependent ones); rows of several chunks are folded by k_sparse_combine.
// MODE 0: scalars vals[j] (4 canonical words); 1: 16-byte values (2 words: the leaf halves of
// an extension's c1 / c2 rows); 2: item[child[j]] - (sidx[j] < 0 ? 0 : snap[sidx[j]]) mod r (a
// verkle level's children's items from the mirror, minus the old item of a delta row's slot).
struct SmallChunk {
    uint32_t j0, npairs, p0, pad;  // the row's first non-zero, its pair count, this chunk's first pair
};
template <class C, class Fr, int MODE, int NT>
__global__ void __launch_bounds__(NT) k_fb_sparse_small(const FbE<C>* __restrict__ tab, const uint8_t* __restrict__ inf,
                                                       FbGeom fg, const SmallChunk* __restrict__ ck,
                                                       const uint32_t* __restrict__ cols, const uint64_t* __restrict__ vals,
                                                       const uint64_t* __restrict__ item, const uint32_t* __restrict__ child,
                                                       const int32_t* __restrict__ sidx, const uint64_t* __restrict__ snap,
                                                       typename C::Acc* __restrict__ part) {
    using FC = typename Fast29<C>::type;
    const SmallChunk c = ck[blockIdx.x];
    const uint32_t p = c.p0 + threadIdx.x, W = (uint32_t)fg.W;
    typename FC::Acc fa = FC::zero();
    if (p < c.npairs) {
        const size_t j = (size_t)c.j0 + p / W;
        const int w = (int)(p % W);
        const uint32_t col = cols[j];
        fe<Fr> s = fe_zero<Fr>();
        if constexpr (MODE == 0) {
            memcpy(s.v, vals + 4 * j, 32);
        } else if constexpr (MODE == 1) {
            memcpy(s.v, vals + 2 * j, 16);
        } else {
            memcpy(s.v, item + 4 * (size_t)child[j], 32);
            const int32_t k = sidx ? sidx[j] : -1;
            if (k >= 0) {
                fe<Fr> o;
                memcpy(o.v, snap + 4 * (size_t)k, 32);
                s = fe_sub<Fr>(s, o);  // canonical in, canonical out
            }
        }
        int32_t d = 0;
        for_each_digit_fb<Fr>(s, fg, [&](int ww, int32_t dd) {
            if (ww == w) d = dd;
        });
        if (d != 0 && !inf[col])
            fa = FC::madd(fa, tab[(size_t)col * fg.stride() + fg.off(w) + (uint32_t)(d < 0 ? -d : d) - 1].u, d < 0);
    }
    fb_block_sum_store<C, NT>(fa, &part[blockIdx.x]);
}

size_t sparse_small_pairs(const Table* t, size_t nnz) {
    const int W = t->fb_c ? t->fb_geom().W : 32;
    return nnz * (size_t)W;
}

int sparse_small_items_dev(vc_ctx* ctx, Table* t, const SmallRows& in, const std::function<void()>* overlap) {
    using C = BN254G1;
    using Fr = BN254Fr;
    using Acc = C::Acc;
    if (t->curve != VC_CURVE_BN254) return VC_E_INVALID;
    const size_t batch = in.batch;
    if (batch == 0) return VC_OK;
    if (t->fb_c == 0) VK_TRY(fixed_base_precompute(ctx, t, 8));
    const FbGeom fg = t->fb_geom();
    const uint64_t W = (uint64_t)fg.W;
    const uint64_t* rp = in.row_ptr;
    if (rp[batch] * W >= (1ull << 32)) return VC_E_RANGE;
    // chunks of NT pairs: a wave (7 dependent quad adds) while every row fits one (<= 2 non-zeros at
    // W = 32: the extension c1 / c2 rows), else 256 threads (9 adds; rows of <= 8 non-zeros -- the
    // extension rows [1, stem, c1, c2], an update's delta rows -- need no k_sparse_combine, whose
    // one full add per level costs ~30 us, profiles/r05/verkle/)
    uint64_t maxp = 0;
    for (size_t g = 0; g < batch; g++) maxp = std::max<uint64_t>(maxp, (rp[g + 1] - rp[g]) * W);
    const uint32_t NT = maxp <= 64 ? 64 : 256;
    // chunk table (host, page-locked: one upload) and, when a row has several chunks, rc
    size_t nch = 0;
    bool multi = false;
    for (size_t g = 0; g < batch; g++) {
        const uint64_t np = (rp[g + 1] - rp[g]) * W;
        const size_t k = np == 0 ? 1 : (size_t)((np + NT - 1) / NT);
        multi |= k > 1;
        nch += k;
    }
    const size_t ck_bytes = nch * sizeof(SmallChunk), rc_bytes = multi ? (batch + 1) * 4 : 0;
    VK_TRY(ctx->pin_sparse_ck.ensure(ck_bytes + rc_bytes));
    SmallChunk* hck = ctx->pin_sparse_ck.as<SmallChunk>();
    uint32_t* hrc = reinterpret_cast<uint32_t*>(ctx->pin_sparse_ck.as<uint8_t>() + ck_bytes);
    size_t b = 0;
    for (size_t g = 0; g < batch; g++) {
        const uint32_t np = (uint32_t)((rp[g + 1] - rp[g]) * W);
        if (multi) hrc[g] = (uint32_t)b;
        uint32_t p0 = 0;
        do {
            hck[b++] = SmallChunk{(uint32_t)rp[g], np, p0, 0};
            p0 += NT;
        } while (p0 < np);
    }
    if (multi) hrc[batch] = (uint32_t)b;
    hipStream_t st = ctx->stream;
    DevBuf d_ck(ctx), d_part(ctx), d_rows(ctx);
    VK_TRY(d_ck.ensure(ck_bytes + rc_bytes));
    VK_TRY(d_part.ensure(nch * sizeof(Acc)));
    if (multi) VK_TRY(d_rows.ensure(batch * sizeof(Acc)));
    VK_CHECK_HIP(hipMemcpyAsync(d_ck.p, hck, ck_bytes + rc_bytes, hipMemcpyHostToDevice, st));
    using FA = FbE<C>;
    const FA* tab = t->fb.as<FA>();
    const uint8_t* tinf = t->inf.as<uint8_t>();
    const SmallChunk* dck = d_ck.as<SmallChunk>();
#define VK_SMALL_(MODE, NTV)                                                                                  \
    VK_LAUNCH(ctx, "sparse_small", (k_fb_sparse_small<C, Fr, MODE, NTV>), nch, NTV, 0, tab, tinf, fg, dck, in.d_cols, \
              in.d_vals, in.d_item, in.d_child, in.d_sidx, in.d_snap, d_part.as<Acc>())
    if (NT == 64) {
        if (in.mode == 0) VK_SMALL_(0, 64);
        else if (in.mode == 1) VK_SMALL_(1, 64);
        else VK_SMALL_(2, 64);
    } else {
        if (in.mode == 0) VK_SMALL_(0, 256);
        else if (in.mode == 1) VK_SMALL_(1, 256);
        else VK_SMALL_(2, 256);
    }
#undef VK_SMALL_
    Acc* rows = d_part.as<Acc>();
    if (multi) {
        VK_LAUNCH(ctx, "sparse_combine", (k_sparse_combine<C::Inl>), batch, 64, 0, d_part.as<Acc>(),
                  reinterpret_cast<const uint32_t*>(d_ck.as<uint8_t>() + ck_bytes), d_rows.as<Acc>());
        rows = d_rows.as<Acc>();
    }
    return normalize_rows_items(ctx, rows, batch, in.d_add_ids, in.d_add_xy, in.d_add_inf, in.d_dst, in.d_out_xy,
                                in.d_out_inf, in.d_out_item, overlap);
}

// BN254 sparse commits with device inputs and outputs (the verkle tree's device-resident levels)
int sparse_commit_items_dev(vc_ctx* ctx, Table* t, size_t batch, const uint64_t* row_ptr, bool rows_fit,
                            const uint32_t* d_cols, const void* d_sc, void* d_xy, uint8_t* d_inf, void* d_items,
                            const uint32_t* d_add_ids, const uint64_t* d_add_xy, const uint8_t* d_add_inf,
                            const uint32_t* d_dst, const std::function<void()>* overlap, const uint64_t* d_row_ptr) {
    if (t->curve != VC_CURVE_BN254 || !d_items) return VC_E_INVALID;
    return sparse_commit_dev<BN254G1, BN254Fr>(ctx, t, batch, row_ptr, rows_fit, d_cols, d_sc, 0, d_xy, d_inf, d_items,
                                               d_add_ids, d_add_xy, d_add_inf, d_dst, overlap, d_row_ptr);
}

int msm_batch_sparse_items(vc_ctx* ctx, Table* t, size_t batch, const uint64_t* row_ptr, const uint32_t* cols,
                           const uint64_t* scalars, int mont, uint64_t* out_xy, uint8_t* out_inf, uint64_t* out_items) {
    if (t->curve != VC_CURVE_BN254 || (batch && !out_items)) return VC_E_INVALID;
    return msm_batch_sparse_t<BN254G1, BN254Fr>(ctx, t, batch, row_ptr, cols, scalars, mont, out_xy, out_inf,
                                                 out_items);
}

int msm_batch_sparse(vc_ctx* ctx, Table* t, size_t batch, const uint64_t* row_ptr, const uint32_t* cols,
                     const uint64_t* scalars, int mont, uint64_t* out_xy, uint8_t* out_inf) {
    switch (t->curve) {
        case VC_CURVE_BN254:
            return msm_batch_sparse_t<BN254G1, BN254Fr>(ctx, t, batch, row_ptr, cols, scalars, mont, out_xy, out_inf);
        case VC_CURVE_BLS12_381:
            return msm_batch_sparse_t<BLS381G1, BLS381Fr>(ctx, t, batch, row_ptr, cols, scalars, mont, out_xy,
                                                           out_inf);
        case VC_CURVE_BANDERSNATCH:
            return msm_batch_sparse_t<Bandersnatch, BandFr>(ctx, t, batch, row_ptr, cols, scalars, mont, out_xy,
                                                             out_inf);
    }
    return VC_E_INVALID;
}
}  // namespace vk

// Accumulators to affine points, split around the host (batch_inv.hpp has the pieces): the single
// field inversion of each 256-element block is ~130 us on one GPU lane (a lone wave's serial
// binary-Euclid loop), while the host inverts in a few us. A prep kernel leaves each element the
// product of its block's OTHER denominators and the block product; the host inverts all block
// products with one inversion (Montgomery's trick) and a finish kernel scales. One pinned round trip
// (~20 us) replaces the lane inversion: 10k Bandersnatch commits normalise in ~0.06 instead of
// 0.18 ms. Two forms: normalize_to_canon (any curve; copies and two stream waits) and the verkle
// rows' normalize_rows_items (BN254; polled flags in fine-grained memory, a device scan from 128
// blocks on, the finish kernel queued ahead of the host's inverse: NormGo).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "batch_inv.hpp"
#include "ctx.hpp"
#include "ec.hpp"

namespace vk {

// others[j] and tot[block] of this block's accumulators (a: row j's, the identity past count)
template <class C>
__device__ __forceinline__ void norm_prep_block(const typename C::Acc& a, size_t j, size_t count,
                                                fe<typename C::F>* pre, fe<typename C::F>* suf,
                                                fe<typename C::F>* __restrict__ others,
                                                fe<typename C::F>* __restrict__ tot) {
    using F = typename C::F;
    block_scan256<F>((j < count && !norm_as_one<C>(a)) ? denom<C>(a) : fe_one<F>(), pre, suf);
    const fe<F> o = scan_others<F>(pre, suf);
    if (j < count) others[j] = o;
    if (threadIdx.x == 0) tot[blockIdx.x] = pre[255];
}
template <class C>
__global__ void __launch_bounds__(256) k_norm_prep(const typename C::Acc* __restrict__ in, size_t count,
                                                  fe<typename C::F>* __restrict__ others,
                                                  fe<typename C::F>* __restrict__ tot) {
    __shared__ fe<typename C::F> pre[256];
    __shared__ fe<typename C::F> suf[256];
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    norm_prep_block<C>(j < count ? in[j] : C::zero(), j, count, pre, suf, others, tot);
}
// verkle rows (BN254): row j first takes the canonical affine point (add_xy, add_inf)[add_ids[j]]
// (0xffffffff: none) -- the old commitment of a delta row -- and is written back with it
__global__ void __launch_bounds__(256) k_norm_prep_vk(BN254G1::Acc* __restrict__ rows, size_t count,
                                                     const uint32_t* __restrict__ add_ids,
                                                     const uint64_t* __restrict__ add_xy,
                                                     const uint8_t* __restrict__ add_inf,
                                                     fe<BN254Fq>* __restrict__ others, fe<BN254Fq>* __restrict__ tot,
                                                     uint32_t* __restrict__ flags, uint32_t epoch,
                                                     uint32_t* __restrict__ counter, fe<BN254Fq>* __restrict__ cof,
                                                     fe<BN254Fq>* __restrict__ total, uint64_t* __restrict__ tags) {
    using C = BN254G1;
    using F = BN254Fq;
    __shared__ fe<F> pre[256], suf[256];  // the rows' scan, then (last block) the segments'
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    C::Acc a = j < count ? rows[j] : C::zero();
    if (add_ids && j < count) {
        const uint32_t id = add_ids[j];
        if (id != 0xffffffffu && !add_inf[id]) {
            C::Aff q;
            memcpy(q.x.v, add_xy + 8 * (size_t)id, 32);
            memcpy(q.y.v, add_xy + 8 * (size_t)id + 4, 32);
            q.x = fe_to_mont<BN254Fq>(q.x);
            q.y = fe_to_mont<BN254Fq>(q.y);
            a = C::madd(a, q, false);
            rows[j] = a;
        }
    }
    norm_prep_block<C>(a, j, count, pre, suf, others, tot);
    if (counter == nullptr) {
        // tot in fine-grained host memory (normalize_rows_items): the block product is made visible
        // system wide, then the block's flag takes this launch's epoch (the host polls the flags)
        if (flags != nullptr && threadIdx.x == 0) {
            __threadfence_system();
            __hip_atomic_store(&flags[blockIdx.x], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    // device scan (tot in device memory): the last block to arrive turns the nblk block products
    // into per-block cofactors cof[b] = prod_{k != b} tot[k] and hands the host only their total
    // (one inversion there, ~1 us, instead of Montgomery's trick over every block product: ~3
    // multiplies per block, 40 us for 512 blocks, with the GPU idle).
    // tags (round 6): each block publishes its product as eight (epoch << 32 | limb) words and
    // arrives without a fence; the last block polls the words until they carry this launch's epoch.
    // An agent-scope fence per block writes back its XCD's whole L2 first -- with 512 blocks that
    // was most of the kernel (profiles/r06/verkle/fence_free/).
    __shared__ uint32_t s_last;
    const uint32_t tid = threadIdx.x, nb = gridDim.x;
    const uint64_t tag = (uint64_t)epoch << 32;
    if (tid == 0) {
        const fe<F> mine = tot[blockIdx.x];  // (this thread's own store in norm_prep_block)
#pragma unroll
        for (int k = 0; k < F::N; k++)
            __hip_atomic_store(&tags[(size_t)F::N * blockIdx.x + k], tag | mine.v[k], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        s_last = atomicAdd(counter, 1u) == nb - 1 ? 1u : 0u;
    }
    __syncthreads();  // (also: every lane has read the rows' scan before pre / suf are scanned again)
    if (!s_last) return;
    // another block's product: every block stored its words before it arrived, so the wait is
    // short (bounded anyway)
    auto load = [&](uint32_t b) {
        fe<F> v;
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            bool all = true;
#pragma unroll
            for (int k = 0; k < F::N; k++) {
                const uint64_t w = __hip_atomic_load(&tags[(size_t)F::N * b + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                v.v[k] = (uint32_t)w;
                all = all && (w & 0xffffffff00000000ull) == tag;
            }
            if (all || __builtin_amdgcn_s_memrealtime() - t0 > 1000000ull) break;  // (10 ms)
        }
        return v;
    };
    const uint32_t per = (nb + 255) / 256, b0 = min(tid * per, nb), b1 = min(b0 + per, nb);
    fe<F> seg = fe_one<F>();
    for (uint32_t b = b1; b-- > b0;) {  // suffix products inside the segment, parked in cof
        cof[b] = seg;
        seg = fe_mul<F>(load(b), seg);
    }
    block_scan256<F>(seg, pre, suf);
    fe<F> run = tid > 0 ? pre[tid - 1] : fe_one<F>();           // the segments before this one
    const fe<F> after = tid < 255 ? suf[tid + 1] : fe_one<F>();  // and after it
    for (uint32_t b = b0; b < b1; b++) {
        cof[b] = fe_mul<F>(fe_mul<F>(run, cof[b]), after);
        run = fe_mul<F>(run, load(b));
    }
    if (tid == 0) {
        *total = pre[255];
        *counter = 0;  // for the next launch (stream-ordered after this one)
        __threadfence_system();
        __hip_atomic_store(&flags[0], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

template <class C>
__global__ void __launch_bounds__(256) k_norm_finish(const typename C::Acc* __restrict__ in, size_t count,
                                                    const fe<typename C::F>* __restrict__ others,
                                                    const fe<typename C::F>* __restrict__ binv,
                                                    typename C::Aff* __restrict__ out_aff,
                                                    uint32_t* __restrict__ out_canon, uint8_t* __restrict__ out_inf) {
    using F = typename C::F;
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= count) return;
    fe<F> x, y;
    bool ident;
    acc_affine<C>(in[j], fe_mul<F>(binv[blockIdx.x], others[j]), x, y, ident);
    store_affine<C>(j, x, y, ident, out_aff, out_canon, out_inf);
}

// A finish kernel queued before the host has its inverse(s) (normalize_rows_items): lane 0 of block
// 0 waits for `flag` == epoch in fine-grained page-locked memory and hands it on through `relay` in
// device memory, where the other blocks wait -- with the total's inverse itself in the device-scan
// form: 512 blocks reading the same page-locked words over PCIe were served one after another,
// ~0.8 us per block, 0.4 ms for the 131,072-row level (measured, profiles/r06/verkle/norm_early/).
// In the per-block form each block reads its own inverse there. Every wait is bounded on the
// 100 MHz clock: past `limit` ticks block 0 (or a block that never saw the relay) inverts the
// value itself (prod: the block products or their total, written by the prep kernel), so the
// kernel ends whatever the host does -- it only gets slower.
struct NormGo {
    const uint32_t* flag = nullptr;  // null: the inverses were written before the launch
    uint64_t* relay = nullptr;       // 9 device words block 0 hands the go on through
    uint32_t epoch = 0;
    uint32_t per_block = 0;             // 1: inv[b] = 1 / prod[b] per block; 0: inv[0] = 1 / prod[0] (the total)
    const fe<BN254Fq>* prod = nullptr;  // what the host inverts (device view of the page-locked staging)
    const fe<BN254Fq>* inv = nullptr;   // where the host writes the inverse(s)
    uint64_t limit = 0;
};
// (four 64-bit loads: page-locked host memory is read over PCIe uncached)
__device__ __forceinline__ fe<BN254Fq> load_fe_sys(const fe<BN254Fq>* p) {
    static_assert(BN254Fq::N == 8, "");
    fe<BN254Fq> v;
    uint64_t* src = const_cast<uint64_t*>(reinterpret_cast<const uint64_t*>(p));
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint64_t w = __hip_atomic_load(&src[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        v.v[2 * k] = (uint32_t)w;
        v.v[2 * k + 1] = (uint32_t)(w >> 32);
    }
    return v;
}

// verkle rows (BN254): canonical affine point, identity flag and to_data_item of row j stored at
// dst[j] (dst null: at j) -- straight into the tree's device mirror
__global__ void __launch_bounds__(256) k_norm_finish_vk(const BN254G1::Acc* __restrict__ rows, size_t count,
                                                       const fe<BN254Fq>* __restrict__ others,
                                                       const fe<BN254Fq>* __restrict__ binv,
                                                       const uint32_t* __restrict__ dst, uint64_t* __restrict__ out_xy,
                                                       uint8_t* __restrict__ out_inf, uint64_t* __restrict__ out_item,
                                                       const fe<BN254Fq>* __restrict__ tinv, NormGo go) {
    using F = BN254Fq;
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    __shared__ fe<F> s_bi;
    if (go.flag) {  // (uniform: every thread of the block reaches the barrier)
        if (threadIdx.x == 0) {
            const uint32_t k = go.per_block ? blockIdx.x : 0u;
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            // relay words in device memory, each (epoch << 32) | payload, so a reader needs no ordering
            // between them and the writer no release (an agent-scope release writes back the whole
            // L2 of block 0's XCD first): [0, 8) the total's inverse, [8] whether the host answered
            uint64_t* rl = go.relay;
            const uint64_t tag = (uint64_t)go.epoch << 32;
            bool host = false, have = false, seen = false;
            fe<F> v;
            if (blockIdx.x == 0) {
                uint32_t* flag = const_cast<uint32_t*>(go.flag);
                for (;;) {
                    if (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) == go.epoch) {
                        host = true;
                        break;
                    }
                    if (__builtin_amdgcn_s_memrealtime() - t0 > go.limit) break;
                    __builtin_amdgcn_s_sleep(1);
                }
                seen = true;
                if (!go.per_block) {  // the one inverse: read over PCIe once, handed on in device memory
                    v = host ? load_fe_sys(go.inv) : fe_inv_bin<F>(load_fe_sys(go.prod));
                    have = true;
#pragma unroll
                    for (int i = 0; i < F::N; i++)
                        __hip_atomic_store(&rl[i], tag | v.v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else {
                    __hip_atomic_store(&rl[8], tag | (host ? 1u : 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else {
                const int nw = go.per_block ? 1 : F::N;
                uint64_t* src = go.per_block ? rl + 8 : rl;
                uint64_t w[F::N];
                for (;;) {
                    bool all = true;
                    for (int i = 0; i < nw; i++) {
                        w[i] = __hip_atomic_load(&src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        all = all && (w[i] >> 32) == go.epoch;
                    }
                    if (all) {
                        seen = true;
                        break;
                    }
                    if (__builtin_amdgcn_s_memrealtime() - t0 > go.limit) break;
                    __builtin_amdgcn_s_sleep(1);
                }
                if (seen && go.per_block) host = (w[0] & 1u) != 0;
                if (seen && !go.per_block) {
#pragma unroll
                    for (int i = 0; i < F::N; i++) v.v[i] = (uint32_t)w[i];
                    have = true;
                }
            }
            // per block: its own inverse from the host (distinct addresses), or made here
            if (!have) v = host ? load_fe_sys(go.inv + k) : fe_inv_bin<F>(load_fe_sys(go.prod + k));
            s_bi = go.per_block ? v : fe_mul<F>(v, binv[blockIdx.x]);
        }
        __syncthreads();
    }
    if (j >= count) return;
    // the block's inverse: binv[b], or (device scan) the cofactor times the total's inverse, or
    // (queued early) what lane 0 got above
    const fe<F> bi = go.flag ? s_bi : tinv ? fe_mul<F>(*tinv, binv[blockIdx.x]) : binv[blockIdx.x];
    fe<F> x, y;
    bool ident;
    acc_affine<BN254G1>(rows[j], fe_mul<F>(bi, others[j]), x, y, ident);
    fe<F> cx = fe_from_mont<F>(x), cy = fe_from_mont<F>(y);
    if (ident) cx = cy = fe_zero<F>();
    const size_t o = dst ? dst[j] : j;
    memcpy(out_xy + 8 * o, cx.v, 32);
    memcpy(out_xy + 8 * o + 4, cy.v, 32);
    out_inf[o] = ident ? 1 : 0;
    const fe<BN254Fr> it = to_data_item_canon(cx, cy, ident);
    memcpy(out_item + 4 * o, it.v, 32);
}

// d_in (count accumulators) -> affine / canonical outputs; synchronises the stream once
template <class C>
static int normalize_split(vc_ctx* ctx, const typename C::Acc* d_in, size_t count, typename C::Aff* out_aff,
                           uint32_t* out_canon, uint8_t* out_inf) {
    using F = typename C::F;
    if (count == 0) return VC_OK;
    const size_t nblk = (count + 255) / 256;
    DevBuf others(ctx), tot(ctx);
    VK_TRY(others.ensure(count * sizeof(fe<F>)));
    VK_TRY(tot.ensure(nblk * sizeof(fe<F>)));
    VK_TRY(ctx->pin_norm.ensure(2 * nblk * sizeof(fe<F>)));
    fe<F>* h = ctx->pin_norm.as<fe<F>>();
    VK_LAUNCH(ctx, "norm_prep", (k_norm_prep<C>), nblk, 256, 0, d_in, count, others.as<fe<F>>(), tot.as<fe<F>>());
    VK_CHECK_HIP(hipMemcpyAsync(h, tot.p, nblk * sizeof(fe<F>), hipMemcpyDeviceToHost, ctx->stream));
    VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    BlockInverses<F> bi{h, h + nblk, nblk};  // (never zero: identities count as 1)
    bi.take(nblk);
    bi.finish();
    VK_CHECK_HIP(hipMemcpyAsync(tot.p, bi.inv, nblk * sizeof(fe<F>), hipMemcpyHostToDevice, ctx->stream));
    VK_LAUNCH(ctx, "norm_finish", (k_norm_finish<C>), nblk, 256, 0, d_in, count, others.as<fe<F>>(),
              tot.as<fe<F>>(), out_aff, out_canon, out_inf);
    // the pinned staging is reused by the next call: the copy above must have left it
    VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return VC_OK;
}

// verkle rows (BN254, device): optional old-commitment adds, then canonical affine points,
// identity flags and to_data_item values at dst[j] (k_norm_prep_vk / k_norm_finish_vk). One
// pinned round trip (the block products' inversion on the host) and no trailing synchronisation:
// the finish kernel and its H2D copy stay queued (the next call synchronises the stream -- after
// the D2H of its products -- before its host writes into pin_norm_vk, so the copy has left it).
int normalize_rows_items(vc_ctx* ctx, void* d_rows, size_t n, const uint32_t* add_ids, const uint64_t* add_xy,
                         const uint8_t* add_inf, const uint32_t* dst, uint64_t* out_xy, uint8_t* out_inf,
                         uint64_t* out_item, const std::function<void()>* overlap) {
    using F = BN254Fq;
    if (n == 0) return VC_OK;
    const size_t nblk = (n + 255) / 256;
    DevBuf others(ctx);
    VK_TRY(others.ensure(n * sizeof(fe<F>)));
    // fine-grained page-locked staging of its own, two halves used by alternate calls, each
    // [block products | inverses | flags]: the prep kernel writes the products and per-block flags
    // straight into it, the host polls the flags, writes the inverses there and the finish kernel
    // reads them in place -- no copies, no stream wait (a bounded spin; the stream wait is the
    // fallback). The previous call's finish may still read its inverses, so this call takes the
    // other half (the call before that finished: its successor's prep, queued after it, was seen
    // complete); the buffer grows only after a sync.
    // [block products | inverses | the prep's flags | the host's go word]
    const size_t flag_off = 2 * nblk * sizeof(fe<F>), go_off = flag_off + nblk * 4;
    const size_t half_bytes = (go_off + 4 + 255) / 256 * 256;
    if (ctx->pin_norm_vk.cap < 2 * half_bytes) {
        VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        VK_TRY(ctx->pin_norm_vk.ensure(2 * half_bytes));
    }
    const size_t half = ctx->pin_norm_vk.cap / 2 / 256 * 256;  // (>= half_bytes)
    ctx->norm_vk_parity ^= 1u;
    uint8_t* hbase = ctx->pin_norm_vk.as<uint8_t>() + ctx->norm_vk_parity * half;
    uint8_t* dbase = static_cast<uint8_t*>(ctx->pin_norm_vk.dp) + ctx->norm_vk_parity * half;
    fe<F>* h = reinterpret_cast<fe<F>*>(hbase);
    fe<F>* dh = reinterpret_cast<fe<F>*>(dbase);
    volatile uint32_t* hflags = reinterpret_cast<volatile uint32_t*>(hbase + flag_off);
    uint32_t* dflags = reinterpret_cast<uint32_t*>(dbase + flag_off);
    volatile uint32_t* hgo = reinterpret_cast<volatile uint32_t*>(hbase + go_off);
    const uint32_t epoch = next_epoch(ctx);
    // the finish kernel queued right behind the prep, before the host has the inverse (NormGo): its
    // blocks wait on the host's go word, so the host's inversion is no longer followed by a launch
    // (~10-20 us of idle GPU per level) and the host queues the next level's work while the prep
    // runs. VKZG_NORM_EARLY=0: launch the finish after the inversion (A/B); VKZG_NORM_EARLY_US: the
    // blocks' wait before they invert on their own.
    // (both read per call: a test sets a 1-us bound to run the blocks' own inversions)
    const char* ee = getenv("VKZG_NORM_EARLY");
    const char* eu = getenv("VKZG_NORM_EARLY_US");
    const bool early = !(ee && atoi(ee) == 0);
    const uint64_t early_ticks = 100ull * (uint64_t)(eu ? std::max(1, atoi(eu)) : 2000);
    // (per-kernel timing keeps the late launch: the finish's events would count the host's wait)
    NormGo go;
    const bool early_now = early && !ctx->timing;
    DevBuf& cnt = ctx->ws[WS_NORM_CNT];  // word 0: the prep's arrival counter; word 16: the sparse commits' (sparse_commit.hip k_sparse_count_scan); bytes [128, 200): the relay
    if (cnt.p == nullptr) {
        VK_TRY(cnt.ensure(256));
        VK_CHECK_HIP(hipMemsetAsync(cnt.p, 0, 256, ctx->stream));
    }
    if (early_now) {
        *hgo = 0;
        go.relay = reinterpret_cast<uint64_t*>(cnt.as<uint8_t>() + 128);
        go.flag = reinterpret_cast<const uint32_t*>(dbase + go_off);
        go.epoch = epoch;
        go.limit = early_ticks;
    }
    auto release_go = [&]() {
        std::atomic_thread_fence(std::memory_order_release);  // the inverses before the word that frees them
        *hgo = epoch;
    };
    // the last block's scan costs ~17 us of serial multiplies whatever nblk is; the host's trick
    // ~54 ns per block: the scan pays from ~128 blocks on (c1 / c2 rows: 88 -> 74 us of prep + gap,
    // width-4 rows 76 -> 58 us; a 256-row level 24 -> 43 us: profiles/r05/verkle/sparse_norm_vk/)
    if (nblk >= 128) {
        // the block products scanned on the device (k_norm_prep_vk's last block): the host inverts
        // their total only; page-locked [total | its inverse | flag] in the same alternating halves
        DevBuf& dt = ctx->ws[WS_NORM_TOT];
        VK_TRY(dt.ensure(2 * nblk * sizeof(fe<F>) + nblk * F::N * 8));
        fe<F>* dtot = dt.as<fe<F>>();
        uint64_t* tags = reinterpret_cast<uint64_t*>(dtot + 2 * nblk);
        hflags[0] = 0;
        VK_LAUNCH(ctx, "norm_prep", k_norm_prep_vk, nblk, 256, 0, static_cast<BN254G1::Acc*>(d_rows), n, add_ids,
                  add_xy, add_inf, others.as<fe<F>>(), dtot, dflags, epoch, cnt.as<uint32_t>(), dtot + nblk, dh, tags);
        if (early_now) {
            go.per_block = 0;
            go.prod = dh;
            go.inv = dh + 1;
            VK_LAUNCH(ctx, "norm_finish", k_norm_finish_vk, nblk, 256, 0, static_cast<const BN254G1::Acc*>(d_rows), n,
                      others.as<fe<F>>(), dtot + nblk, dst, out_xy, out_inf, out_item, (const fe<F>*)nullptr, go);
        }
        if (overlap && *overlap) (*overlap)();
        const bool seen = poll_bounded([&] { return hflags[0] == epoch; });
        std::atomic_thread_fence(std::memory_order_acquire);
        // (queued early: this wait also covers the finish, whose blocks invert on their own past their bound)
        if (!seen) VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        h[1] = fe_inv_bin<F>(h[0]);  // never zero: identities count as 1
        if (early_now) {
            release_go();
            return VC_OK;
        }
        std::atomic_thread_fence(std::memory_order_release);  // the inverse before the launch that reads it
        VK_LAUNCH(ctx, "norm_finish", k_norm_finish_vk, nblk, 256, 0, static_cast<const BN254G1::Acc*>(d_rows), n,
                  others.as<fe<F>>(), dtot + nblk, dst, out_xy, out_inf, out_item, dh + 1, NormGo{});
        return VC_OK;
    }
    for (size_t b = 0; b < nblk; b++) hflags[b] = 0;
    VK_LAUNCH(ctx, "norm_prep", k_norm_prep_vk, nblk, 256, 0, static_cast<BN254G1::Acc*>(d_rows), n, add_ids, add_xy,
              add_inf, others.as<fe<F>>(), dh, dflags, epoch, (uint32_t*)nullptr, (fe<F>*)nullptr, (fe<F>*)nullptr,
              (uint64_t*)nullptr);
    if (early_now) {
        go.per_block = 1;
        go.prod = dh;
        go.inv = dh + nblk;
        VK_LAUNCH(ctx, "norm_finish", k_norm_finish_vk, nblk, 256, 0, static_cast<const BN254G1::Acc*>(d_rows), n,
                  others.as<fe<F>>(), dh + nblk, dst, out_xy, out_inf, out_item, (const fe<F>*)nullptr, go);
    }
    if (overlap && *overlap) (*overlap)();
    // Montgomery's trick over the block products: the forward products are taken as the blocks'
    // flags arrive (blocks finish roughly in order), so only the inversion and the backward pass
    // follow the last block
    BlockInverses<F> bi{h, h + nblk, nblk};
    const bool seen = poll_bounded([&] {
        size_t b = bi.done;
        while (b < nblk && hflags[b] == epoch) b++;
        if (b > bi.done) {
            std::atomic_thread_fence(std::memory_order_acquire);  // the products after their flags
            bi.take(b);
        }
        return bi.done == nblk;
    });
    if (!seen) {
        VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        bi.take(nblk);
    }
    bi.finish();
    if (early_now) {
        release_go();
        return VC_OK;
    }
    std::atomic_thread_fence(std::memory_order_release);  // the inverses before the launch that reads them
    VK_LAUNCH(ctx, "norm_finish", k_norm_finish_vk, nblk, 256, 0, static_cast<const BN254G1::Acc*>(d_rows), n,
              others.as<fe<F>>(), dh + nblk, dst, out_xy, out_inf, out_item, (const fe<F>*)nullptr, NormGo{});
    return VC_OK;
}

// normalise n device accumulators to canonical affine (device outputs)
int normalize_to_canon(vc_ctx* ctx, int curve, const void* d_acc, size_t n, void* d_out_xy, uint8_t* d_out_inf) {
    if (n == 0) return VC_OK;
#define VK_NORM_(C)                                                                                      \
    normalize_split<C>(ctx, reinterpret_cast<const C::Acc*>(d_acc), n, (C::Aff*)nullptr,                \
                       reinterpret_cast<uint32_t*>(d_out_xy), d_out_inf)
    switch (curve) {
        case VC_CURVE_BN254: return VK_NORM_(BN254G1);
        case VC_CURVE_BLS12_381: return VK_NORM_(BLS381G1);
        case VC_CURVE_BANDERSNATCH: return VK_NORM_(Bandersnatch);
    }
#undef VK_NORM_
    return VC_E_INVALID;
}

}  // namespace vk

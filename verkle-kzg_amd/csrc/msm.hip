// Variable-base Pippenger MSM for gfx950 -- the engine behind utils::inner_product
// (the reference's vector-commit/src/utils.rs:16-19) at large n (configs 2 and 4).
//
// Pipeline (all on the ctx stream, one host sync at the end):
//   k_sort_*         scalar -> W signed c-bit digits (|d| <= 2^(c-1), msm_digits.hpp); two-pass LDS counting
//   (msm_sort.hpp)   sort of the (window, bucket) keys: sorted[] = i | sign<<31 grouped by
//                    bucket, offsets[] = bucket starts (all windows concatenated), and the
//                    start record of every accumulate thread (AccStart)
//   k_msm_accumulate every thread sums exactly M consecutive sorted entries (mixed adds
//   (msm_accumulate  of affine bases gathered from HBM), writing complete buckets directly
//    .hpp)           and bucket pieces that straddle a thread boundary to side slots
//   k_msm_fixup      owner thread of a straddling bucket folds the pieces
//   msm_tail.hip     segment sums, bit sums (window sum = sum_b b B_b without a serial
//                    running sum over all buckets), then host Horner over bit positions
// Load balance does not depend on the scalar distribution: the accumulate work per
// thread is fixed (M entries) even when every scalar hits one bucket.
// Here: the slices and the msm_run* paths; their geometry is msm_plan.hpp's, the tables msm_tables.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "msm_internal.hpp"
#include "msm_sort.hpp"  // msm_accumulate.hpp, msm_digits.hpp, msm_tail.hpp (ctx, ec, ec29), msm_plan.hpp

namespace vk {

// One window slice [wb, we) of an MSM enqueued on a lane: sort, accumulate, fix-up, reduction and
// the read-back of its W (J + 1) reduced points; slice_finish waits for it and folds them by
// Horner over bit positions. (Two staggered slices of one window range on the two lanes measured
// no faster at 2^20 BLS12-381, 4.09-4.29 vs 3.98-4.06 ms: a 4-window slice's accumulate fills one
// wave per SIMD, and the overlapped tail shares the same SIMDs. Removed.)
template <class C>
struct MsmSlice {
    using Acc = typename C::Acc;
    Lane L{};
    int c = 0, wb = 0, we = 0, W = 0;
    bool shared = false;  // all windows into one bucket set (Table::win copies)
    int top_f = 0;        // per-window buckets: the top window's shortfall (top_shortfall), if in the slice
    uint32_t m = 1;       // > 1: radix m 2^c digits (RadixDigits), m 2^(c-1) buckets
    int sets = 1;         // shared windows: bucket sets = MSMs over the table in this slice
    uint32_t wps = 0;     // shared windows: windows per set (the window copies' count)
    uint32_t stride = 0;  // shared windows: points per window copy (2N for a table of N); 0 = the terms
    int Wr = 0;           // bucket sets reduced: `sets` shared, W otherwise
    SlicePlan p{};        // the geometry slice_enqueue planned (msm_plan.hpp)
    uint32_t* offsets = nullptr;
    uint32_t* chain_max = nullptr;  // in the WS_TAIL buffer, tail_bytes after the tail points
    size_t tail_bytes = 0;
    uint8_t* through = nullptr;
    uint32_t* owner_b = nullptr;
    FAcc<C>* buckets = nullptr;
    FAcc<C>* carry = nullptr;
    FAcc<C>* owner = nullptr;
    FAcc<C>* seg = nullptr;
    FAcc<C>* rs = nullptr;
    FAcc<C>* bsum_part = nullptr;
    Acc* tail = nullptr;
    std::vector<Acc> ht;
    uint32_t Lmax = 0;
    // chunked MSMs (msm_run_host_chunks_t): the accumulate writes these buckets instead of the
    // workspace's, the chain word is this one, and the reduction is left to the caller
    FAcc<C>* bucket_dst = nullptr;
    uint32_t* chain_dst = nullptr;
    bool skip_reduce = false;
    // direct completion (TailDirect): the final stage wrote the points and the chain word into the
    // lane's fine-grained page-locked buffer, then `nflags` flags at flag_off took `epoch`
    bool direct = false;
    uint32_t epoch = 0, nflags = 0;
    size_t flag_off = 0;
    double t_launch0 = 0.0;  // host_timing(): when the slice's first kernel was launched (us)
    // BLS12-381 radix digits still to be made (msm_run_t leaves the GLV split to slice_enqueue,
    // which fuses the sort histogram into it when the geometry allows): sc == nullptr otherwise
    struct {
        std::vector<const uint32_t*> sc;  // one scalar set per bucket set (empty: digits made already)
        std::vector<int> mont;
        const uint8_t* inf = nullptr;
        uint32_t n = 0;
        int32_t* dig = nullptr;  // set s at dig + s W 2n
    } radix;
};

template <class C, class BT, class Src>
static int slice_enqueue(vc_ctx* ctx, MsmSlice<C>& sl, Src src, size_t nv, const BT* bases, const BT* phi,
                         uint32_t nphi) {
    using Acc = typename C::Acc;
    using RAcc = FAcc<C>;  // raw radix-29 accumulators of the accumulate / fix-up / reduction
    const Lane L = sl.L;
    const int c = sl.c, W = sl.W;  // shared: W = sets x windows per set
    const int Wr = sl.shared ? sl.sets : W;
    sl.Wr = Wr;
    SliceShape sh;
    sh.nv = nv, sh.c = c, sh.W = W, sh.wb = sl.wb, sh.we = sl.we;
    sh.shared = sl.shared, sh.sets = sl.sets, sh.m = sl.m, sh.top_f = sl.top_f, sh.sort_chunk = SORT_CHUNK;
    if (const char* em = getenv("VKZG_MSM_M")) sh.m_override = (uint32_t)std::max(1, atoi(em));  // tuning probe
    const SlicePlan p = sl.p = msm_slice_plan(sh);
    const uint32_t NB = p.NB, NBtot = p.NBtot, M = p.M, Lseg = p.Lseg, S = p.S, J = p.J, nU = p.nU, Tmax = p.Tmax;
    const uint32_t FB = p.FB, NBC = p.NBC, nblk = p.nblk, chunk = p.chunk;
    const size_t ncnt = p.ncnt, maxL = nv * (size_t)W;
    hipStream_t st = L.st;
    DevBuf* ws = L.ws;
    VK_TRY(ws[WS_DIGITS].ensure(maxL * 8));
    VK_TRY(ws[WS_COUNTS].ensure(ncnt * 4));
    VK_TRY(ws[WS_CURSOR].ensure(ncnt * 4));
    VK_TRY(ws[WS_OFFSETS].ensure((size_t)(NBtot + 1) * 4));
    VK_TRY(ws[WS_SORTED].ensure(maxL * 4));
    VK_TRY(ws[WS_BUCKETS].ensure((size_t)NBtot * sizeof(RAcc)));
    VK_TRY(ws[WS_CARRY].ensure((size_t)(Tmax + 8) * sizeof(RAcc)));
    VK_TRY(ws[WS_THROUGH].ensure((size_t)(Tmax + 8)));
    VK_TRY(ws[WS_OWNER].ensure((size_t)(Tmax + 8) * sizeof(RAcc)));
    VK_TRY(ws[WS_OWNER_B].ensure((size_t)(Tmax + 8) * 4));
    VK_TRY(ws[WS_STARTS].ensure((size_t)(Tmax + 8) * sizeof(AccStart)));  // threads < T <= Tmax and the sentinel T
    AccStart* const starts = ws[WS_STARTS].as<AccStart>();
    VK_TRY(ws[WS_SEG].ensure((size_t)S * Wr * sizeof(RAcc)));
    VK_TRY(ws[WS_TREE].ensure((size_t)S * Wr * sizeof(RAcc)));
    VK_TRY(ws[WS_WIN].ensure((size_t)Wr * msm_tail_plan(S, (uint32_t)Wr, J, nU, Fast29<C>::type::quad, Lseg == 1).slots *
                             sizeof(RAcc)));
    // tail points, then the chain_max word: one read-back
    const size_t tail_bytes = ((size_t)Wr * (J + nU) * sizeof(Acc) + 15) & ~(size_t)15;
    VK_TRY(ws[WS_TAIL].ensure(tail_bytes + 16));

    sl.offsets = ws[WS_OFFSETS].as<uint32_t>();
    sl.tail_bytes = tail_bytes;
    sl.chain_max = sl.chain_dst ? sl.chain_dst : reinterpret_cast<uint32_t*>(ws[WS_TAIL].as<uint8_t>() + tail_bytes);
    sl.through = ws[WS_THROUGH].as<uint8_t>();
    sl.owner_b = ws[WS_OWNER_B].as<uint32_t>();
    sl.buckets = sl.bucket_dst ? sl.bucket_dst : ws[WS_BUCKETS].as<RAcc>();
    sl.carry = ws[WS_CARRY].as<RAcc>();
    sl.owner = ws[WS_OWNER].as<RAcc>();
    sl.seg = ws[WS_SEG].as<RAcc>();
    sl.rs = ws[WS_TREE].as<RAcc>();
    sl.bsum_part = ws[WS_WIN].as<RAcc>();
    sl.tail = ws[WS_TAIL].as<Acc>();

    bool counts_ready = false;
    if (host_timing()) sl.t_launch0 = clock_us();
    if constexpr (std::is_same<C, BLS381G1>::value) {
        if (!sl.radix.sc.empty()) {
            // whole bucket sets over all their windows, whole sort blocks of scalars: the GLV split
            // of set s writes the sort histogram of its bins [s NBC, (s + 1) NBC) itself
            const uint32_t rn = sl.radix.n;
            const int ns = (int)sl.radix.sc.size();
            counts_ready = sl.shared && Wr == ns && sl.wb == 0 && (uint32_t)sl.we == sl.wps * (uint32_t)ns &&
                           nv == 2 * (size_t)rn && rn % chunk == 0 && (size_t)2 * NBC * 4 <= 64 * 1024;
            for (int s2 = 0; s2 < ns; s2++) {
                int32_t* dig = sl.radix.dig + (size_t)s2 * sl.wps * nv;
                if (counts_ready)
                    VK_LAUNCH_ON(ctx, st, "glv_split", (k_glv_radix_hist<BLS381Fr, 5, 16>), rn / chunk, 1024,
                                 (size_t)2 * NBC * 4, sl.radix.sc[s2], sl.radix.inf, rn, sl.radix.mont[s2], glv_consts(),
                                 (int)sl.wps, dig, FB, NBC, nblk, chunk, ws[WS_COUNTS].as<uint32_t>(),
                                 (uint32_t)s2 * NBC, (uint32_t)Wr * NBC);
                else
                    VK_LAUNCH_ON(ctx, st, "glv_split", (k_glv_radix<BLS381Fr, 5, 16>), (rn + 255) / 256, 256, 0,
                                 sl.radix.sc[s2], sl.radix.inf, rn, sl.radix.mont[s2], glv_consts(), (int)sl.wps, dig);
            }
        }
    }
    VK_TRY(sort_entries(ctx, L, src, (uint32_t)nv, c, sl.wb, sl.we, FB, NBC, nblk, chunk, sl.shared ? (sl.stride ? sl.stride : (uint32_t)nv) : 0u,
                        sl.wps, ncnt,
                        ws[WS_COUNTS].as<uint32_t>(),
                        ws[WS_CURSOR].as<uint32_t>(), ws[WS_DIGITS].p, sl.offsets,
                        ws[WS_SORTED].as<uint32_t>(), sl.chain_max, starts, M, p.cstage, counts_ready,
                        sl.shared ? (uint32_t)Wr : 1u));
    // entry count L = offsets[NBtot] stays on the device; grids are sized for L <= nv*W;
    // chain_max was cleared by k_sort_fine
    VK_LAUNCH_ON(ctx, st, "msm_accumulate", (k_msm_accumulate<C, BT>), (Tmax + 255) / 256, 256, 0, bases, phi, nphi,
                 ws[WS_SORTED].as<uint32_t>(), sl.offsets, NBtot, M, sl.buckets, sl.carry, sl.through, sl.owner,
                 sl.owner_b, sl.chain_max, (unsigned long long*)ctx->clk_slot(), starts);
    VK_TRY(msm_tail_fixup_walk<C>(ctx, L, sl.offsets, NBtot, M, sl.buckets, sl.carry, sl.owner, 1u << sl.p.guard,
                                  sl.owner_b, sl.through, Tmax));
    if (sl.skip_reduce) return VC_OK;
    // direct completion: the final stage writes its W (J + nU) points and the chain word straight
    // into the lane's fine-grained page-locked buffer and flags each block; the host polls the flags
    // (slice_finish) -- no read-back copy (a ~4-us blit plus its dispatch) and no stream wake-up
    // (~10-20 us). A lane whose buffer is not fine-grained copies and waits.
    TailDirect td;
    Acc* out = sl.tail;
    sl.direct = false;
    if (L.pin->flags == hipHostMallocCoherent) {
        sl.nflags = (uint32_t)Wr * (J + nU);
        sl.flag_off = tail_bytes + 16;
        VK_TRY(L.pin->ensure(sl.flag_off + (size_t)sl.nflags * 4));
        // (fresh page-locked memory holds anything: no stale flag may match)
        volatile uint32_t* hf = reinterpret_cast<volatile uint32_t*>(static_cast<uint8_t*>(L.pin->p) + sl.flag_off);
        for (uint32_t k = 0; k < sl.nflags; k++) hf[k] = 0;
        sl.epoch = next_epoch(ctx->tail_epoch);
        uint8_t* dbase = static_cast<uint8_t*>(L.pin->dp);
        td.flags = reinterpret_cast<uint32_t*>(dbase + sl.flag_off);
        td.epoch = sl.epoch;
        td.chain_src = sl.chain_max;
        td.chain_dst = reinterpret_cast<uint32_t*>(dbase + tail_bytes);
        out = reinterpret_cast<Acc*>(dbase);
        sl.direct = true;
    }
    VK_TRY(msm_tail_reduce<C>(ctx, L, sl.buckets, sl.offsets, NB, Wr, Lseg, S, J, sl.seg, sl.rs, sl.bsum_part, out,
                              nU > 1, sl.direct ? &td : nullptr));
    return VC_OK;
}

// read back (after every slice has been enqueued: a copy into pageable memory may block the host)
template <class C>
static int slice_fetch(MsmSlice<C>& sl) {
    sl.ht.resize((size_t)sl.Wr * (sl.p.J + sl.p.nU));
    if (sl.direct) return VC_OK;  // written in place by the final stage
    VK_TRY(sl.L.pin->ensure(sl.tail_bytes + 16));
    VK_CHECK_HIP(hipMemcpyAsync(sl.L.pin->p, sl.tail, sl.tail_bytes + 4, hipMemcpyDeviceToHost, sl.L.st));
    return VC_OK;
}

// the wait for a slice's results: its flags at this epoch (direct completion), bounded -- past
// 20 ms (a first launch loading its code, or a fault) the stream wait, which also reports errors
template <class C>
static int slice_wait(const MsmSlice<C>& sl) {
    if (sl.direct) {
        const volatile uint32_t* hf =
            reinterpret_cast<const volatile uint32_t*>(static_cast<const uint8_t*>(sl.L.pin->p) + sl.flag_off);
        const bool seen = poll_bounded([&] {
            uint32_t k = 0;
            while (k < sl.nflags && hf[k] == sl.epoch) k++;
            return k == sl.nflags;
        });
        if (seen) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return VC_OK;
        }
    }
    VK_CHECK_HIP(hipStreamSynchronize(sl.L.st));
    return VC_OK;
}

template <class C>
static int slice_finish(vc_ctx* ctx, MsmSlice<C>& sl, typename C::Acc* res);

// the reduced points of bucket set `set` (shared windows: one MSM each) -> its sum
//   Lseg sum_j 2^j T_j + A,  A = sum_r (r + 1) U_r = sum_k (U_k + ... + U_{nU-1}) (suffix sums)
template <class C>
static typename C::Acc shared_set_sum(const MsmSlice<C>& sl, int set) {
    using Acc = typename C::Acc;
    const uint32_t J = sl.p.J;
    const Acc* ht = sl.ht.data() + (size_t)set * (J + sl.p.nU);
    Acc x = C::zero();  // sum_j 2^j T_j
    for (int j = (int)J - 1; j >= 0; j--) {
        if (!C::is_zero(x)) x = C::dbl(x);
        x = C::add(x, ht[j]);
    }
    Acc r = C::zero();  // Lseg x by double-and-add (Lseg = m for the radix buckets)
    for (int b = 31 - __builtin_clz(sl.p.Lseg); b >= 0; b--) {
        if (!C::is_zero(r)) r = C::dbl(r);
        if ((sl.p.Lseg >> b) & 1) r = C::add(r, x);
    }
    Acc suf = C::zero();
    for (int k = (int)sl.p.nU - 1; k >= 0; k--) {
        suf = C::add(suf, ht[J + k]);
        r = C::add(r, suf);
    }
    return r;
}

template <class C>
static int slice_finish(vc_ctx* ctx, MsmSlice<C>& sl, typename C::Acc* res) {
    using Acc = typename C::Acc;
    VK_TRY(slice_wait<C>(sl));
    memcpy(sl.ht.data(), sl.L.pin->p, sl.ht.size() * sizeof(Acc));
    memcpy(&sl.Lmax, static_cast<const uint8_t*>(sl.L.pin->p) + sl.tail_bytes, 4);
    if (sl.Lmax > (1u << sl.p.guard)) {  // rare (heavily repeated scalars): pointer jumping, redo the tail
        VK_TRY(msm_tail_fixup<C>(ctx, sl.L, sl.p.Tmax, sl.offsets + sl.p.NBtot, sl.p.M, sl.buckets, sl.carry, sl.through,
                                 sl.owner, sl.owner_b, sl.chain_max));
        VK_TRY(msm_tail_reduce<C>(ctx, sl.L, sl.buckets, sl.offsets, sl.p.NB, sl.Wr, sl.p.Lseg, sl.p.S, sl.p.J, sl.seg,
                                  sl.rs, sl.bsum_part, sl.tail, sl.p.nU > 1));
        VK_CHECK_HIP(hipMemcpyAsync(sl.ht.data(), sl.tail, sl.ht.size() * sizeof(Acc), hipMemcpyDeviceToHost,
                                    sl.L.st));
        VK_CHECK_HIP(hipStreamSynchronize(sl.L.st));
    }
    // row-derived totals (TailPlan::urow): the final stage left X = sum of the even-hi row sums in
    // each set's U slot; U = X + T_h (the odd-hi rows)
    const TailPlan tp = msm_tail_plan(sl.p.S, (uint32_t)sl.Wr, sl.p.J, sl.p.nU, Fast29<C>::type::quad, sl.p.Lseg == 1);
    if (tp.urow)
        for (int w = 0; w < sl.Wr; w++) {
            Acc* u = &sl.ht[(size_t)w * (sl.p.J + sl.p.nU) + sl.p.J];
            *u = C::add(*u, sl.ht[(size_t)w * (sl.p.J + sl.p.nU) + tp.h]);
        }
    // slice = sum_w 2^(c w) (A_w + Lseg sum_j 2^j T_wj): Horner over bit positions (host); with
    // shared windows the one bucket set already holds the 2^(c w) factors: A + Lseg sum_j 2^j T_j
    const uint32_t J = sl.p.J;
    if (sl.shared && sl.sets > 1) {  // several MSMs: res[k] = set k's sum
        for (int k = 0; k < sl.sets; k++) res[k] = shared_set_sum<C>(sl, k);
        return VC_OK;
    }
    if (sl.shared) {  // one bucket set: Lseg x (radix buckets: Lseg = m is odd) and the U_r weights
        *res = shared_set_sum<C>(sl, 0);
        return VC_OK;
    }
    const int lg_seg = (int)msm_ceil_log2(sl.p.Lseg);
    const int maxpos = (sl.shared ? 0 : sl.c * (sl.we - 1)) + lg_seg + (int)J;
    std::vector<std::vector<int>> at(maxpos + 1);
    const int st = (int)(J + sl.p.nU);  // reduced points per window: T_0 .. T_{J-1}, then the U sums
    std::vector<Acc> aw(sl.Wr);       // A_w = sum_r (r + 1) U_r by suffix sums (nU = 1: the sum A)
    for (int w = 0; w < sl.Wr; w++) {
        const int p0 = sl.shared ? 0 : sl.c * (sl.wb + w);  // absolute bit position of window wb + w
        Acc a = C::zero(), suf = C::zero();
        for (int k = (int)sl.p.nU - 1; k >= 0; k--) {
            suf = C::add(suf, sl.ht[(size_t)w * st + J + k]);
            a = C::add(a, suf);
        }
        aw[w] = a;
        at[p0].push_back(-1 - w);  // < 0: A_w
        for (uint32_t j = 0; j < J; j++) at[p0 + lg_seg + (int)j].push_back(w * st + (int)j);
    }
    Acc r = C::zero();
    for (int pos = maxpos; pos >= 0; pos--) {
        if (!C::is_zero(r)) r = C::dbl(r);
        for (int idx : at[pos]) r = C::add(r, idx < 0 ? aw[-1 - idx] : sl.ht[idx]);
    }
    *res = r;
    return VC_OK;
}

template <class C, class Fr>
static int msm_run_t(vc_ctx* ctx, Table* t, size_t offset, const uint32_t* d_sc, size_t n,
                     int mont, int part, int parts, uint32_t* out_acc) {
    using Acc = typename C::Acc;
    using Aff = typename C::Aff;
    const double t_entry = host_timing() ? clock_us() : 0.0;  // (phases on stderr; tools/msm_probe.py)
    if (n == 0) {
        Acc z = C::zero();
        memcpy(out_acc, &z, sizeof(Acc));
        return VC_OK;
    }
    if (n >= 0x7fffffffu) return VC_E_INVALID;
    if (parts < 1 || part < 0 || part >= parts) return VC_E_INVALID;
    bool glv = false;
    if constexpr (std::is_same<C, BLS381G1>::value) {
        if (n >= GLV_MIN_N && n < (1u << 30)) VK_TRY(glv_table_ok(ctx, t, &glv));
    }
    const size_t nv = glv ? 2 * n : n;  // MSM terms after the endomorphism split
    VK_TRY(fast_tables<C>(ctx, t, glv));
    const Aff* bases = t->fast.as<Aff>() + offset;  // packed-29 copies (ec29.hpp)
    // shared windows (GLV MSM over the whole table): every window into one bucket set through
    // the 2^(c w) copies of the bases (Table::win, built once; up to 8 GB of HBM). The window
    // size then only trades mixed adds (W per term) against one bucket reduction: c = 19 at
    // 2^21 terms (7 windows instead of 8).
    bool shared = false;
    int top_shift = 0;
    uint32_t radix_m = 1;  // > 1: radix-B shared windows, B = radix_m 2^c
    int c = glv ? glv_window(nv) : choose_window(nv, Fr::BITS + 1);
    if constexpr (std::is_same<C, BLS381G1>::value) {
        const bool shared_env = ctx->opt_shared_windows != 0;  // vc_ctx_set_option(VC_OPT_MSM_SHARED_WINDOWS)
        // Radix-B shared windows (B = 5 x 2^16 ~ 2^18.3, one MSM on one GPU): 7 uniformly loaded
        // windows instead of 8 (B^7 / 2 > 2^127, the GLV halves' bound) -- 12.5 % fewer mixed
        // adds -- into 5 x 2^15 buckets. The power-of-two c = 19 (7 windows) left a 14-bit top
        // window whose digits hit 1 bucket in 16 (chains in the fix-up) and 2^18 buckets to
        // reduce. Window-sliced (multi-GPU) parts keep c = 16: a one-window slice would reduce
        // the whole bucket set for 1/7 of the adds.
        // a point range [offset, offset + n) of >= 2^18 points (one GPU's share of a point-split
        // MSM, vc_msm_device_partial) reads the same whole-table copies, its entries at their table
        // positions (RadixDigits::pt): one copy layout serves whole-table and point-range MSMs
        const bool whole = offset == 0 && n == t->n;
        // ranges down to 2^16 points of a >= 2^18-point table: an eighth of 2^20 on the copies (the
        // 163,840-bucket tail is a fixed cost, but a standalone 2^17-term plan took 1.8 ms against
        // ~0.6: profiles/r04/split_probe*.txt)
        const bool big = whole ? nv >= (1u << 19) : (2 * (size_t)t->n >= (1u << 19) && nv >= (1u << 17));
        if (glv && shared_env && parts == 1 && big) {
            const size_t win_bytes = (size_t)7 * 2 * t->n * 2 * sizeof(typename Fast29<C>::type::AffP);
            if (win_bytes <= (8ull << 30)) {
                const int st = win_tables<C>(ctx, t, 16, 7, 0, 5, true);
                if (st == VC_OK) {
                    shared = true;
                    c = 16;
                    radix_m = 5;
                } else if (st != VC_E_OOM) {
                    return st;
                } else {
                    t->win.release();
                }
            }
        }
        const int cs = glv_window(nv);
        const int Ws = (GLV_BITS + cs - 1) / cs;
        // top window: GLV_BITS - cs (Ws - 1) bits -> digits up to 2^tb; scaled to fill 2^(cs-1)
        const int tb = GLV_BITS - cs * (Ws - 1);
        const int ts = std::max(0, (cs - 1) - tb);
        const size_t win_bytes = (size_t)Ws * 2 * t->n * sizeof(typename Fast29<C>::type::AffN);
        if (!shared && glv && shared_env && offset == 0 && n == t->n && win_bytes <= (8ull << 30)) {
            const int st = win_tables<C>(ctx, t, cs, Ws, ts);
            if (st == VC_OK) {
                shared = true;
                c = cs;
                top_shift = ts;
            } else if (st != VC_E_OOM) {
                return st;
            } else {
                t->win.release();  // out of memory: per-window buckets instead
            }
        }
    }
    // one spare bit absorbs the final carry of the signed recoding
    const int Wfull = radix_m > 1 ? 7 : glv ? (GLV_BITS + c - 1) / c : (Fr::BITS + 1 + c - 1) / c;
    ctx->plan = {c, Wfull, glv ? 2 : 1, (int)radix_m, shared ? 1 : 0};  // vc_msm_last_plan
    // window slice [wb, we) of this call (parts > 1: the MSM split by windows across GPUs;
    // the slices' results add up to the whole MSM)
    const int wb = part * Wfull / parts, we = (part + 1) * Wfull / parts;
    const int W = we - wb;
    // entry counts, offsets, scan counts and sorted positions are u32: nv * W must fit (msm_run
    // cuts larger MSMs into chunks of ctx->opt_msm_chunk points, so this only guards misuse)
    if ((uint64_t)nv * (uint64_t)Wfull >= 0xffffffffull) return VC_E_RANGE;
    if (W == 0) {
        Acc z = C::zero();
        memcpy(out_acc, &z, sizeof(Acc));
        return VC_OK;
    }
    const uint8_t* inf = t->inf.as<uint8_t>() + offset;
    MsmSlice<C> sl;
    sl.L = ctx->lane(0);
    sl.c = c;
    sl.wb = wb;
    sl.we = we;
    sl.W = W;
    sl.shared = shared;
    sl.m = radix_m;
    sl.wps = (uint32_t)Wfull;
    if (!shared && radix_m == 1 && we == Wfull) sl.top_f = top_shortfall(c, glv ? GLV_BITS : Fr::BITS + 1);
    if (glv) {
        if constexpr (std::is_same<C, BLS381G1>::value) {
            VK_TRY(ctx->ws[WS_GLV_SC].ensure(radix_m > 1 ? nv * 4 * (size_t)Wfull : nv * 16));
            uint4* halves = ctx->ws[WS_GLV_SC].as<uint4>();
            const Aff* dphi = t->fast.as<Aff>() + t->n + offset;
            if (radix_m > 1) {  // the split runs in slice_enqueue (sort histogram fused)
                sl.radix.sc = {d_sc};
                sl.radix.mont = {mont};
                sl.radix.inf = inf;
                sl.radix.n = (uint32_t)n;
                sl.radix.dig = ctx->ws[WS_GLV_SC].as<int32_t>();
            } else {
                VK_LAUNCH(ctx, "glv_split", (k_glv_split<Fr>), (n + 255) / 256, 256, 0, d_sc, (uint32_t)n, mont,
                          glv_consts(), halves);
            }
            // [w][2n] limb-form copies: entry w * 2n + i (sort_entries' stride)
            const auto* win = t->win.as<typename Fast29<C>::type::AffN>();
            GlvDigits src{halves, inf, (uint32_t)n};
            if (shared && top_shift > 0) {
                src.tw = Wfull - 1;
                src.ts = top_shift;
            }
            if (radix_m > 1) {  // (the radix copies are in the pair layout)
                RadixDigits rd{ctx->ws[WS_GLV_SC].as<int32_t>(), (uint32_t)nv};
                rd.off = (uint32_t)offset;  // the point range inside the table's copies
                rd.half = (uint32_t)n;
                rd.gap = (uint32_t)(t->n - n);
                sl.stride = (uint32_t)(2 * t->n);
                const auto* wp = t->win.as<typename Fast29<C>::type::AffP>();
                VK_TRY(slice_enqueue<C>(ctx, sl, rd, nv, wp, wp, 0xffffffffu));
            } else if (shared) {  // (power-of-two shared windows: whole tables only)
                VK_TRY(slice_enqueue<C>(ctx, sl, src, nv, win, win, 0xffffffffu));
            } else {
                VK_TRY(slice_enqueue<C>(ctx, sl, src, nv, bases, dphi, (uint32_t)n));
            }
        }
    } else {
        VK_TRY(slice_enqueue<C>(ctx, sl, ScalarDigits<Fr>{d_sc, inf, mont}, nv, bases, bases, 0xffffffffu));
    }
    VK_TRY(slice_fetch<C>(sl));
    const double t_enq = host_timing() ? clock_us() : 0.0;
    if (host_timing()) VK_CHECK_HIP(hipStreamSynchronize(sl.L.st));
    const double t_sync = host_timing() ? clock_us() : 0.0;
    Acc res;
    VK_TRY(slice_finish<C>(ctx, sl, &res));
    // (through the unified Edwards add, which rescales: vc_msm_device_partial hands out these
    // projective words, and they stay what they were when this summed a list of slices)
    res = C::add(C::zero(), res);
    if (host_timing())
        fprintf(stderr, "msm_host n=%zu first_launch_us=%.1f enqueue_us=%.1f wait_us=%.1f fold_us=%.1f\n", n,
                sl.t_launch0 - t_entry, t_enq - t_entry, t_sync - t_enq, clock_us() - t_sync);
    memcpy(out_acc, &res, sizeof(Acc));
    return VC_OK;
}

// K MSMs over one whole table (e.g. a KZG commitment and its opening proof over the Lagrange
// SRS): one pipeline for all K -- the radix digits of every scalar set, ONE sort into K bucket
// sets (bucket set k of entry (k, w, i) names the same window copy B^w P_i), one accumulate
// launch, one fix-up and one reduction over the K sets -- so the latency-bound tail and the
// launch gaps are paid once, not K times. Only the radix shared-window geometry (BLS12-381, GLV,
// whole table from 2^18 points) batches; other tables run the K MSMs one by one.
template <class C, class Fr>
static int msm_run_many_t(vc_ctx* ctx, Table* t, const void* const* d_sc, const int* mont, size_t n, size_t K,
                          uint32_t* out_accs) {
    using Acc = typename C::Acc;
    bool batched = false;
    if constexpr (std::is_same<C, BLS381G1>::value) {
        bool glv = false;
        if (K > 1 && n == t->n && n >= (1u << 18) && n < (1u << 30) && ctx->opt_shared_windows != 0 &&
            (uint64_t)2 * n * 7 * std::min<size_t>(K, 8) < 0xffffffffull)
            VK_TRY(glv_table_ok(ctx, t, &glv));
        if (glv) {
            VK_TRY(fast_tables<C>(ctx, t, true));
            const int st = win_tables<C>(ctx, t, 16, 7, 0, 5, true);
            if (st == VC_E_OOM) t->win.release();
            else if (st != VC_OK) return st;
            batched = st == VC_OK;
        }
        if (batched) {
            const size_t nv = 2 * n;
            const int Ws = 7;
            // up to 8 bucket sets per pipeline (the sort's LDS histogram holds 8 x 1280 coarse bins)
            for (size_t k0 = 0; k0 < K; k0 += 8) {
                const size_t Kb = std::min<size_t>(8, K - k0);
                if (Kb == 1) {
                    VK_TRY(msm_run(ctx, t, 0, d_sc[k0], n, mont[k0], out_accs + k0 * (sizeof(Acc) / 4)));
                    continue;
                }
                VK_TRY(ctx->ws[WS_GLV_SC].ensure(nv * 4 * (size_t)Ws * Kb));
                MsmSlice<C> sl;
                sl.L = ctx->lane(0);
                sl.c = 16;
                sl.m = 5;
                sl.shared = true;
                sl.sets = (int)Kb;
                sl.wps = (uint32_t)Ws;
                sl.wb = 0;
                sl.we = Ws * (int)Kb;
                sl.W = sl.we;
                sl.radix.inf = t->inf.as<uint8_t>();
                sl.radix.n = (uint32_t)n;
                sl.radix.dig = ctx->ws[WS_GLV_SC].as<int32_t>();
                for (size_t k = k0; k < k0 + Kb; k++) {  // the GLV split of every set runs in slice_enqueue
                    sl.radix.sc.push_back(static_cast<const uint32_t*>(d_sc[k]));
                    sl.radix.mont.push_back(mont[k]);
                }
                const auto* wp = t->win.as<typename Fast29<C>::type::AffP>();  // (radix copies: the pair layout)
                VK_TRY(slice_enqueue<C>(ctx, sl, RadixDigits{sl.radix.dig, (uint32_t)nv}, nv, wp, wp, 0xffffffffu));
                VK_TRY(slice_fetch<C>(sl));
                std::vector<Acc> res(Kb);
                VK_TRY(slice_finish<C>(ctx, sl, res.data()));
                memcpy(out_accs + k0 * (sizeof(Acc) / 4), res.data(), Kb * sizeof(Acc));
            }
            ctx->plan = {16, Ws, 2, 5, 1};
            return VC_OK;
        }
    }
    for (size_t k = 0; k < K; k++)
        VK_TRY(msm_run(ctx, t, 0, d_sc[k], n, mont[k], out_accs + k * (sizeof(Acc) / 4)));
    return VC_OK;
}

int msm_run_many(vc_ctx* ctx, Table* t, const void* const* d_sc, const int* mont, size_t n, size_t K, uint32_t* out) {
    switch (t->curve) {
        case VC_CURVE_BN254:
            return msm_run_many_t<BN254G1, BN254Fr>(ctx, t, d_sc, mont, n, K, out);
        case VC_CURVE_BLS12_381:
            return msm_run_many_t<BLS381G1, BLS381Fr>(ctx, t, d_sc, mont, n, K, out);
        case VC_CURVE_BANDERSNATCH:
            return msm_run_many_t<Bandersnatch, BandFr>(ctx, t, d_sc, mont, n, K, out);
    }
    return VC_E_INVALID;
}
int msm_windows(int curve, size_t n, int* c, int* W, int* terms) {
    int bits = curve == VC_CURVE_BN254 ? BN254Fr::BITS : curve == VC_CURVE_BLS12_381 ? BLS381Fr::BITS : BandFr::BITS;
    // BLS12-381 tables of subgroup points take the GLV split (2n terms of 127-bit scalars)
    const bool glv = curve == VC_CURVE_BLS12_381 && n >= GLV_MIN_N && n < (1u << 30);
    // (a GLV MSM over a whole table takes the shared-window size, msm_run_t)
    *c = glv ? glv_window(2 * n) : choose_window(n, bits + 1);
    *W = glv ? (GLV_BITS + *c - 1) / *c : (bits + 1 + *c - 1) / *c;
    if (terms) *terms = glv ? 2 : 1;
    return VC_OK;
}

// MSMs of more than ctx->opt_msm_chunk points (default 2^27: nv * W then stays below 2^31 on
// every curve, so the u32 entry space of the sort cannot wrap) run as consecutive point chunks
// whose accumulators are added on the host; each chunk is an ordinary partial-table MSM.
template <class C, class Fr>
static int msm_run_chunked(vc_ctx* ctx, Table* t, size_t offset, const uint32_t* sc, size_t n, int mont,
                           int part, int parts, uint32_t* out_acc) {
    using Acc = typename C::Acc;
    const size_t chunk = std::max<size_t>(ctx->opt_msm_chunk, 1);
    if (n <= chunk) return msm_run_t<C, Fr>(ctx, t, offset, sc, n, mont, part, parts, out_acc);
    Acc res = C::zero();
    for (size_t lo = 0; lo < n; lo += chunk) {
        const size_t m = std::min(chunk, n - lo);
        Acc r;
        VK_TRY((msm_run_t<C, Fr>(ctx, t, offset + lo, sc + 8 * lo, m, mont, part, parts,
                                 reinterpret_cast<uint32_t*>(&r))));
        res = C::add(res, r);
    }
    memcpy(out_acc, &res, sizeof(Acc));
    return VC_OK;
}

// chunked host-scalar MSM: chunk j's buckets added into the running set (first: empty buckets
// set to the identity, so the one reduction after the last chunk reads every bucket as live)
template <class A>
__global__ void __launch_bounds__(256) k_bucket_merge(typename A::Acc* __restrict__ acc,
                                                     const typename A::Acc* __restrict__ add,
                                                     const uint32_t* __restrict__ offsets, uint32_t NBtot,
                                                     uint32_t first) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= NBtot) return;
    const bool ne = offsets[b + 1] > offsets[b];
    if (first) {
        if (!ne) acc[b] = A::zero();
    } else if (ne) {
        acc[b] = A::add(acc[b], add[b]);
    }
}
__global__ void k_iota(uint32_t* __restrict__ o, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) o[i] = i;
}

// vc_msm with host scalars (the drop-in `commit` of INTEGRATION.md over utils.rs:16-19): the
// 32 n bytes cross PCIe in K chunks on the side stream while the context's stream runs the
// previous chunk -- each chunk a point-range MSM on the table's radix shared-window copies (GLV
// split + histogram, sort, accumulate, fix-up) whose buckets add into one set -- and ONE
// reduction + host fold finish it. Only for that geometry (BLS12-381, GLV, radix copies);
// *done = false otherwise (the caller copies and runs msm_run). A chunk whose fix-up chains
// exceed its walk (adversarial scalars) sends the whole MSM to msm_run_t once the scalars are in.
template <class C, class Fr>
static int msm_run_host_chunks_t(vc_ctx* ctx, Table* t, size_t offset, const uint64_t* host_sc, size_t n, int mont,
                                 int K, uint32_t* out_acc, bool* done) {
    *done = false;
    if constexpr (!std::is_same<C, BLS381G1>::value) {
        return VC_OK;
    } else {
        using Acc = typename C::Acc;
        using A = typename Fast29<C>::type;
        using RAcc = FAcc<C>;
        if (K < 2 || K > 4 || n >= (1u << 30) || !ctx->opt_shared_windows || 2 * (size_t)t->n < (1u << 19))
            return VC_OK;
        // chunks of whole 8192-scalar sort blocks, each >= 2^16 points (a point range on the copies)
        const size_t blk = 8192, nb = (n + blk - 1) / blk;
        if (nb < (size_t)K || n / K < (1u << 16)) return VC_OK;
        bool glv = false;
        VK_TRY(glv_table_ok(ctx, t, &glv));
        if (!glv) return VC_OK;
        VK_TRY(fast_tables<C>(ctx, t, true));
        {
            const size_t win_bytes = (size_t)7 * 2 * t->n * 2 * sizeof(typename A::AffP);
            if (win_bytes > (8ull << 30)) return VC_OK;
            const int st = win_tables<C>(ctx, t, 16, 7, 0, 5, true);
            if (st == VC_E_OOM) {
                t->win.release();
                return VC_OK;
            }
            VK_TRY(st);
        }
        ctx->plan = {16, 7, 2, 5, 1};
        const uint32_t NB = 5u << 15;
        std::vector<size_t> lo(K + 1);
        for (int j = 0; j <= K; j++) lo[j] = std::min(n, (nb * j / K) * blk);
        size_t nmax = 0;
        for (int j = 0; j < K; j++) nmax = std::max(nmax, lo[j + 1] - lo[j]);
        VK_TRY(ctx->ws[WS_SCALARS].ensure(n * 32));
        VK_TRY(ctx->ws[WS_GLV_SC].ensure(2 * nmax * 4 * 7));
        VK_TRY(ctx->ws[WS_BUCKETS].ensure((size_t)NB * sizeof(RAcc)));
        VK_TRY(ctx->ws2[WS_BUCKETS].ensure((size_t)NB * sizeof(RAcc)));
        VK_TRY(ctx->ws2[WS_CHAIN].ensure(16));
        VK_TRY(ctx->ws2[WS_OFFSETS].ensure(((size_t)NB + 1) * 4));
        uint8_t* d_sc = ctx->ws[WS_SCALARS].as<uint8_t>();
        RAcc* bA = ctx->ws[WS_BUCKETS].as<RAcc>();
        RAcc* bB = ctx->ws2[WS_BUCKETS].as<RAcc>();
        uint32_t* chain = ctx->ws2[WS_CHAIN].as<uint32_t>();
        std::vector<hipEvent_t> ev(K);
        for (int j = 0; j < K; j++) ev[j] = ctx->get_event();
        // on every exit (errors included): no copy still reading the caller's buffer, events back
        struct Done {
            vc_ctx* ctx;
            std::vector<hipEvent_t>& ev;
            ~Done() {
                (void)hipStreamSynchronize(ctx->side_stream);
                for (hipEvent_t e : ev) ctx->event_pool.push_back(e);
            }
        } done_guard{ctx, ev};
        MsmSlice<C> sl;
        std::vector<uint32_t> guard(K);
        for (int j = 0; j < K; j++) {
            const size_t nj = lo[j + 1] - lo[j];
            // chunk j's scalars on the side stream, issued after chunk j - 1's kernels are queued (a
            // pageable copy can block the host until its data is staged)
            VK_CHECK_HIP(hipMemcpyAsync(d_sc + lo[j] * 32, host_sc + lo[j] * 4, nj * 32, hipMemcpyHostToDevice,
                                        ctx->side_stream));
            VK_CHECK_HIP(hipEventRecord(ev[j], ctx->side_stream));
            VK_CHECK_HIP(hipStreamWaitEvent(ctx->stream, ev[j], 0));
            sl = MsmSlice<C>();
            sl.L = ctx->lane(0);
            sl.c = 16;
            sl.wb = 0;
            sl.we = 7;
            sl.W = 7;
            sl.shared = true;
            sl.m = 5;
            sl.wps = 7;
            sl.bucket_dst = j == 0 ? bA : bB;
            sl.chain_dst = chain + j;
            sl.skip_reduce = true;
            sl.radix.sc = {reinterpret_cast<const uint32_t*>(d_sc + lo[j] * 32)};
            sl.radix.mont = {mont};
            sl.radix.inf = t->inf.as<uint8_t>() + offset + lo[j];
            sl.radix.n = (uint32_t)nj;
            sl.radix.dig = ctx->ws[WS_GLV_SC].as<int32_t>();
            RadixDigits rd{ctx->ws[WS_GLV_SC].as<int32_t>(), (uint32_t)(2 * nj)};
            rd.off = (uint32_t)(offset + lo[j]);
            rd.half = (uint32_t)nj;
            rd.gap = (uint32_t)(t->n - nj);
            sl.stride = (uint32_t)(2 * t->n);
            const auto* wp = t->win.as<typename A::AffP>();  // (radix copies: the pair layout)
            VK_TRY(slice_enqueue<C>(ctx, sl, rd, 2 * nj, wp, wp, 0xffffffffu));
            guard[j] = sl.p.guard;
            VK_LAUNCH(ctx, "msm_merge", (k_bucket_merge<A>), (NB + 255) / 256, 256, 0, bA, bB, sl.offsets, NB,
                      j == 0 ? 1u : 0u);
        }
        // one reduction over the merged set: every bucket live (empty ones hold the identity)
        uint32_t* iota = ctx->ws2[WS_OFFSETS].as<uint32_t>();
        VK_LAUNCH(ctx, "msm_iota", k_iota, (NB + 1 + 255) / 256, 256, 0, iota, NB);
        VK_TRY(msm_tail_reduce<C>(ctx, sl.L, bA, iota, sl.p.NB, sl.Wr, sl.p.Lseg, sl.p.S, sl.p.J, sl.seg, sl.rs, sl.bsum_part,
                                  sl.tail, sl.p.nU > 1));
        // the tail buffer's own chain word (read by slice_finish) was not used by the chunks
        VK_CHECK_HIP(hipMemsetAsync(reinterpret_cast<uint8_t*>(sl.tail) + sl.tail_bytes, 0, 4, ctx->stream));
        VK_TRY(slice_fetch<C>(sl));
        uint32_t hchain[4] = {0, 0, 0, 0};
        VK_CHECK_HIP(hipMemcpyAsync(hchain, chain, 4 * K, hipMemcpyDeviceToHost, ctx->stream));
        VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        for (int j = 0; j < K; j++)
            if (hchain[j] > (1u << guard[j])) {  // long chains: the unchunked MSM over the copied scalars
                *done = true;
                return msm_run_t<C, Fr>(ctx, t, offset, reinterpret_cast<const uint32_t*>(d_sc), n, mont, 0, 1,
                                        out_acc);
            }
        Acc res;
        VK_TRY(slice_finish<C>(ctx, sl, &res));
        memcpy(out_acc, &res, sizeof(Acc));
        *done = true;
        return VC_OK;
    }
}

// vc_msm: host scalars
int msm_run_host(vc_ctx* ctx, Table* t, size_t offset, const uint64_t* host_sc, size_t n, int mont,
                 uint32_t* out_acc) {
    if (t->curve == VC_CURVE_BLS12_381 && ctx->opt_host_chunks > 1 && ctx->opt_msm_chunk >= n) {
        bool done = false;
        VK_TRY((msm_run_host_chunks_t<BLS381G1, BLS381Fr>(ctx, t, offset, host_sc, n, mont, ctx->opt_host_chunks,
                                                          out_acc, &done)));
        if (done) return VC_OK;
    }
    if (n > 0) {
        VK_TRY(ctx->ws[WS_SCALARS].ensure(n * 32));
        VK_CHECK_HIP(hipMemcpyAsync(ctx->ws[WS_SCALARS].p, host_sc, n * 32, hipMemcpyHostToDevice, ctx->stream));
    }
    return msm_run(ctx, t, offset, ctx->ws[WS_SCALARS].p, n, mont, out_acc, 0, 1);
}

int msm_run(vc_ctx* ctx, Table* t, size_t offset, const void* d_scalars, size_t n, int mont,
            uint32_t* out_acc, int part, int parts) {
    const uint32_t* sc = reinterpret_cast<const uint32_t*>(d_scalars);
    switch (t->curve) {
        case VC_CURVE_BN254:
            return msm_run_chunked<BN254G1, BN254Fr>(ctx, t, offset, sc, n, mont, part, parts, out_acc);
        case VC_CURVE_BLS12_381:
            return msm_run_chunked<BLS381G1, BLS381Fr>(ctx, t, offset, sc, n, mont, part, parts, out_acc);
        case VC_CURVE_BANDERSNATCH:
            return msm_run_chunked<Bandersnatch, BandFr>(ctx, t, offset, sc, n, mont, part, parts, out_acc);
    }
    return VC_E_INVALID;
}

}  // namespace vk

// The MSM's host-side plans: window sizes, the geometry of one window slice (msm_slice_plan) and of
// its tail's bit stage (msm_tail_plan). Pure functions of the shape -- no HIP types, no environment
// -- so tests/cpp/slice_plan_check.cpp and tail_plan_check.cpp pin them without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace vk {
// smallest k with 2^k >= x
inline uint32_t msm_ceil_log2(uint64_t x) {
    uint32_t k = 0;
    while (k < 63 && (1ull << k) < x) k++;
    return k;
}
// GLV halves are < 2^127: window sizes whose top window still spans most of its digit range
// (16 -> 8 windows, top 15 of 16 bits; 13 -> 10, top 10; 10 -> 13, top 7). A nearly empty
// top window (c = 15 leaves 7 bits, c = 14 one) piles all its entries into a few buckets:
// one fine-sort block and long fix-up chains (measured 0.25 + 0.23 ms at 2^16 with c = 15).
inline int glv_window(size_t nv) {
    if (nv >= (1u << 19)) return 16;
    if (nv >= (1u << 15)) return 13;
    return 10;
}
// shared windows (msm_run_t): a short top window's digits are scaled to span the bucket range
// (GlvDigits::ts), so c need not divide 128. Measured at 2^21 terms: c = 19 (7 windows) cuts
// the accumulate by 0.3-0.45 ms but its 2^18-bucket reduction, the top window's hot buckets in
// the fix-up and the sort give it all back (3.61 vs 3.60 ms) -- c = 16 stays.
// bits of the top window of `total` digit bits cut into c-bit windows, as a shortfall: the top
// window's digits fall into 2^-(shortfall) of its bucket set
inline int top_shortfall(int c, int total) {
    const int W = (total + c - 1) / c;
    return c - (total - c * (W - 1));
}
// window bits of a per-window (non-GLV) MSM of n terms whose signed digits cover `total` bits
// (scalar bits + 1). The size rule alone gave BN254 (255 bits) top windows of 2 bits at c = 11
// and 8 of 13 at c = 13: a 4096-term MSM piled all its top digits into 2 of 1,024 buckets,
// chains of ~256 pieces, so every call redid its fix-up by pointer jumping and the reduction
// (+0.37 ms of a 0.7 ms MSM, the multiproof verifier's). A size whose top window is short by more
// than 2 bits is replaced by the cheapest of c - 5 .. c + 2 (W n mixed adds + 2 W 2^(c-1)
// reduction adds) that is not.
inline int choose_window(size_t n, int total) {
    int c0 = 5;
    if (n >= (1u << 19)) c0 = 16;
    else if (n >= (1u << 17)) c0 = 15;
    else if (n >= (1u << 15)) c0 = 13;
    else if (n >= (1u << 12)) c0 = 11;
    else if (n >= (1u << 9)) c0 = 9;
    else if (n >= 64) c0 = 7;
    if (top_shortfall(c0, total) <= 2) return c0;
    int best = c0;
    double best_cost = 0.0;
    for (int c = std::max(4, c0 - 5); c <= std::min(16, c0 + 2); c++) {
        if (top_shortfall(c, total) > 2) continue;
        const double W = (total + c - 1) / c;
        const double cost = W * (double)n + 2.0 * W * (double)(1u << (c - 1));
        if (best == c0 || cost < best_cost) best = c, best_cost = cost;
    }
    return best;
}
// items per lane of the bit-sum stage: the smallest K in [2, 32] whose busy waves (a wave per
// `lanes` K items of each of the W (J + 1) sums) fit one wave per SIMD (1024): a wave costs K +
// log2(lanes) serial adds (its butterfly included) and a SIMD's second wave doubles its time, so
// fewer, longer waves win until every SIMD has one (measured: 1192 busy waves at K = 7 took 2x the
// 960 of K = 8 on a GLV 2^20 MSM). lanes = logical lanes per wave (64; 16 for quads of the
// cooperative add, SW29::add_quad -- not used here: with every SIMD busy the stage is issue-bound,
// and quads' 2.1x shorter adds lose to their 4x fewer lanes)
inline uint32_t msm_bitsum_k(uint32_t S, uint32_t W, uint32_t J, uint32_t lanes = 64, uint32_t nU = 1) {
    for (uint32_t k = 2; k < 32; k++) {
        const uint64_t per = (uint64_t)lanes * k;
        const uint64_t busy = (uint64_t)W * ((uint64_t)J * ((S / 2 + per - 1) / per) + nU * ((S + per - 1) / per));
        if (busy <= 1024) return k;
    }
    return 32;
}
// waves (= partial slots) of one bit-stage sum over `items` items (K per logical lane)
inline uint32_t msm_bitsum_pw(uint32_t items, uint32_t K, uint32_t lanes = 64) {
    return (items + lanes * K - 1) / (lanes * K);
}
// Geometry of the bit stage. Bit form (h = 0): J sums T_j over S/2 items each (nb1 waves per
// sum) + nU sums U over S items (nb2 waves). Marginal form (h > 0, J >= 12): with s = G hi + lo
// (G = 2^h, Hn = 2^(J-h) high values) the stage instead makes the G column sums L_lo = sum_hi
// R_(G hi + lo) (Hn items) and the Hn row sums H_hi = sum_lo R_(G hi + lo) (G items), each by one
// wave, plus the U sums as before; the final stage then reads T_j = sum over lo with bit j of L_lo
// (j < h) or over hi with bit j - h of H_hi (j >= h) -- the same T_j from 2 S + ~S adds instead of
// J S / 2. per_w = partial slots per set (the WS_WIN layout).
// Row-derived total (urow, marginal form with nU = 1 and Lseg = 1, where U = sum_s R_s is the
// total of the row sums): no U waves; the final stage sums X = the H_hi of even hi (Hn / 2 items, as
// every T_j >= h) and the host adds T_h (the odd hi) to it. The column sums may then take pL waves
// each (Hn / pL items per wave, pL <= Hn / G, so the T_j < h sums still read <= Hn / 2 partials).
// Packed marginal waves (gL, gH > 1, several sets on quads): a wave makes gL column sums (or gH row
// sums) on 64 / g lanes each, so the column / row waves carry as many items per lane as the U waves
// and leave room for them in one round (the one-call KZG's two radix sets: 2 x (64 + 64 + 5 x 64)
// waves of 8 items instead of the bit form's 13). Partial slots stay one per sum (`slots` per set;
// per_w counts waves).
struct TailPlan {
    uint32_t h = 0, K = 0, nb1 = 0, nb2 = 0, per_w = 0, pL = 1, gL = 1, gH = 1, slots = 0;
    bool urow = false;
};
// Chosen by a cost model in full-add times: a wave costs its K serial adds plus the in-wave
// butterfly (7 quad adds ~ 3.5 full adds; 6 full adds without quads), and a stage whose waves fit
// one round (<= 1024, a wave per SIMD) takes its longest wave. The marginal form is taken only
// within one round and when shorter: measured on one MI355X, the 2^20 radix MSM's one set 10.5 ->
// 7.5 units, 0.165 -> 0.118 ms; the 8-way window slice 8.5 -> 7.5, 0.121 -> 0.107 ms. Stacked
// rounds do not follow the model (8 and 16 windows of 2^13 segments, 1744+ waves of 1-5 items
// per lane: 0.170 -> 0.198 and 0.139 -> 0.179 ms), so several sets keep the bit form.
inline TailPlan msm_tail_plan(uint32_t S, uint32_t W, uint32_t J, uint32_t nU, bool quad = true,
                              bool u_total = false) {
    const double bf = quad ? 3.5 : 6.0;
    TailPlan p;
    p.K = msm_bitsum_k(S, W, J, 64, nU);
    p.nb1 = msm_bitsum_pw(S / 2, p.K);
    p.nb2 = msm_bitsum_pw(S, p.K);
    p.per_w = J * p.nb1 + nU * p.nb2;
    p.slots = p.per_w;
    if (!(J >= 12 && S == (1u << J))) return p;
    if ((uint64_t)W * p.per_w > 1024) return p;
    const uint32_t h = J / 2, G = 1u << h, Hn = 1u << (J - h), kl = Hn / 64;  // Hn >= G >= 64
    double best = p.K + bf;
    for (uint32_t k = kl; k <= 32; k++) {  // U sums: no fewer items per lane than the L waves
        const uint32_t nb = msm_bitsum_pw(S, k);
        if ((uint64_t)W * (G + Hn + nU * nb) > 1024) continue;
        const double t = k + bf;  // one round: the longest wave (k >= kl >= G / 64)
        if (t < best - 1e-9) {
            best = t;
            p.h = h;
            p.K = k;
            p.nb1 = 0;
            p.nb2 = nb;
            p.per_w = G + Hn + nU * nb;
            p.slots = p.per_w;
        }
    }
    if (quad && W > 1) {  // several sets: pack 2-4 column / row sums per wave
        for (uint32_t k = kl; k <= 32; k++) {
            uint32_t gL = 1, gH = 1;
            while (gL < 16 && Hn * (gL * 2) / 64 <= k) gL *= 2;  // items per lane of a column wave <= k
            while (gH < 16 && G * (gH * 2) / 64 <= k) gH *= 2;
            if (gL == 1 && gH == 1) continue;  // the plain marginal form above
            const uint32_t nb = msm_bitsum_pw(S, k);
            const uint32_t waves = G / gL + Hn / gH + nU * nb;
            if ((uint64_t)W * waves > 1024) continue;
            const double t = k + bf;
            if (t < best - 1e-9) {
                best = t;
                p.h = h;
                p.K = k;
                p.nb1 = 0;
                p.nb2 = nb;
                p.gL = gL;
                p.gH = gH;
                p.per_w = waves;
                p.slots = G + Hn + nU * nb;
            }
        }
    }
    if (u_total && nU == 1) {  // U from the row sums (u_total: the U items are the R_s)
        for (uint32_t pl = 1; pl <= Hn / G; pl *= 2) {
            if ((uint64_t)W * (G * pl + Hn) > 1024) break;
            const uint32_t k = std::max(Hn / (64 * pl), G / 64);
            const double t = k + bf;
            if (t < best + 1e-9) {  // ties too: no U waves, and X reads half the U sum's partials
                best = t;
                p.h = h;
                p.K = k;
                p.nb1 = 0;
                p.nb2 = 0;
                p.pL = pl;
                p.gL = p.gH = 1;
                p.urow = true;
                p.per_w = G * pl + Hn;
                p.slots = p.per_w;
            }
        }
    }
    return p;
}
// guarded rounds for nv entries over NB buckets per window at M entries per thread: covers a
// bucket of 4x the mean load (the top window of a GLV split uses half its buckets: 2x)
inline uint32_t msm_fixup_guard_rounds(size_t nv, uint32_t NB, uint32_t M) {
    const size_t chain = 4 * nv / ((size_t)NB * M) + 2;
    return std::min<uint32_t>(6, std::max<uint32_t>(1, msm_ceil_log2(chain)));
}
// sorted entries per accumulate thread: 64 at 2^20 x 16 windows (2 rounds of 2048 waves),
// fewer for window slices / small MSMs so the grid still fills the chip
// (not below 16: a bucket then straddles more threads and the fix-up's serial merge chain
// costs more than the emptier accumulate rounds -- measured at 2 windows of 2^20)
inline uint32_t msm_entries_per_thread(size_t maxL) {
    return (uint32_t)std::min<size_t>(64, std::max<size_t>(16, maxL / 131072));
}
// One window slice [wb, we) of an MSM of nv terms (msm.hip MsmSlice): W windows of c bits in the
// slice (shared: sets x windows per set, all into `sets` bucket sets), m > 1: radix m 2^c digits,
// top_f: the top window's shortfall if it is in the slice, m_override > 0: M as given (a probe),
// sort_chunk: scalars per sort block of the plain digit sources (msm_sort.hpp SORT_CHUNK).
struct SliceShape {
    size_t nv = 0;
    int c = 0, W = 0, wb = 0, we = 0, sets = 1, top_f = 0;
    bool shared = false;
    uint32_t m = 1, m_override = 0, sort_chunk = 1024;
};
// Its geometry: M entries per accumulate thread (Tmax threads), NB buckets per set (NBtot in all)
// in S = 2^J reduction segments of Lseg, nU sums per set after the J bit sums (A, or the Lseg
// residue sums U_r); the sort's 2^FB fine buckets per coarse bin (NBC bins per set), nblk blocks of
// `chunk` scalars, ncnt counters, the staged coarse scatter (cstage); guard: see below.
struct SlicePlan {
    uint32_t M, Lseg, S, J, nU, Tmax, NB, NBtot, FB, chunk, NBC, nblk, guard;
    bool cstage;
    size_t ncnt;
};
inline SlicePlan msm_slice_plan(const SliceShape& sh) {
    const size_t nv = sh.nv;
    const int c = sh.c, W = sh.W;
    const int Wr = sh.shared ? sh.sets : W;  // bucket sets
    const uint32_t NB = sh.m << (c - 1);
    const uint32_t NBtot = NB * (uint32_t)Wr;
    const size_t maxL = nv * (size_t)W;
    const size_t load = maxL / Wr;  // entries per bucket set
    uint32_t M = msm_entries_per_thread(maxL);
    // ... and at least twice the mean bucket load, so few buckets straddle more than two
    // threads (the GLV 2^20 MSM has 64 entries per bucket: M = 128 drops the fix-up's
    // pointer-jumping rounds, 0.23 -> 0.06 ms, for 0.1 ms more accumulate)
    if (load / NB > M / 2 && M < 128) M *= 2;
    // shared windows: the fix-up is a lane per bucket, so M just fills one round of two waves
    // per SIMD (131072 lanes)
    if (sh.shared) M = (uint32_t)std::max<size_t>(16, (maxL + 131071) / 131072);
    if (sh.m_override) M = sh.m_override;
    // buckets per reduction segment (the segment sum is a serial chain of 2*Lseg adds): 4, or 2
    // when the segments (one lane each) would not give every SIMD a wave (GLV 2^20: 4 at 8
    // windows, 2 for the 1-4 window slices of multi-GPU runs; 8 measured 0.1-0.15 ms slower)
    uint32_t Lseg = NB >= 64 ? 4 : (NB >= 4 ? 2 : 1);
    if (Lseg == 4 && (size_t)(NB / Lseg) * Wr < 65536) Lseg = 2;
    // one bucket set: the bit sums straight over 2^15 buckets (measured), segments of 4 at 2^18;
    // radix m 2^c: segments of m buckets (S = 2^(c-1) segments)
    if (sh.shared) Lseg = sh.m > 1 ? sh.m : (NB >= (1u << 17) ? 4 : 1);
    const uint32_t S = NB / Lseg;  // power of two
    const uint32_t J = msm_ceil_log2(S);
    // shared windows with segments: the residue form of the reduction (msm_tail.hip k_msm_segr)
    // per-window bucket sets too, up to 8 of them: the segment stage's 2 Lseg dependent adds become Lseg - 1 for Lseg more U sums in the bit
    // stage. Measured (`profiles/r03/probes/residue_perwin/`): the GLV variable-base 2^20 MSM (8 sets)
    // tail 0.436 -> 0.38 ms; 16-20 sets (BN254, Bandersnatch) 0.05-0.16 ms slower, so they keep acc_s
    const bool resid_sets = sh.shared || Wr <= 8;
    const uint32_t nU = (Lseg > 1 && resid_sets) ? Lseg : 1;
    const uint32_t Tmax = (uint32_t)((maxL + M - 1) / M);

    // bucket sort geometry (k_sort_*): 2^FB fine buckets per coarse bin
    const uint32_t lgNB = (uint32_t)c - 1;  // NB = m 2^lgNB
    uint32_t FB = lgNB < 8 ? lgNB : 8;
    uint32_t chunk = sh.sort_chunk;
    if (sh.m > 1) {
        // radix buckets (5 x 2^15 at 2^21 x 7 entries): FB = 7 keeps the coarse entries narrow
        // (entry index < 7 x 2^21 < 2^24), i.e. 1280 coarse bins; blocks of 8192 scalars keep a
        // block's runs ~45 entries long
        FB = lgNB < 7 ? lgNB : 7;
        chunk = 8192;
    }
    // radix buckets: the staged coarse scatter (k_sort_coarse_st) holds a block's chunk x W entries in
    // LDS, so the chunk is the largest power of two that fits 152 KB beside the 2 x bins counters
    bool cstage = false;
    if (sh.m > 1 && sh.shared) {
        // one coarse launch per bucket set (sort_entries): a block stages one set's windows
        const uint64_t bins_l = (uint64_t)(NB >> FB);
        const uint32_t Wl = (uint32_t)W / (uint32_t)Wr;
        const uint64_t room = (152u * 1024 / 4 > 2 * bins_l + 1) ? 152u * 1024 / 4 - 2 * bins_l - 1 : 0;
        uint32_t ch = 1u << 12;
        while (ch > 1024 && (uint64_t)ch * Wl > room) ch >>= 1;
        if ((uint64_t)ch * Wl <= room) {  // 4096 scalars for one set and for each of several
            chunk = ch;
            cstage = true;
        }
    }
    // per-window buckets: one more coarse bit when the fine bins would be too big to stage in LDS
    // (GLV variable-base 2^21 x 8: 16K -> 8K entries; fine pass 0.118 -> 0.041 ms)
    if (sh.m == 1 && !sh.shared && FB > 1 && load / (NB >> FB) > 12000) FB--;
    // shared windows: ~64K entries per coarse bin (one 1024-thread k_sort_fine block each) but at
    // least 256 bins (a fine block per CU). Measured at 2^21 x 8 entries (hist + coarse + fine):
    // 0.233 ms at 2^14 entries per bin (256-thread fine blocks), 0.222 at 2^15, 0.204 at 2^16,
    // 0.295 at 2^17 -- bigger bins shorten the scatter's partial-line writes
    while (sh.shared && sh.m == 1 && FB > 1 && (load >> 16) > (size_t)(NB >> FB)) FB--;
    while (sh.shared && sh.m == 1 && FB > 1 && (NB >> FB) < 256) FB--;
    const uint32_t NBC = NB >> FB;
    const uint32_t nblk = (uint32_t)((nv + chunk - 1) / chunk);
    // the staged coarse pass pays for its LDS sort and write-out with >= 4096 entries per block and
    // either runs of >= 10 entries per bin (radix: 22, or 11 with two sets) or LDS <= 64 KB (two or
    // more blocks per CU: GLV variable-base 2^21 x 8, 4-entry runs, 0.129 -> 0.106 ms). Measured
    // slower: BN254 2^20 (16 windows, 98 KB, 0.119 -> 0.169 ms) and the 8-way window slice (1024
    // entries per block, 0.016 -> 0.029 ms)
    if (sh.m == 1) {
        const uint64_t per_blk = (uint64_t)chunk * (uint32_t)(sh.we - sh.wb), bins_all = (uint64_t)Wr * NBC;
        const uint64_t lds_b = (2 * bins_all + 1 + per_blk) * 4;
        cstage = per_blk >= 4096 && (per_blk >= 10 * bins_all || lds_b <= 64 * 1024);
    }
    const size_t ncnt = (size_t)Wr * NBC * nblk + 1;
    // chains up to 2^guard carry pieces are walked serially by their owners; longer ones
    // (adversarial scalars) take the pointer-jumping path in slice_finish
    // (a top window short by f bits loads its buckets 2^f times the mean)
    uint32_t guard = msm_fixup_guard_rounds(sh.shared ? load : load << sh.top_f, NB, M);
    // shared windows: a short top window's digits load 2^-tb of the buckets several times the
    // mean (c = 19: ~310 entries vs 56), so the walk takes chains of up to 16 pieces
    if (sh.shared) guard = std::max<uint32_t>(guard, 4);
    return SlicePlan{M, Lseg, S, J, nU, Tmax, NB, NBtot, FB, chunk, NBC, nblk, guard, cstage, ncnt};
}
}  // namespace vk

// Batched fixed-base commits: thousands of width-w commitments against one small CRS
// (IPA::commit ipa/mod.rs:130-135 at N = 256; verkle Node::gen_commitment node.rs:243-271;
// the commit phase of prove_multiproof multiproof.rs:151,168). Config 3 of BASELINE.json.
//
// MI355X-first design: the bases never change, so each base G_i has a window table
// T[i][w][k] = (k+1) * 2^(c*w) * G_i in HBM (fb_table.hip). A commit is then sum over (i, w) of
// +-T[i][w][|d_iw|-1]: W mixed adds per base, no doublings, no buckets. Two schedules:
// throughput (large batches: persistent equal runs of (commit, base) items, one resident
// round, piece combine, split normalisation: normalize.hip) and latency (small batches such as the
// IPA prover's L/R: per-window threads, wave/LDS fold, host combine + normalisation).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <vector>

#include "commit_internal.hpp"
#include "ec29.hpp"

namespace vk {

// ------------------------------------------------------------------ the batched commit
// Chunk-major runs: the width is cut into nch chunks of <= K bases and run r = chunk * batch + g
// adds commit g's items of chunk `chunk`. The 64 lanes of a wave are 64 commits at the same base
// and window, so each gather instruction stays inside one (base, window) block of the table
// (3 MB at c = 16) instead of touching 64 blocks spread over the whole table (GBs): far fewer
// distinct pages per instruction, and the identity-base skip is wave-uniform.
template <class C, class Fr>
__global__ void __launch_bounds__(256) VK_COMMIT_OCC k_fb_commit_cm(const FbE<C>* __restrict__ tab,
                                                     const uint8_t* __restrict__ inf, uint32_t width,
                                                     FbGeom fg, const uint32_t* __restrict__ sc,
                                                     uint32_t batch, int mont, uint32_t K, uint32_t nruns,
                                                     typename Fast29<C>::type::Acc* __restrict__ piece) {
    using FC = typename Fast29<C>::type;
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nruns) return;
    const uint32_t chunk = r / batch, g = r - chunk * batch;
    const int W = fg.W;
    const uint32_t i0 = chunk * K, i1 = min(i0 + K, width);
    typename FC::Acc acc = FC::zero();
    for (uint32_t i = i0; i < i1; i++) {
        if (inf[i]) continue;
        FbDigits<Fr> dg;
        dg.s = load_scalar_fb<Fr>(sc, (size_t)g * width + i);
        if (mont) dg.s = fe_from_mont<Fr>(dg.s);
        const FbE<C>* ti = tab + (size_t)i * fg.stride();
        int32_t dn = dg.next(fg.width(0));
        typename FC::Aff Pn = ti[dn != 0 ? (uint32_t)(dn < 0 ? -dn : dn) - 1 : 0].u;
        for (int w = 0; w < W; w++) {
            const int32_t d = dn;
            const typename FC::Aff P = Pn;
            if (w + 1 < W) {
                dn = dg.next(fg.width(w + 1));
                Pn = ti[fg.off(w + 1) + (dn != 0 ? (uint32_t)(dn < 0 ? -dn : dn) - 1 : 0)].u;
            }
            if (d != 0) acc = FC::madd(acc, P, d < 0);
        }
    }
    piece[r] = acc;
}

// commit g = sum over chunks of the raw pieces piece[chunk * batch + g]: a thread per commit
// (coalesced across g) for large batches, or a wave per commit (lanes fold a strided share,
// then an xor butterfly) for small ones, which the chip spreads over up to `width` chunks per
// commit: a serial chain of 257 adds cost ~2 ms (IPA prover rounds)
template <class C>
__global__ void __launch_bounds__(256) k_fb_combine_cm(const typename Fast29<C>::type::Acc* __restrict__ piece,
                                                      uint32_t nch, uint32_t batch, typename C::Acc* __restrict__ out) {
    using FC = typename Fast29<C>::type;
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= batch) return;
    typename FC::Acc acc = piece[g];
    for (uint32_t k = 1; k < nch; k++) acc = FC::add(acc, piece[(size_t)k * batch + g]);
    out[g] = FC::store(acc);
}
// G = 2^lgG lanes per commit (consecutive lanes of one wave): each folds a strided share of the
// nch pieces, then lgG xor levels -- ceil(nch / G) + lgG serial adds. G grows while the lanes
// still fit one wave per SIMD: 10k width-256 commits (13 chunks) take 4 lanes each, 5 adds
// instead of the 12 of a thread per commit on 157 waves
template <class C>
__global__ void __launch_bounds__(256) k_fb_combine_grp(const typename Fast29<C>::type::Acc* __restrict__ piece,
                                                       uint32_t nch, uint32_t batch, uint32_t lgG,
                                                       typename C::Acc* __restrict__ out) {
    using FC = typename Fast29<C>::type;
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, g = gid >> lgG, j = gid & ((1u << lgG) - 1);
    const uint32_t G = 1u << lgG, nk = (nch + G - 1) / G;
    typename FC::Acc v = FC::zero();
    for (uint32_t it = 0; it < nk + lgG; it++) {  // one add call site; every lane runs the shuffles
        typename FC::Acc o;
        if (it < nk) {
            const uint32_t k = j + it * G;
            o = (g < batch && k < nch) ? piece[(size_t)k * batch + g] : FC::zero();
        } else {
            o = shfl_xor_pod(v, 1u << (it - nk));
        }
        v = FC::add(v, o);
    }
    if (g < batch && j == 0) out[g] = FC::store(v);
}
template <class C>
__global__ void __launch_bounds__(64) k_fb_combine_wave(const typename Fast29<C>::type::Acc* __restrict__ piece,
                                                       uint32_t nch, uint32_t batch, typename C::Acc* __restrict__ out) {
    using FC = typename Fast29<C>::type;
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    uint32_t span = 1, lg = 0;
    while (span < nch && span < 64) {
        span <<= 1;
        lg++;
    }
    const uint32_t nk = (nch + 63) / 64;
    typename FC::Acc v = FC::zero();
    for (uint32_t it = 0; it < nk + lg; it++) {  // one add call site
        typename FC::Acc o;
        if (it < nk) {
            const uint32_t k = lane + it * 64;
            o = k < nch ? piece[(size_t)k * batch + g] : FC::zero();
        } else {
            o = shfl_xor_pod(v, 1u << (it - nk));
        }
        v = FC::add(v, o);
    }
    if (lane == 0) out[g] = FC::store(v);
}
// ---- latency path for small batches (the IPA prover's L/R, multiproof D/E): every thread
// adds the table points of WPT windows of one base, then a wave butterfly and an LDS step
// fold the block to one partial; the host adds a commit's few block partials.
// Serial depth WPT + 8 + blocks-per-commit adds instead of W + width (persistent path at K = 1).
// windows per thread of the latency path. 1 is best by far (IPA prover L/R, width 257, c = 8:
// 111 us per launch vs 469 / 658 us at 2 / 4): a lone wave executing a mixed add's ~25 KB of
// straight-line code once runs on cold instruction-cache misses, so any serial madd beyond the
// first costs ~0.35 ms; one (base, window) point per thread leaves only the looped butterfly.
// The host side relies on it being 1: a commit's threads are its width x W (base, window) pairs
// (the kernel's WG == W), in fb_is_small and in the launch's blocks per commit.
constexpr int FB_WPT = 1;
static_assert(FB_WPT == 1, "fb_is_small and fb_commit_t's bpc count one window per thread");

// A strided base pattern of compacted rows (the IPA rounds' L / R on their N / 2 + 1 non-zero
// bases: measured slower and removed, commit f54c503 has the callers). Every launch passes half = 0,
// item i is base i. The argument and its select stay in the kernel: without them the BLS12-381
// instantiation allocates 271 VGPRs + 15 AGPRs against 270 + 14 (profiles/r11/knobs/kernels.md).
struct StrideCols {
    uint32_t half = 0, m = 0, off_even = 0, off_odd = 0, n_main = 0, extra = 0;
    __host__ __device__ uint32_t base(uint32_t g, uint32_t i) const {
        return i < n_main ? (i / half) * m + ((g & 1) ? off_odd : off_even) + i % half : extra;
    }
};

template <class C, class Fr>
__global__ void __launch_bounds__(256) k_fb_commit_small(const FbE<C>* __restrict__ tab,
                                                        const uint8_t* __restrict__ inf, uint32_t width, FbGeom fg,
                                                        const uint32_t* __restrict__ sc, int mont,
                                                        uint32_t bpc, int wpt, StrideCols cols, IpaRows ipa,
                                                        typename C::Acc* __restrict__ part,
                                                        uint32_t* __restrict__ flags, uint32_t epoch) {
    using FC = typename Fast29<C>::type;
    const uint32_t g = blockIdx.x / bpc, blk = blockIdx.x % bpc;
    const int W = fg.W;
    const uint32_t WG = (uint32_t)(W + wpt - 1) / wpt;
    const uint32_t j = blk * 256 + threadIdx.x;
    const uint32_t i = j / WG, wg = j % WG;
    typename FC::Acc fa = FC::zero();
    const uint32_t base = cols.half ? cols.base(g, i) : i;
    // the IPA rows (IpaRows): this round's coefficient of item i, folded and stored by L's window-0
    // thread for the next round -- identity bases included -- then the item's scalar
    fe<Fr> ipa_s = fe_zero<Fr>();
    if (ipa.a != nullptr && i < width) {
        const uint32_t p = g >> 1;
        if (i < ipa.N) {
            fe<Fr> c = load_scalar_fb<Fr>(ipa.coeff_in, (size_t)p * ipa.N + i);
            if (ipa.fold && (i % ipa.m_prev) < ipa.h_prev) c = fe_mul<Fr>(c, load_scalar_fb<Fr>(ipa.x, p));
            if ((g & 1) == 0 && wg == 0) {
                uint4* o = reinterpret_cast<uint4*>(ipa.coeff_out + 8 * ((size_t)p * ipa.N + i));
                o[0] = make_uint4(c.v[0], c.v[1], c.v[2], c.v[3]);
                o[1] = make_uint4(c.v[4], c.v[5], c.v[6], c.v[7]);
            }
            const uint32_t jj = i % ipa.m;
            const bool on = (g & 1) ? jj < ipa.h : jj >= ipa.h;
            if (on)
                ipa_s = fe_mul<Fr>(load_scalar_fb<Fr>(ipa.a, (size_t)p * ipa.N + ((g & 1) ? jj + ipa.h : jj - ipa.h)), c);
        } else {
            ipa_s = load_scalar_fb<Fr>(ipa.q, g);
        }
    }
    if (i < width && !inf[base]) {
        FbDigits<Fr> dg;
        dg.s = ipa.a != nullptr ? ipa_s : load_scalar_fb<Fr>(sc, (size_t)g * width + i);
        if (mont) dg.s = fe_from_mont<Fr>(dg.s);
        const FbE<C>* ti = tab + (size_t)base * fg.stride();
        const int wb = (int)wg * wpt, we = min(W, wb + wpt);
        for (int w = 0; w < we; w++) {
            const int32_t d = dg.next(fg.width(w));
            if (w >= wb && d != 0) fa = FC::madd(fa, ti[fg.off(w) + (uint32_t)(d < 0 ? -d : d) - 1].u, d < 0);
        }
    }
    fb_block_sum_store<C>(fa, &part[blockIdx.x]);
    // zero-copy completion: the block's partial (written by thread 0 above) is made visible system
    // wide, then its flag takes this launch's epoch -- the host polls the flags instead of waiting
    // for the stream (fb_commit_t)
    if (flags != nullptr && threadIdx.x == 0) {
        __threadfence_system();
        __hip_atomic_store(&flags[blockIdx.x], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// lanes resident in one round for a kernel (occupancy x CUs x block)
template <class Kern>
static uint32_t resident_lanes(Kern k, int block) {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, block, 0) != hipSuccess) return 0;
    return (uint32_t)(cus * per_cu * block);
}

// ------------------------------------------------------------------ host drivers
// resident lanes of k_fb_commit_cm on this context's device (cached per ctx: the Guard's mutex
// serialises it), and whether `batch` commits of `width` items over W windows take the latency
// path: the one text of that choice, for the commit (fb_commit_t) and for the IPA prover's choice
// of device rows (fb_small_path)
template <class C>
static size_t fb_lanes(vc_ctx* ctx) {
    if (!ctx->fb_lanes) ctx->fb_lanes = resident_lanes(k_fb_commit_cm<C, ScalarOf<C>>, 256);
    return ctx->fb_lanes ? ctx->fb_lanes : 131072;
}
static bool fb_is_small(size_t lanes, size_t width, size_t batch, size_t W) {
    return batch <= 64 && batch * width * W <= lanes;
}

template <class C>
static int fb_commit_t(vc_ctx* ctx, Table* t, size_t width, const void* d_sc, size_t batch, int mont,
                       void* d_out_xy, uint8_t* d_out_inf, uint64_t* h_out_xy, uint8_t* h_out_inf, bool* on_host,
                       const PinBuf* pin_sc, const std::function<void()>* overlap, const IpaRows* ipa) {
    using Acc = typename C::Acc;
    using Fr = ScalarOf<C>;
    if (width > t->n) return VC_E_RANGE;
    if (t->fb_c == 0) {
        int c = fb_default_c<Fr>(t->n, ctx->fb_auto_used());
        int st = fixed_base_precompute(ctx, t, c);
        while (st == VC_E_OOM && c > 8) {  // another context or caller took the memory: narrower
            (void)hipGetLastError();
            st = fixed_base_precompute(ctx, t, --c);
        }
        VK_TRY(st);
        t->fb_auto = true;
    }
    if (batch == 0) {
        if (overlap && *overlap) (*overlap)();
        return VC_OK;
    }
    VK_TRY(ctx->ws[WS_OUT].ensure(batch * sizeof(Acc)));
    const size_t items = batch * width;
    const size_t lanes = fb_lanes<C>(ctx);
    const FbGeom fg = t->fb_geom();
    const size_t W = (size_t)fg.W;
    const bool small = fb_is_small(lanes, width, batch, W);
    if (ipa && !small) return VC_E_INVALID;  // IPA rows: the latency path only
    if (ipa && (width != (size_t)ipa->N + 1 || batch % 2)) return VC_E_INVALID;
    // zero-copy on the latency path: the kernel reads host-pinned scalars and writes its block
    // partials to fine-grained host memory over PCIe instead of a copy engine moving them before /
    // after it
    if (pin_sc) {
        if (small) {
            d_sc = pin_sc->dp;
        } else {
            VK_TRY(ctx->ws[WS_SCALARS].ensure(items * 32));
            VK_CHECK_HIP(hipMemcpyAsync(ctx->ws[WS_SCALARS].p, pin_sc->p, items * 32, hipMemcpyHostToDevice,
                                        ctx->stream));
            d_sc = ctx->ws[WS_SCALARS].p;
        }
    }
    if (small) {  // small batch: latency path
        const uint32_t bpc = (uint32_t)((width * W + 255) / 256);
        // host_timing(): launch-to-readback, host adds and normalisation on stderr
        const bool timing = host_timing();
        const double t0 = timing ? clock_us() : 0.0;
        const size_t part_bytes = (size_t)batch * bpc * sizeof(Acc);
        const uint32_t nblk = (uint32_t)(batch * bpc);
        // zero-copy partials: the blocks' completion flags follow them in the fine-grained buffer
        const size_t flag_off = (part_bytes + 63) / 64 * 64;
        VK_TRY(ctx->pin_small.ensure(flag_off + (size_t)nblk * 4));
        Acc* d_part = static_cast<Acc*>(ctx->pin_small.dp);
        volatile uint32_t* hflags = reinterpret_cast<volatile uint32_t*>(static_cast<uint8_t*>(ctx->pin_small.p) + flag_off);
        uint32_t* dflags = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ctx->pin_small.dp) + flag_off);
        const uint32_t epoch = next_epoch(ctx);
        // (fresh page-locked memory holds anything: no stale flag may match)
        for (uint32_t b = 0; b < nblk; b++) hflags[b] = 0;
        VK_LAUNCH(ctx, "fb_commit_small", (k_fb_commit_small<C, Fr>), batch * bpc, 256, 0, t->fb.as<FbE<C>>(),
                  t->inf.as<uint8_t>(), (uint32_t)width, fg, reinterpret_cast<const uint32_t*>(d_sc), mont,
                  bpc, FB_WPT, StrideCols{}, ipa ? *ipa : IpaRows{}, d_part, dflags, epoch);
        // the few block partials are added and normalised on the host: a lone GPU lane pays
        // ~10 us per serial EC add and ~160 us per field inversion, the host ~1 us / ~20 us
        // (pinned read-back; a caller that wants host results -- h_out_xy -- gets them without the
        // upload / second read-back round trip)
        const Acc* parts = ctx->pin_small.as<Acc>();
        if (overlap && *overlap) (*overlap)();
        // the partials serially on this thread (the host pool's wake-up cost more than the ~23 us
        // of adds of the IPA prover's 2 x 33 partials: prove 0.89 -> 1.07 ms); each block's partial
        // is added as soon as its flag arrives, so the adds overlap the blocks that finish later.
        // Then one batched inversion.
        std::vector<Acc> sums(batch);
        std::vector<uint8_t> done(nblk, 0), have(batch, 0);
        uint32_t ndone = 0;
        // every block's flag at this epoch: the partials are in host memory. Bounded: past 20 ms (a
        // first launch loading its code, or a fault) wait for the stream, which also reports any error
        const bool seen = poll_bounded([&] {
            for (uint32_t b = 0; b < nblk; b++) {
                if (done[b] || hflags[b] != epoch) continue;
                std::atomic_thread_fence(std::memory_order_acquire);
                const uint32_t g = b / bpc;
                sums[g] = have[g] ? C::add(sums[g], parts[b]) : parts[b];
                have[g] = 1;
                done[b] = 1;
                ndone++;
            }
            return ndone == nblk;
        });
        const double t1 = timing ? clock_us() : 0.0;
        if (!seen) {  // the poll gave up: the stream's end, and the sums from the start
            VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
            std::atomic_thread_fence(std::memory_order_acquire);
            for (size_t g = 0; g < batch; g++) {
                Acc a = parts[g * bpc];
                for (uint32_t b = 1; b < bpc; b++) a = C::add(a, parts[g * bpc + b]);
                sums[g] = a;
            }
        }
        const int nl = (int)(C::F::N / 2);
        std::vector<uint64_t> oxy(h_out_xy ? 0 : (size_t)batch * 2 * nl);
        std::vector<uint8_t> oinf(h_out_xy ? 0 : batch);
        uint64_t* rxy = h_out_xy ? h_out_xy : oxy.data();
        uint8_t* rinf = h_out_xy ? h_out_inf : oinf.data();
        const double t2 = timing ? clock_us() : 0.0;
        VK_TRY(acc_to_affine_batch(ctx->curve, reinterpret_cast<const uint32_t*>(sums.data()), batch, rxy, rinf));
        if (timing)
            fprintf(stderr, "[fb_small] %zu x %u partials: launch..last flag (adds overlapped) %.1f us, rest %.1f us, affine %.1f us\n",
                    batch, bpc, t1 - t0, t2 - t1, clock_us() - t2);
        if (h_out_xy) {
            *on_host = true;
            return VC_OK;
        }
        VK_CHECK_HIP(hipMemcpyAsync(d_out_xy, oxy.data(), oxy.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        VK_CHECK_HIP(hipMemcpyAsync(d_out_inf, oinf.data(), batch, hipMemcpyHostToDevice, ctx->stream));
        VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));  // host staging vectors die on return
        return VC_OK;
    }
    // chunk-major: the chunk count minimising rounds-of-resident-lanes x items-per-run
    // (fewest chunks on ties: fewer pieces to combine)
    size_t K = width, best = SIZE_MAX;
    for (size_t nc = 1; nc <= width; nc++) {
        const size_t k = (width + nc - 1) / nc;
        if ((width + k - 1) / k != nc) continue;  // same K as a smaller chunk count
        const size_t cost = ((nc * batch + lanes - 1) / lanes) * k;
        if (cost < best) best = cost, K = k;
    }
    const size_t nch = (width + K - 1) / K;
    const size_t nruns = nch * batch;
    if (nruns >= (1ull << 31)) return VC_E_RANGE;
    VK_TRY(ctx->ws[WS_PIECE].ensure(nruns * sizeof(typename Fast29<C>::type::Acc)));
    VK_LAUNCH(ctx, "fb_commit", (k_fb_commit_cm<C, Fr>), (nruns + 255) / 256, 256, 0,
              t->fb.as<FbE<C>>(), t->inf.as<uint8_t>(), (uint32_t)width, fg,
              reinterpret_cast<const uint32_t*>(d_sc), (uint32_t)batch, mont, (uint32_t)K, (uint32_t)nruns,
              ctx->ws[WS_PIECE].as<typename Fast29<C>::type::Acc>());
    // serial adds per SIMD: a thread per commit (nch adds, batch / 64 waves) vs a wave per commit
    // (ceil(nch / 64) + log2 adds, batch waves) -- 1024 SIMDs
    size_t lg = 0;
    while ((1ull << lg) < std::min<size_t>(nch, 64)) lg++;
    const size_t cost_thread = nch * ((batch + 65535) / 65536);
    const size_t cost_wave = ((batch + 1023) / 1024) * ((nch + 63) / 64 + lg);
    // lanes per commit: grow while there are pieces to split and the lanes fit a wave per SIMD
    uint32_t lgG = 0;
    while (lgG < 6 && (2ull << lgG) <= nch && batch * (2ull << lgG) <= 65536) lgG++;
    if (lgG > 0 && lgG < 6)
        VK_LAUNCH(ctx, "fb_combine", (k_fb_combine_grp<C>), (uint32_t)(((batch << lgG) + 255) / 256), 256, 0,
                  ctx->ws[WS_PIECE].as<typename Fast29<C>::type::Acc>(), (uint32_t)nch, (uint32_t)batch, lgG,
                  ctx->ws[WS_OUT].as<Acc>());
    else if (cost_thread <= cost_wave)
        VK_LAUNCH(ctx, "fb_combine", (k_fb_combine_cm<C>), (batch + 255) / 256, 256, 0,
                  ctx->ws[WS_PIECE].as<typename Fast29<C>::type::Acc>(), (uint32_t)nch, (uint32_t)batch,
                  ctx->ws[WS_OUT].as<Acc>());
    else
        VK_LAUNCH(ctx, "fb_combine", (k_fb_combine_wave<C>), batch, 64, 0,
                  ctx->ws[WS_PIECE].as<typename Fast29<C>::type::Acc>(), (uint32_t)nch, (uint32_t)batch,
                  ctx->ws[WS_OUT].as<Acc>());
    if (overlap && *overlap) (*overlap)();
    return normalize_to_canon(ctx, t->curve, ctx->ws[WS_OUT].p, batch, d_out_xy, d_out_inf);
}

template <class C>
static bool fb_small_path_t(vc_ctx* ctx, Table* t, size_t width, size_t batch) {
    using Fr = ScalarOf<C>;
    size_t W = (size_t)t->fb_W;
    if (!t->fb_c) {  // before the default tables exist: the geometry fb_commit_t will build
        const int c = fb_default_c<Fr>(t->n, ctx->fb_auto_used());
        W = (size_t)(Fr::BITS + 1 + c - 1) / c;
    }
    return fb_is_small(fb_lanes<C>(ctx), width, batch, W);
}
bool fb_small_path(vc_ctx* ctx, Table* t, size_t width, size_t batch) {
    if (t->curve != ctx->curve || batch == 0 || batch > 64) return false;
    switch (t->curve) {
        case VC_CURVE_BN254: return fb_small_path_t<BN254G1>(ctx, t, width, batch);
        case VC_CURVE_BLS12_381: return fb_small_path_t<BLS381G1>(ctx, t, width, batch);
        case VC_CURVE_BANDERSNATCH: return fb_small_path_t<Bandersnatch>(ctx, t, width, batch);
    }
    return false;
}

int msm_batch_run(vc_ctx* ctx, Table* t, size_t width, const void* d_sc, size_t batch, int mont,
                  void* d_out_xy, uint8_t* d_out_inf, uint64_t* h_out_xy, uint8_t* h_out_inf, bool* on_host,
                  const PinBuf* pin_sc, const std::function<void()>* overlap,
                  const IpaRows* ipa) {
    bool dummy = false;
    if (!on_host) on_host = &dummy;
    *on_host = false;
    if (h_out_xy && !h_out_inf) return VC_E_INVALID;
#define VK_FB_COMMIT_(C) \
    fb_commit_t<C>(ctx, t, width, d_sc, batch, mont, d_out_xy, d_out_inf, h_out_xy, h_out_inf, on_host, pin_sc, overlap, ipa)
    switch (t->curve) {
        case VC_CURVE_BN254: return VK_FB_COMMIT_(BN254G1);
        case VC_CURVE_BLS12_381: return VK_FB_COMMIT_(BLS381G1);
        case VC_CURVE_BANDERSNATCH: return VK_FB_COMMIT_(Bandersnatch);
    }
#undef VK_FB_COMMIT_
    return VC_E_INVALID;
}

}  // namespace vk

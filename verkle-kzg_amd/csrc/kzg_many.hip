// KZG batch proving (vc_kzg_prove_many): n openings, each KZG::prove_point (kzg/mod.rs:136-154) of
// one of `rows` data rows at its own point, one proof each. The rows are uploaded and converted to
// Montgomery form once and stay resident; per chunk of at most 16,384 openings:
//   lane    k_kzg_many_lane, a lane per opening: the point's class (in the domain at m / outside) and
//           D = z^N - 1 for the openings outside (zero for the others);
//   invert  batch_inverse over the chunk's D (zeros stay zero), one host round trip -- skipped when
//           every opening of the chunk is in the domain;
//   wave    k_kzg_many_wave, a wave per opening, four to a block: the quotient row (Montgomery, the
//           layout msm_batch_run reads) and y (canonical);
//   commit  msm_batch_run over the quotient rows (commit.hip, its own latency / throughput choice,
//           a first-use fixed-base table as vc_msm_batch builds one).
// The arithmetic is csrc/kzg_many.hpp, the text tests/cpp/kzg_many_check.cpp runs on the host. Every
// status other than VC_OK is decided on the host before the first upload. The workspace beside the
// resident rows is sized by the chunk, not by n.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ctx.hpp"
#include "ec29.hpp"
#include "host/fr.hpp"
#include "host/pool.hpp"
#include "kzg_many.hpp"
#include "poly.hpp"
#include "scheme_internal.hpp"

namespace vk {

using namespace kzgm;

constexpr uint32_t KM_BLOCK = 256;  // four waves, four openings
constexpr size_t KM_CHUNK_MAX = 16384;

// points: canonical words (F::N per opening, below r: the host has checked). cls[i] = m or
// KM_OUTSIDE; D[i] = z^N - 1 (Montgomery) outside the domain, zero in it.
template <class F>
__global__ __launch_bounds__(KM_BLOCK) void k_kzg_many_lane(const uint32_t* __restrict__ points, uint32_t N, int lgN,
                                                            uint32_t n, uint32_t* __restrict__ cls,
                                                            fe<F>* __restrict__ D) {
    const uint32_t i = blockIdx.x * KM_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t zw[F::N];
    for (int k = 0; k < F::N; k++) zw[k] = points[(size_t)F::N * i + k];
    const uint32_t c = classify<F>(zw, N);
    cls[i] = c;
    D[i] = c == KM_OUTSIDE ? vanishing<F>(fe_to_mont<F>(words_load<F>(zw)), lgN) : fe_zero<F>();
}

// Wave w of the grid takes opening w < n: row row[w] (row == nullptr: row `first + w`) of f (rows of
// `width` Montgomery values), the point points[w], its class cls[w], D[w] = z^N - 1 and dinv[w] =
// 1 / D[w]. pw, inv1: the domain's cached tables. q: n rows of N Montgomery values; y: n canonical values. The branch
// is per wave.
template <class F>
__global__ __launch_bounds__(KM_BLOCK, 4) void k_kzg_many_wave(const fe<F>* __restrict__ f, uint32_t width,
                                                            const uint32_t* __restrict__ row, uint32_t first,
                                                            const uint32_t* __restrict__ points,
                                                            const uint32_t* __restrict__ cls,
                                                            const fe<F>* __restrict__ D,
                                                            const fe<F>* __restrict__ dinv,
                                                            const fe<F>* __restrict__ pw,
                                                            const fe<F>* __restrict__ inv1, fe<F> n_inv, uint32_t N,
                                                            uint32_t n, fe<F>* q, fe<F>* __restrict__ y) {
    // (the wave's index through readfirstlane: the compiler then knows the opening, its row, its
    // class and the branch below to be uniform, and keeps their addresses out of the vector registers)
    const uint32_t o = blockIdx.x * (KM_BLOCK / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    if (o >= n) return;
    const fe<F>* fr = f + (size_t)(row ? row[o] : first + o) * width;
    fe<F>* qr = q + (size_t)o * N;
    const uint32_t c = cls[o];
    if (c != KM_OUTSIDE) {
        const uint32_t m = c;
        const fe<F> fm = row_at<F>(fr, width, m);
        const fe<F> wminv = pw[(N - m) & (N - 1)];
        fe<F> acc = in_pass<F>(fr, width, pw, inv1, N, m, fm, wminv, lane, qr);
        for (uint32_t s = 1; s < 64; s <<= 1) acc = fe_add<F>(acc, shfl_xor_pod(acc, s));
        if (lane == (m & 63u)) qr[m] = in_qm<F>(wminv, acc);
        if (lane == 0) y[o] = fe_from_mont<F>(fm);
        return;
    }
    uint32_t zw[F::N];
    for (int k = 0; k < F::N; k++) zw[k] = points[(size_t)F::N * o + k];
    const fe<F> z = fe_to_mont<F>(words_load<F>(zw));
    fe<F> tot = out_prefix_pass<F>(pw, N, z, lane, qr);
    fe<F> oth = fe_one<F>();
    for (uint32_t s = 1; s < 64; s <<= 1) {
        const fe<F> pt = shfl_xor_pod(tot, s);
        others_step<F>(tot, oth, pt);
    }
    // (tot is D on every lane now; D[o] is read again after the pass instead of kept through it)
    fe<F> acc = out_inverse_pass<F>(fr, width, pw, N, z, fe_mul<F>(oth, dinv[o]), lane, qr);
    for (uint32_t s = 1; s < 64; s <<= 1) acc = fe_add<F>(acc, shfl_xor_pod(acc, s));
    const fe<F> yv = out_y<F>(D[o], n_inv, acc);
    out_quotient_pass<F>(fr, width, N, yv, lane, qr);
    if (lane == 0) y[o] = fe_from_mont<F>(yv);
}

namespace {

struct Args {
    int table;
    size_t N, rows, width;
    const void* data;
    bool d_data;
    const uint32_t* row;
    const uint64_t* points;
    size_t n;
    uint64_t* proof_xy;
    uint8_t* proof_inf;
    uint64_t* y;
};

template <class C_, class F>
int prove_many_t(vc_ctx* ctx, Table* t, const Args& a) {
    const size_t N = a.N, n = a.n, width = a.width;
    int lgN = 0;
    while ((size_t(1) << lgN) < N) lgN++;
    const uint32_t* pts32 = reinterpret_cast<const uint32_t*>(a.points);
    // ---- every status but VC_OK, before any GPU work
    if (a.row)
        for (size_t i = 0; i < n; i++)
            if (a.row[i] >= a.rows) return VC_E_INVALID;
    std::vector<uint8_t> outside(n);
    std::atomic<int> bad{0};  // 1: a point >= r; 2: a domain error
    pool_for(0, n, 1024, [&](size_t i) {
        uint32_t c = 0;
        const int st = point_status<F>(pts32 + (size_t)F::N * i, (uint32_t)N, lgN, &c);
        if (st == VC_OK) outside[i] = c == KM_OUTSIDE;
        else bad |= st == VC_E_INVALID ? 1 : 2;
    });
    if (bad & 1) return VC_E_INVALID;
    if (bad & 2) return VC_E_DOMAIN;

    size_t chunk = KM_CHUNK_MAX;
    // VKZG_KZG_PROVE_CHUNK (read per call): a test forces small chunks
    if (const char* e = getenv("VKZG_KZG_PROVE_CHUNK"))
        if (atol(e) > 0) chunk = std::min<size_t>((size_t)atol(e), KM_CHUNK_MAX);
    chunk = std::min(chunk, n);
    const bool timing = host_timing();
    const double call0 = timing ? clock_us() : 0.0;
    hipStream_t st = ctx->stream;
    const size_t xyb = (size_t)C_::F::N * 8;  // canonical affine x, y

    // the rows, resident for the call
    DevBuf d_f(ctx);
    {
        const size_t cells = a.rows * width;
        VK_TRY(d_f.ensure(std::max<size_t>(cells, 1) * sizeof(fe<F>)));
        if (cells) {
            DevBuf raw(ctx);
            const void* src = a.data;
            if (!a.d_data) {
                VK_TRY(raw.ensure(cells * sizeof(fe<F>)));
                VK_CHECK_HIP(hipMemcpyAsync(raw.p, a.data, cells * sizeof(fe<F>), hipMemcpyHostToDevice, st));
                src = raw.p;
            }
            VK_TRY(canon_to_mont_dev<F>(ctx, src, cells, cells, d_f.as<fe<F>>()));
        }
    }
    const fe<F> omega = group_gen_t<F>(N, fr_generator<F>());
    const fe<F>*pw = nullptr, *inv1 = nullptr;
    VK_TRY(domain_tables<F>(ctx, omega, N, &pw, nullptr, &inv1));
    const fe<F> n_inv = fe_inv_bin<F>(mont_from_u64<F>(N));

    DevBuf d_q(ctx), d_pts(ctx), d_row(ctx), d_cls(ctx), d_D(ctx), d_y(ctx), d_out(ctx);
    VK_TRY(d_q.ensure(chunk * N * sizeof(fe<F>)));
    VK_TRY(d_pts.ensure(chunk * sizeof(fe<F>)));
    VK_TRY(d_row.ensure(chunk * 4));
    VK_TRY(d_cls.ensure(chunk * 4));
    VK_TRY(d_D.ensure(2 * chunk * sizeof(fe<F>)));  // D | 1 / D
    VK_TRY(d_y.ensure(chunk * sizeof(fe<F>)));
    VK_TRY(d_out.ensure(chunk * (xyb + 1)));        // the proofs, then their identity flags
    fe<F>* d_Dv = d_D.as<fe<F>>();
    fe<F>* d_Dinv = d_Dv + chunk;
    uint8_t* d_xy = d_out.as<uint8_t>();
    uint8_t* d_inf = d_xy + chunk * xyb;

    double lap_up = 0, lap_lane = 0, lap_inv = 0, lap_wave = 0, lap_commit = 0, lap_back = 0;
    size_t nchunks = 0;
    auto lap = [&](double& into, double& since) -> int {  // (timing only: waits for the stream)
        if (!timing) return VC_OK;
        VK_CHECK_HIP(hipStreamSynchronize(st));
        const double now = clock_us();
        into += now - since;
        since = now;
        return VC_OK;
    };
    for (size_t lo = 0; lo < n; lo += chunk, nchunks++) {
        const size_t cnt = std::min(chunk, n - lo);
        size_t n_out = 0;
        for (size_t i = 0; i < cnt; i++) n_out += outside[lo + i];
        double c0 = timing ? clock_us() : 0.0;
        VK_CHECK_HIP(hipMemcpyAsync(d_pts.p, a.points + 4 * lo, cnt * sizeof(fe<F>), hipMemcpyHostToDevice, st));
        if (a.row) VK_CHECK_HIP(hipMemcpyAsync(d_row.p, a.row + lo, cnt * 4, hipMemcpyHostToDevice, st));
        VK_TRY(lap(lap_up, c0));
        VK_LAUNCH(ctx, "kzg_many_lane", (k_kzg_many_lane<F>), (cnt + KM_BLOCK - 1) / KM_BLOCK, KM_BLOCK, 0,
                  d_pts.as<uint32_t>(), (uint32_t)N, lgN, (uint32_t)cnt, d_cls.as<uint32_t>(), d_Dv);
        VK_TRY(lap(lap_lane, c0));
        if (n_out) VK_TRY(batch_inverse<F>(ctx, d_Dv, d_Dinv, cnt));
        VK_TRY(lap(lap_inv, c0));
        VK_LAUNCH(ctx, "kzg_many_wave", (k_kzg_many_wave<F>), (cnt + KM_BLOCK / 64 - 1) / (KM_BLOCK / 64), KM_BLOCK, 0,
                  d_f.as<fe<F>>(), (uint32_t)width, a.row ? d_row.as<uint32_t>() : nullptr, (uint32_t)lo,
                  d_pts.as<uint32_t>(), d_cls.as<uint32_t>(), d_Dv, d_Dinv, pw, inv1, n_inv, (uint32_t)N, (uint32_t)cnt,
                  d_q.as<fe<F>>(), d_y.as<fe<F>>());
        VK_TRY(lap(lap_wave, c0));
        bool on_host = false;
        VK_TRY(msm_batch_run(ctx, t, N, d_q.p, cnt, /*mont=*/1, d_xy, d_inf, a.proof_xy + lo * (xyb / 8),
                             a.proof_inf + lo, &on_host));
        VK_TRY(lap(lap_commit, c0));
        if (!on_host) {
            VK_CHECK_HIP(hipMemcpyAsync(a.proof_xy + lo * (xyb / 8), d_xy, cnt * xyb, hipMemcpyDeviceToHost, st));
            VK_CHECK_HIP(hipMemcpyAsync(a.proof_inf + lo, d_inf, cnt, hipMemcpyDeviceToHost, st));
        }
        VK_CHECK_HIP(hipMemcpyAsync(a.y + 4 * lo, d_y.p, cnt * sizeof(fe<F>), hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipStreamSynchronize(st));
        if (timing) lap_back += clock_us() - c0;
    }
    if (timing)
        fprintf(stderr,
                "[kzg_prove_many] n=%zu N=%zu rows=%zu chunks=%zu: upload %.1f us, lane %.1f us, inverse %.1f us, "
                "wave %.1f us, commit %.1f us, read-back %.1f us, call %.1f us (rows' upload and conversion in "
                "the first chunk's upload)\n",
                n, N, a.rows, nchunks, lap_up, lap_lane, lap_inv, lap_wave, lap_commit, lap_back, clock_us() - call0);
    return VC_OK;
}

int prove_many(vc_ctx* ctx, const Args& a) {
    if (!ctx || (ctx->curve != VC_CURVE_BN254 && ctx->curve != VC_CURVE_BLS12_381)) return VC_E_INVALID;
    if (a.N < 2 || (a.N & (a.N - 1)) || a.N > KM_MAX_N || a.width > a.N) return VC_E_INVALID;
    if (a.n && (!a.points || !a.proof_xy || !a.proof_inf || !a.y || (a.width && !a.data))) return VC_E_INVALID;
    if (a.n >= (size_t(1) << 32) || a.rows >= (size_t(1) << 32)) return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(a.table);
    if (!t) return VC_E_TABLE;
    if (t->n < a.N) return VC_E_RANGE;
    if (a.n == 0) return VC_OK;
    if (!a.row && a.rows != a.n) return VC_E_INVALID;
    if (ctx->curve == VC_CURVE_BN254) return prove_many_t<BN254G1, BN254Fr>(ctx, t, a);
    return prove_many_t<BLS381G1, BLS381Fr>(ctx, t, a);
}

}  // namespace
}  // namespace vk

extern "C" int vc_kzg_prove_many(vc_ctx* ctx, int table, size_t N, size_t rows, size_t width, const uint64_t* data,
                                 const uint32_t* row, const uint64_t* points, size_t n, uint64_t* proof_xy,
                                 uint8_t* proof_inf, uint64_t* y) {
    return vk::prove_many(ctx, vk::Args{table, N, rows, width, data, false, row, points, n, proof_xy, proof_inf, y});
}

extern "C" int vc_kzg_prove_many_device(vc_ctx* ctx, int table, size_t N, size_t rows, size_t width,
                                        const void* d_data, const uint32_t* row, const uint64_t* points, size_t n,
                                        uint64_t* proof_xy, uint8_t* proof_inf, uint64_t* y) {
    return vk::prove_many(ctx, vk::Args{table, N, rows, width, d_data, true, row, points, n, proof_xy, proof_inf, y});
}

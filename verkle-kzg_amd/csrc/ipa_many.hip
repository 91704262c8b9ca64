// IPA batch proving (vc_ipa_prove_many): n openings, each IPA::prove_point (ipa/mod.rs:137-154) of
// one of `rows` data rows at its own point over a fresh "ipa" transcript, one proof each -- the
// prover half of the reference's todo!() batch (ipa/mod.rs:156-163). The rows are uploaded and
// converted to Montgomery form once and stay resident; per chunk of at most 8,192 openings, with
// nothing of the proof crossing to the host between the rounds (the commit's own normalisation
// inverts its block products there):
//   init    k_ipa_many_init, a wave per opening: the barycentric weights b, y = <a, b>, the
//           transcript's w;
//   round   k_ipa_many_round, a wave per opening, K = log2 N times: for r > 0 it closes round r - 1
//           (L, R from the previous commit's output into the proof, the challenge x hashed on the
//           device, a, b and the coefficients folded), then writes the round's two rows of N + 1
//           Montgomery scalars in the layout msm_batch_run reads;
//   commit  msm_batch_run over the 2 cnt rows, results left in device memory;
//   finish  k_ipa_many_finish, a wave per opening: closes round K - 1, the tip;
//   one copy back per output array.
// The arithmetic is csrc/ipa_many.hpp, the text tests/cpp/ipa_many_check.cpp runs on the host. Every
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
#include "ipa_many.hpp"
#include "poly.hpp"
#include "scheme_internal.hpp"

namespace vk {

using namespace ipam;

constexpr size_t IM_CHUNK_MAX = 8192;  // 16,384 rows of N + 1: vc_ipa_verify_many's row workspace

// what the three kernels share: the resident rows, the chunk's inputs, its workspace and its proofs
struct IpaManyArgs {
    const FrE* f;          // rows x N, Montgomery
    const uint32_t* row;   // the chunk's row indices, or null: opening o of the chunk has row first + o
    uint32_t first;
    const uint32_t* com;   // the openings' commitments: 16 canonical words each
    const uint8_t* cinf;
    const uint32_t* point; // 8 canonical words each
    const FrE* pw;         // w^i
    FrE n_inv;
    uint32_t N;
    int K;
    FrE* wa;               // N per opening: a's levels 1 .. K (ipam::a_level)
    FrE* wb;               // 2 N per opening: b's levels 0 .. K (ipam::b_level)
    FrE* wc;               // N per opening: the coefficients
    uint32_t* state;       // IM_STATE_WORDS per opening: w, the previous challenge
    FrE* rows;             // 2 (N + 1) per opening: the round's L and R rows
    const uint32_t* cxy;   // the previous commit's output: 2 points per opening, then
    const uint8_t* cflag;  //   their identity flags
    uint32_t *l_xy, *r_xy; // the proofs: K x 16 words per opening
    uint8_t *l_inf, *r_inf;
    uint32_t *tip, *y;     // 8 canonical words per opening
};

__device__ __forceinline__ const FrE* opening_row(const IpaManyArgs& A, uint32_t o) {
    return A.f + (size_t)(A.row ? A.row[o] : A.first + o) * A.N;
}

// Closes round k of opening o: L_k, R_k into the proof, the challenge into the state; returns the
// level that round k + 1 (or the tip) reads. Every lane computes the same challenge.
__device__ __forceinline__ Level close_round(const IpaManyArgs& A, uint32_t o, int k, uint32_t lane) {
    uint32_t lw[16], rw[16], prev[8];
    const uint32_t* src = A.cxy + (size_t)o * 32;
    for (int i = 0; i < 16; i++) lw[i] = src[i], rw[i] = src[16 + i];
    const uint8_t linf = A.cflag[2 * (size_t)o], rinf = A.cflag[2 * (size_t)o + 1];
    uint32_t* st = A.state + (size_t)o * IM_STATE_WORDS;
    for (int i = 0; i < 8; i++) prev[i] = st[8 + i];
    const size_t at = (size_t)o * (size_t)A.K + (size_t)k;
    if (lane < 16) A.l_xy[16 * at + lane] = lw[lane];
    else if (lane < 32) A.r_xy[16 * at + lane - 16] = rw[lane - 16];
    else if (lane == 32) A.l_inf[at] = linf;
    else if (lane == 33) A.r_inf[at] = rinf;
    const FrE x = close_challenge(prev, k, lw, linf != 0, rw, rinf != 0);
    if (lane == 0) fr_store(fe_from_mont<BN254Fr>(x), st + 8);
    return level_after(opening_row(A, o), A.wa + (size_t)o * A.N, A.wb + (size_t)o * 2 * A.N, A.N, k, x);
}

__global__ __launch_bounds__(64) void k_ipa_many_init(IpaManyArgs A) {
    const uint32_t o = blockIdx.x, lane = threadIdx.x, N = A.N;
    const FrE* a = opening_row(A, o);
    FrE* b = A.wb + (size_t)o * 2 * N;
    uint32_t zw[8], cw[16];
    for (int i = 0; i < 8; i++) zw[i] = A.point[8 * (size_t)o + i];
    for (int i = 0; i < 16; i++) cw[i] = A.com[16 * (size_t)o + i];
    uint64_t idx = 0;
    const bool in_dom = point_in_domain(zw, N, &idx);  // (uniform over the wave)
    const FrE z = fe_to_mont<BN254Fr>(fr_load(zw));
    FrE oth = fe_one<BN254Fr>();
    if (!in_dom) {
        FrE tot = bary_lane_total(A.pw, N, z, lane);
        for (uint32_t s = 1; s < 64; s <<= 1) {
            const FrE pt = shfl_xor_pod(tot, s);
            kzgm::others_step<BN254Fr>(tot, oth, pt);
        }
    }
    FrE y = init_lane(a, A.pw, N, z, in_dom, idx, oth, A.n_inv, lane, b);
    for (uint32_t s = 1; s < 64; s <<= 1) y = fe_add<BN254Fr>(y, shfl_xor_pod(y, s));
    uint32_t yc[8];
    const FrE w = opening_w(cw, A.cinf[o] != 0, zw, y, yc);
    if (lane == 0) {
        uint32_t* st = A.state + (size_t)o * IM_STATE_WORDS;
        fr_store(w, st);
        fr_store(fe_from_mont<BN254Fr>(w), st + 8);
        for (int i = 0; i < 8; i++) A.y[8 * (size_t)o + i] = yc[i];
    }
}

__global__ __launch_bounds__(64) void k_ipa_many_round(IpaManyArgs A, int r) {
    const uint32_t o = blockIdx.x, lane = threadIdx.x, N = A.N;
    const Level lv =
        r == 0 ? level_first(opening_row(A, o), A.wb + (size_t)o * 2 * N, N) : close_round(A, o, r - 1, lane);
    FrE* sL = A.rows + (size_t)o * 2 * (N + 1);
    FrE* sR = sL + (N + 1);
    rows_lane(lv, A.wc + (size_t)o * N, N, r, lane, sL, sR);
    FrE dl, dr;  // (round 0 stores no level: a's level 0 is the data row, b's is in place)
    FrE* a_out = a_store(A.wa + (size_t)o * N, N, r);
    FrE* b_out = b_store(A.wb + (size_t)o * 2 * N, N, r);
    halves_lane(lv, (N >> r) / 2, lane, a_out, b_out, dl, dr);
    for (uint32_t s = 1; s < 64; s <<= 1) {
        dl = fe_add<BN254Fr>(dl, shfl_xor_pod(dl, s));
        dr = fe_add<BN254Fr>(dr, shfl_xor_pod(dr, s));
    }
    if (lane == 0) {
        const FrE w = fr_load(A.state + (size_t)o * IM_STATE_WORDS);
        sL[N] = q_term(w, dl);
        sR[N] = q_term(w, dr);
    }
}

__global__ __launch_bounds__(64) void k_ipa_many_finish(IpaManyArgs A) {
    const uint32_t o = blockIdx.x, lane = threadIdx.x;
    const Level lv = close_round(A, o, A.K - 1, lane);
    uint32_t tw[8];
    tip_words(lv, tw);
    if (lane < 8) A.tip[8 * (size_t)o + lane] = tw[lane];
}

namespace {

struct Args {
    int table;
    size_t N, rows;
    const void* data;
    bool d_data;
    const uint32_t* row;
    const uint64_t *com_xy, *points;
    const uint8_t* com_inf;
    size_t n;
    uint64_t *l_xy, *r_xy, *tip, *y;
    uint8_t *l_inf, *r_inf;
};

int prove_many_run(vc_ctx* ctx, Table* t, const Args& a) {
    using F = BN254Fr;
    const size_t N = a.N, n = a.n;
    int K = 0;
    while ((size_t(1) << K) < N) K++;
    size_t chunk = IM_CHUNK_MAX;
    // VKZG_IPA_PROVE_CHUNK (read per call): a test forces small chunks
    if (const char* e = getenv("VKZG_IPA_PROVE_CHUNK"))
        if (atol(e) > 0) chunk = std::min<size_t>((size_t)atol(e), IM_CHUNK_MAX);
    chunk = std::min(chunk, n);
    const bool timing = host_timing();
    const double call0 = timing ? clock_us() : 0.0;
    hipStream_t st = ctx->stream;

    // the rows, resident for the call
    DevBuf d_f(ctx);
    {
        const size_t cells = a.rows * N;
        VK_TRY(d_f.ensure(cells * sizeof(FrE)));
        DevBuf raw(ctx);
        const void* src = a.data;
        if (!a.d_data) {
            VK_TRY(raw.ensure(cells * sizeof(FrE)));
            VK_CHECK_HIP(hipMemcpyAsync(raw.p, a.data, cells * sizeof(FrE), hipMemcpyHostToDevice, st));
            src = raw.p;
        }
        VK_TRY(canon_to_mont_dev<F>(ctx, src, cells, cells, d_f.as<FrE>()));
    }
    DevBuf d_pw(ctx), d_in(ctx), d_flag(ctx), d_row(ctx), d_wa(ctx), d_wb(ctx), d_wc(ctx), d_state(ctx), d_rows(ctx),
        d_commit(ctx), d_pts(ctx), d_pinf(ctx), d_fr(ctx);
    VK_TRY(d_pw.ensure(N * 32));
    VK_TRY(d_in.ensure(chunk * (64 + 32)));  // the commitments | the points
    VK_TRY(d_flag.ensure(chunk));
    VK_TRY(d_row.ensure(chunk * 4));
    VK_TRY(d_wa.ensure(chunk * N * 32));
    VK_TRY(d_wb.ensure(chunk * 2 * N * 32));
    VK_TRY(d_wc.ensure(chunk * N * 32));
    VK_TRY(d_state.ensure(chunk * IM_STATE_WORDS * 4));
    VK_TRY(d_rows.ensure(chunk * 2 * (N + 1) * 32));
    VK_TRY(d_commit.ensure(chunk * 2 * 65));          // a round's L, R and their identity flags
    VK_TRY(d_pts.ensure(chunk * 2 * (size_t)K * 64));  // the proofs' L | R
    VK_TRY(d_pinf.ensure(chunk * 2 * (size_t)K));
    VK_TRY(d_fr.ensure(chunk * 2 * 32));               // tip | y
    {
        std::vector<Fr> pw(N);
        const Fr omega = bn254_group_gen(N);
        Fr w = fe_one<F>();
        for (size_t i = 0; i < N; i++) pw[i] = w, w = fe_mul<F>(w, omega);
        VK_CHECK_HIP(hipMemcpyAsync(d_pw.p, pw.data(), N * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipStreamSynchronize(st));  // (pw dies here)
    }
    const double lap_rows = timing ? clock_us() - call0 : 0.0;  // the rows' upload and conversion, the workspace
    IpaManyArgs A;
    A.f = d_f.as<FrE>();
    uint32_t* d_com = d_in.as<uint32_t>();
    uint32_t* d_point = d_com + chunk * 16;
    A.com = d_com, A.point = d_point, A.cinf = d_flag.as<uint8_t>();
    A.pw = d_pw.as<FrE>();
    A.n_inv = fe_inv_bin<F>(mont_from_u64<F>(N));
    A.N = (uint32_t)N, A.K = K;
    A.wa = d_wa.as<FrE>(), A.wb = d_wb.as<FrE>(), A.wc = d_wc.as<FrE>();
    A.state = d_state.as<uint32_t>();
    A.rows = d_rows.as<FrE>();
    uint8_t* d_cxy = d_commit.as<uint8_t>();
    uint8_t* d_cflag = d_cxy + chunk * 2 * 64;
    A.cxy = reinterpret_cast<const uint32_t*>(d_cxy), A.cflag = d_cflag;
    A.l_xy = d_pts.as<uint32_t>(), A.r_xy = A.l_xy + chunk * (size_t)K * 16;
    A.l_inf = d_pinf.as<uint8_t>(), A.r_inf = A.l_inf + chunk * (size_t)K;
    A.tip = d_fr.as<uint32_t>(), A.y = A.tip + chunk * 8;

    double lap_up = 0, lap_init = 0, lap_field = 0, lap_commit = 0, lap_back = 0;
    size_t nchunks = 0;
    auto lap = [&](double& into, double& since) -> int {  // (timing only: waits for the stream)
        if (!timing) return VC_OK;
        VK_CHECK_HIP(hipStreamSynchronize(st));
        const double now = clock_us();
        into += now - since;
        since = now;
        return VC_OK;
    };
    std::vector<uint64_t> cxy;  // the chunk's commitments, gathered by row
    std::vector<uint8_t> cinf;
    for (size_t lo = 0; lo < n; lo += chunk, nchunks++) {
        const size_t cnt = std::min(chunk, n - lo);
        double c0 = timing ? clock_us() : 0.0;
        cxy.resize(cnt * 8), cinf.resize(cnt);
        for (size_t i = 0; i < cnt; i++) {
            const size_t r = a.row ? a.row[lo + i] : lo + i;
            memcpy(&cxy[8 * i], a.com_xy + 8 * r, 64);
            cinf[i] = a.com_inf[r];
        }
        VK_CHECK_HIP(hipMemcpyAsync(d_com, cxy.data(), cnt * 64, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_flag.p, cinf.data(), cnt, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_point, a.points + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
        if (a.row) VK_CHECK_HIP(hipMemcpyAsync(d_row.p, a.row + lo, cnt * 4, hipMemcpyHostToDevice, st));
        A.row = a.row ? d_row.as<uint32_t>() : nullptr;
        A.first = (uint32_t)lo;
        VK_TRY(lap(lap_up, c0));
        VK_LAUNCH(ctx, "ipa_many_init", k_ipa_many_init, cnt, 64, 0, A);
        VK_TRY(lap(lap_init, c0));
        for (int r = 0; r < K; r++) {
            VK_LAUNCH(ctx, "ipa_many_round", k_ipa_many_round, cnt, 64, 0, A, r);
            VK_TRY(lap(lap_field, c0));
            VK_TRY(msm_batch_run(ctx, t, N + 1, d_rows.p, 2 * cnt, /*mont=*/1, d_cxy, d_cflag));
            VK_TRY(lap(lap_commit, c0));
        }
        VK_LAUNCH(ctx, "ipa_many_finish", k_ipa_many_finish, cnt, 64, 0, A);
        VK_TRY(lap(lap_field, c0));
        const size_t Ks = (size_t)K;
        VK_CHECK_HIP(hipMemcpyAsync(a.l_xy + 8 * lo * Ks, A.l_xy, cnt * Ks * 64, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipMemcpyAsync(a.r_xy + 8 * lo * Ks, A.r_xy, cnt * Ks * 64, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipMemcpyAsync(a.l_inf + lo * Ks, A.l_inf, cnt * Ks, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipMemcpyAsync(a.r_inf + lo * Ks, A.r_inf, cnt * Ks, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipMemcpyAsync(a.tip + 4 * lo, A.tip, cnt * 32, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipMemcpyAsync(a.y + 4 * lo, A.y, cnt * 32, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipStreamSynchronize(st));  // (cxy / cinf are refilled by the next chunk)
        if (timing) lap_back += clock_us() - c0;
    }
    if (timing)
        fprintf(stderr,
                "[ipa_prove_many] n=%zu N=%zu rows=%zu chunks=%zu: rows %.1f us, upload %.1f us, init %.1f us, rounds' "
                "field kernels %.1f us, commits %.1f us, copy-back %.1f us, call %.1f us\n",
                n, N, a.rows, nchunks, lap_rows, lap_up, lap_init, lap_field, lap_commit, lap_back, clock_us() - call0);
    return VC_OK;
}

// every status but VC_OK, on the host, before any GPU work
int prove_many(vc_ctx* ctx, const Args& a) {
    using F = BN254Fr;
    if (!ctx || ctx->curve != VC_CURVE_BN254) return VC_E_INVALID;
    if (a.N < 2 || (a.N & (a.N - 1)) || a.N > IM_N_MAX) return VC_E_INVALID;
    if (a.n && (!a.data || !a.com_xy || !a.com_inf || !a.points || !a.l_xy || !a.l_inf || !a.r_xy || !a.r_inf ||
                !a.tip || !a.y))
        return VC_E_INVALID;
    if (a.n >= (size_t(1) << 32) || a.rows >= (size_t(1) << 32)) return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(a.table);
    if (!t) return VC_E_TABLE;
    if (t->n < a.N + 1) return VC_E_INVALID;
    if (a.n == 0) return VC_OK;
    if (!a.row && a.rows != a.n) return VC_E_INVALID;
    if (a.row)
        for (size_t i = 0; i < a.n; i++)
            if (a.row[i] >= a.rows) return VC_E_INVALID;
    const uint32_t* pts32 = reinterpret_cast<const uint32_t*>(a.points);
    std::atomic<int> bad{0};  // 1: a point >= r; 2: a domain element that is not below N
    pool_for(0, a.n, 1024, [&](size_t i) {
        const uint32_t* zw = pts32 + 8 * i;
        if (!ate::words_below_modulus<F>(zw)) {
            bad |= 1;
            return;
        }
        if (barycentric_panics(a.N, canon_to_mont<F>(a.points + 4 * i))) bad |= 2;
    });
    if (bad & 1) return VC_E_INVALID;
    if (bad & 2) return VC_E_DOMAIN;
    return prove_many_run(ctx, t, a);
}

}  // namespace
}  // namespace vk

extern "C" int vc_ipa_prove_many(vc_ctx* ctx, int table, size_t N, size_t rows, const uint64_t* data,
                                 const uint32_t* row, const uint64_t* com_xy, const uint8_t* com_inf,
                                 const uint64_t* points, size_t n, uint64_t* l_xy, uint8_t* l_inf, uint64_t* r_xy,
                                 uint8_t* r_inf, uint64_t* tip, uint64_t* y) {
    return vk::prove_many(
        ctx, vk::Args{table, N, rows, data, false, row, com_xy, points, com_inf, n, l_xy, r_xy, tip, y, l_inf, r_inf});
}

extern "C" int vc_ipa_prove_many_device(vc_ctx* ctx, int table, size_t N, size_t rows, const void* d_data,
                                        const uint32_t* row, const uint64_t* com_xy, const uint8_t* com_inf,
                                        const uint64_t* points, size_t n, uint64_t* l_xy, uint8_t* l_inf,
                                        uint64_t* r_xy, uint8_t* r_inf, uint64_t* tip, uint64_t* y) {
    return vk::prove_many(
        ctx, vk::Args{table, N, rows, d_data, true, row, com_xy, points, com_inf, n, l_xy, r_xy, tip, y, l_inf, r_inf});
}

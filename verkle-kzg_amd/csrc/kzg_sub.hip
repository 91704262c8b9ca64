// KZG subvector proving (vc_kzg_prove_subvector_many): n subsets, each one constant-size proof that
// the k_s positions idx[idx_off[s] .. idx_off[s + 1]) of row row[s] hold their values -- the
// reference's prove_batch (kzg/mod.rs:156-163, todo!() there). The rows are uploaded and converted
// to Montgomery form once and stay resident; per chunk of at most 16,384 subsets:
//   wave    k_kzg_sub_wave, a wave per subset, four to a block: the weights cw_i = c_i w^-i into a
//           scratch row in device memory, the y in the caller's order, then the quotient row
//           (Montgomery, the layout msm_batch_run reads) and its k diagonal terms;
//   commit  msm_batch_run over the quotient rows (commit.hip), as vc_kzg_prove_many.
// The arithmetic is csrc/kzg_sub.hpp, the text tests/cpp/kzg_sub_check.cpp runs on the host. Every
// status other than VC_OK is decided on the host before the first upload. The workspace beside the
// resident rows is sized by the chunk, not by n.
// vc_kzg_g1_powers: the powers [s^t]_1, t < K, from the Lagrange SRS alone, as K batched commits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ctx.hpp"
#include "ec29.hpp"
#include "host/fr.hpp"
#include "kzg_sub.hpp"
#include "poly.hpp"
#include "scheme_internal.hpp"

namespace vk {

using namespace kzgs;

constexpr uint32_t KS_BLOCK = 256;  // four waves, four subsets
constexpr size_t KS_CHUNK_MAX = 16384;

// Wave w of the grid takes subset w < n: the indices S = idx[off[w] .. off[w + 1]) (distinct, below N:
// the host has checked) of row row[w] (row == nullptr: row `first + w`) of f (rows of `width`
// Montgomery values). pw, inv1: the domain's cached tables. cw: a scratch value per index, y: a
// canonical value per index (both laid out as idx); q: n rows of N Montgomery values. The loops'
// bounds are per wave.
template <class F>
__global__ __launch_bounds__(KS_BLOCK, 4) void k_kzg_sub_wave(const fe<F>* __restrict__ f, uint32_t width,
                                                           const uint32_t* __restrict__ row, uint32_t first,
                                                           const uint32_t* __restrict__ idx,
                                                           const uint32_t* __restrict__ off,
                                                           const fe<F>* __restrict__ pw,
                                                           const fe<F>* __restrict__ inv1, uint32_t N, uint32_t n,
                                                           fe<F>* cw, fe<F>* q, fe<F>* __restrict__ y) {
    // (the wave's index through readfirstlane, as k_kzg_many_wave: the subset, its row and every loop
    // bound below are then known to be uniform)
    const uint32_t o = blockIdx.x * (KS_BLOCK / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    if (o >= n) return;
    const fe<F>* fr = f + (size_t)(row ? row[o] : first + o) * width;
    const uint32_t b = off[o], k = off[o + 1] - b;
    const uint32_t* S = idx + b;
    fe<F>* cwr = cw + b;
    fe<F>* qr = q + (size_t)o * N;
    // ---- the weights, lanes over the subset
    uint32_t sum = 0;
    for (uint32_t t = lane; t < k; t += 64) sum += S[t];
    for (uint32_t s = 1; s < 64; s <<= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)s);
    const fe<F> wsum = sub_wsum<F>(pw, N, sum);
    for (uint32_t t = lane; t < k; t += 64) {
        cwr[t] = sub_weight<F>(S, k, inv1, N, t, wsum);
        y[b + t] = fe_from_mont<F>(row_at<F>(fr, width, S[t]));
    }
    // The passes below read weights other lanes of this wave stored. The release waits for the wave's
    // stores (they are in the CU's vector cache, which its loads go through), and the pair keeps
    // the compiler from moving a load of cw above them; producers and consumers are lanes of one wave
    // in one instruction stream, so no flag is needed.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // ---- the row, lanes over its entries
    for (uint32_t j = lane; j < N; j += 64) qr[j] = sub_row_entry<F>(fr, width, S, k, cwr, inv1, N, j);
    // ---- the diagonal terms: entry m is its lane's own from the pass above
#pragma unroll 1
    for (uint32_t t = 0; t < k; t++) {
        const uint32_t m = S[t];
        fe<F> acc = sub_diag_pass<F>(fr, width, inv1, N, m, row_at<F>(fr, width, m), lane);
        for (uint32_t s = 1; s < 64; s <<= 1) acc = fe_add<F>(acc, shfl_xor_pod(acc, s));
        if (lane == (m & 63u)) qr[m] = sub_diag<F>(qr[m], cwr[t], acc);
    }
}

namespace {

struct Args {
    int table;
    size_t N, rows, width;
    const void* data;
    bool d_data;
    const uint32_t* row;
    const uint32_t* idx_off;
    const uint32_t* idx;
    size_t n;
    uint64_t* proof_xy;
    uint8_t* proof_inf;
    uint64_t* y;
};

template <class C_, class F>
int prove_sub_t(vc_ctx* ctx, Table* t, const Args& a) {
    const size_t N = a.N, n = a.n, width = a.width;
    // ---- every status but VC_OK, before any GPU work
    if (a.row)
        for (size_t i = 0; i < n; i++)
            if (a.row[i] >= a.rows) return VC_E_INVALID;
    {
        std::vector<uint32_t> seen(N, UINT32_MAX);  // the last subset that held the index
        for (size_t s = 0; s < n; s++) {
            if (a.idx_off[s + 1] <= a.idx_off[s]) return VC_E_INVALID;  // empty, or not monotone
            if (a.idx_off[s + 1] - a.idx_off[s] > N) return VC_E_INVALID;
            for (uint32_t p = a.idx_off[s]; p < a.idx_off[s + 1]; p++) {
                const uint32_t i = a.idx[p];
                if (i >= N || seen[i] == (uint32_t)s) return VC_E_INVALID;
                seen[i] = (uint32_t)s;
            }
        }
    }
    size_t chunk = KS_CHUNK_MAX;
    // VKZG_KZG_PROVE_CHUNK (read per call): a test forces small chunks
    if (const char* e = getenv("VKZG_KZG_PROVE_CHUNK"))
        if (atol(e) > 0) chunk = std::min<size_t>((size_t)atol(e), KS_CHUNK_MAX);
    chunk = std::min(chunk, n);
    size_t max_idx = 0;  // the most indices a chunk holds: its scratch row and its y
    for (size_t lo = 0; lo < n; lo += chunk)
        max_idx = std::max<size_t>(max_idx, a.idx_off[std::min(lo + chunk, n)] - a.idx_off[lo]);
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

    DevBuf d_q(ctx), d_idx(ctx), d_off(ctx), d_row(ctx), d_cw(ctx), d_y(ctx), d_out(ctx);
    VK_TRY(d_q.ensure(chunk * N * sizeof(fe<F>)));
    VK_TRY(d_idx.ensure(max_idx * 4));
    VK_TRY(d_off.ensure((chunk + 1) * 4));
    VK_TRY(d_row.ensure(chunk * 4));
    VK_TRY(d_cw.ensure(max_idx * sizeof(fe<F>)));
    VK_TRY(d_y.ensure(max_idx * sizeof(fe<F>)));
    VK_TRY(d_out.ensure(chunk * (xyb + 1)));  // the proofs, then their identity flags
    uint8_t* d_xy = d_out.as<uint8_t>();
    uint8_t* d_inf = d_xy + chunk * xyb;
    std::vector<uint32_t> rel(chunk + 1);  // the chunk's offsets from its first index

    double lap_up = 0, lap_wave = 0, lap_commit = 0, lap_back = 0;
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
        const size_t base = a.idx_off[lo], nidx = a.idx_off[lo + cnt] - base;
        for (size_t i = 0; i <= cnt; i++) rel[i] = a.idx_off[lo + i] - (uint32_t)base;
        double c0 = timing ? clock_us() : 0.0;
        VK_CHECK_HIP(hipMemcpyAsync(d_idx.p, a.idx + base, nidx * 4, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_off.p, rel.data(), (cnt + 1) * 4, hipMemcpyHostToDevice, st));
        if (a.row) VK_CHECK_HIP(hipMemcpyAsync(d_row.p, a.row + lo, cnt * 4, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipStreamSynchronize(st));  // rel is rewritten for the next chunk
        VK_TRY(lap(lap_up, c0));
        VK_LAUNCH(ctx, "kzg_sub_wave", (k_kzg_sub_wave<F>), (cnt + KS_BLOCK / 64 - 1) / (KS_BLOCK / 64), KS_BLOCK, 0,
                  d_f.as<fe<F>>(), (uint32_t)width, a.row ? d_row.as<uint32_t>() : nullptr, (uint32_t)lo,
                  d_idx.as<uint32_t>(), d_off.as<uint32_t>(), pw, inv1, (uint32_t)N, (uint32_t)cnt, d_cw.as<fe<F>>(),
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
        VK_CHECK_HIP(hipMemcpyAsync(a.y + 4 * base, d_y.p, nidx * sizeof(fe<F>), hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipStreamSynchronize(st));
        if (timing) lap_back += clock_us() - c0;
    }
    if (timing)
        fprintf(stderr,
                "[kzg_prove_subvector_many] n=%zu N=%zu rows=%zu indices=%u chunks=%zu: upload %.1f us, wave %.1f us, "
                "commit %.1f us, read-back %.1f us, call %.1f us (rows' upload and conversion in the first chunk's "
                "upload)\n",
                n, N, a.rows, a.idx_off[n] - a.idx_off[0], nchunks, lap_up, lap_wave, lap_commit, lap_back,
                clock_us() - call0);
    return VC_OK;
}

int prove_sub(vc_ctx* ctx, const Args& a) {
    if (!ctx || (ctx->curve != VC_CURVE_BN254 && ctx->curve != VC_CURVE_BLS12_381)) return VC_E_INVALID;
    if (a.N < 2 || (a.N & (a.N - 1)) || a.N > kzgm::KM_MAX_N || a.width > a.N) return VC_E_INVALID;
    if (a.n && (!a.idx_off || !a.idx || !a.proof_xy || !a.proof_inf || !a.y || (a.width && !a.data)))
        return VC_E_INVALID;
    if (a.n >= (size_t(1) << 32) || a.rows >= (size_t(1) << 32)) return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(a.table);
    if (!t) return VC_E_TABLE;
    if (t->n < a.N) return VC_E_RANGE;
    if (a.n == 0) return VC_OK;
    if (!a.row && a.rows != a.n) return VC_E_INVALID;
    if (ctx->curve == VC_CURVE_BN254) return prove_sub_t<BN254G1, BN254Fr>(ctx, t, a);
    return prove_sub_t<BLS381G1, BLS381Fr>(ctx, t, a);
}

// row t of the commits' scalars is (w^(j t))_j: X^t on the domain, whose commit over the Lagrange
// SRS is [s^t]_1
template <class C_, class F>
int g1_powers_t(vc_ctx* ctx, Table* t, size_t N, size_t K, uint64_t* out) {
    const fe<F> omega = group_gen_t<F>(N, fr_generator<F>());
    std::vector<fe<F>> pw(N), rows(K * N);
    pw[0] = fe_one<F>();
    for (size_t j = 1; j < N; j++) pw[j] = fe_mul<F>(pw[j - 1], omega);
    for (size_t p = 0; p < K; p++)
        for (size_t j = 0; j < N; j++) rows[p * N + j] = pw[(j * p) & (N - 1)];
    const size_t xyb = (size_t)C_::F::N * 8;
    hipStream_t st = ctx->stream;
    DevBuf d_rows(ctx), d_out(ctx);
    VK_TRY(d_rows.ensure(K * N * sizeof(fe<F>)));
    VK_TRY(d_out.ensure(K * (xyb + 1)));
    uint8_t* d_xy = d_out.as<uint8_t>();
    uint8_t* d_inf = d_xy + K * xyb;
    VK_CHECK_HIP(hipMemcpyAsync(d_rows.p, rows.data(), K * N * sizeof(fe<F>), hipMemcpyHostToDevice, st));
    std::vector<uint64_t> xy(K * (xyb / 8));
    std::vector<uint8_t> inf(K);
    bool on_host = false;
    VK_TRY(msm_batch_run(ctx, t, N, d_rows.p, K, /*mont=*/1, d_xy, d_inf, xy.data(), inf.data(), &on_host));
    if (!on_host) {
        VK_CHECK_HIP(hipMemcpyAsync(xy.data(), d_xy, K * xyb, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipMemcpyAsync(inf.data(), d_inf, K, hipMemcpyDeviceToHost, st));
    }
    VK_CHECK_HIP(hipStreamSynchronize(st));
    for (size_t p = 0; p < K; p++)
        if (inf[p]) return VC_E_INVALID;  // s = 0: not a setup
    std::copy(xy.begin(), xy.end(), out);
    return VC_OK;
}

}  // namespace
}  // namespace vk

extern "C" int vc_kzg_prove_subvector_many(vc_ctx* ctx, int table, size_t N, size_t rows, size_t width,
                                           const uint64_t* data, const uint32_t* row, const uint32_t* idx_off,
                                           const uint32_t* idx, size_t n, uint64_t* proof_xy, uint8_t* proof_inf,
                                           uint64_t* y) {
    return vk::prove_sub(ctx,
                         vk::Args{table, N, rows, width, data, false, row, idx_off, idx, n, proof_xy, proof_inf, y});
}

extern "C" int vc_kzg_prove_subvector_many_device(vc_ctx* ctx, int table, size_t N, size_t rows, size_t width,
                                                  const void* d_data, const uint32_t* row, const uint32_t* idx_off,
                                                  const uint32_t* idx, size_t n, uint64_t* proof_xy,
                                                  uint8_t* proof_inf, uint64_t* y) {
    return vk::prove_sub(ctx,
                         vk::Args{table, N, rows, width, d_data, true, row, idx_off, idx, n, proof_xy, proof_inf, y});
}

extern "C" int vc_kzg_g1_powers(vc_ctx* ctx, int table, size_t N, size_t K, uint64_t* out) {
    if (!ctx || (ctx->curve != VC_CURVE_BN254 && ctx->curve != VC_CURVE_BLS12_381)) return VC_E_INVALID;
    if (N < 2 || (N & (N - 1)) || N > vk::kzgm::KM_MAX_N || K == 0 || !out) return VC_E_INVALID;
    vk::Guard g(ctx);
    vk::Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    if (t->n < N || K > N) return VC_E_RANGE;
    if (ctx->curve == VC_CURVE_BN254) return vk::g1_powers_t<vk::BN254G1, vk::BN254Fr>(ctx, t, N, K, out);
    return vk::g1_powers_t<vk::BLS381G1, vk::BLS381Fr>(ctx, t, N, K, out);
}

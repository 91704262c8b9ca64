// Batched IPA verification on the GPU (vc_ipa_verify_many): n independent openings over one CRS,
// one verdict each. Per chunk of proofs:
//   host    the Fiat-Shamir transcripts (w and the K round challenges per proof) on the host pool,
//           one chunk ahead of the device;
//   field   k_ipa_verify_field, a wave per proof: the N + 1 Montgomery scalars of the fixed row
//           over (g, q) and the 1 + 2K scalars over (C, L_k, R_k), in device memory;
//   fixed   msm_batch_run over the rows (commit.hip, its own latency / throughput choice), affine
//           results in device memory;
//   curve   k_ipa_verify_curve, IPA_LP lanes per proof: validates C, L_k, R_k, sums the variable
//           part, adds the fixed part, writes the verdict byte.
// The arithmetic is csrc/ipa_verify.hpp, the text tests/cpp/ipa_verify_check.cpp runs on the host.
// The workspace is sized by the chunk, not by n; the verdicts come back in one copy.
//
// Curve kernel's shape: a proof's 1 + 2K terms share one chain of 254 doublings, so fewer lanes
// per proof mean less work (a lane per term would double 254 times for each), more lanes mean
// shorter serial chains and more waves for a small batch. IPA_LP = 8: at K = 8 a lane takes 2 or 3
// of the 17 terms (254 doublings + ~300 mixed adds in series), the 8 partial sums fold in 3 xor
// shuffles, and a chunk of 16384 proofs fills the 1024 SIMDs with two waves each (the kernel is a
// chain of dependent multiplies: a second wave per SIMD fills the first one's issue gaps). A lane keeps the
// accumulator and one point in registers; its points (converted to Montgomery form in place by the
// validation pass) and scalar bits are re-read from global memory, 64 B per ~2000 instructions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <memory>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "ec29.hpp"
#include "ipa_verify.hpp"
#include "scheme_internal.hpp"
#include "host/pool.hpp"

namespace vk {

using namespace ipav;

constexpr int IPA_LP = 8;  // lanes per proof of the curve kernel (a power of two <= 64)

// one wave per proof. chal: [w, x_0 .. x_{K-1}] Montgomery per proof; tip, y, point canonical;
// pw: the domain's w^i (Montgomery, N of them); rows: N + 1 Montgomery scalars per proof; vs:
// 1 + 2K canonical scalars per proof; bad: 1 for tip, y or point >= r (row zeroed, vs unwritten)
__global__ __launch_bounds__(64) void k_ipa_verify_field(const uint32_t* __restrict__ chal,
                                                         const uint32_t* __restrict__ tip_w,
                                                         const uint32_t* __restrict__ y_w,
                                                         const uint32_t* __restrict__ point_w,
                                                         const FrE* __restrict__ pw, FrE n_inv, uint32_t N, int K,
                                                         uint32_t* rows, uint32_t* __restrict__ vs,
                                                         uint8_t* __restrict__ bad) {
    __shared__ FrE xs[32];
    const size_t p = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t* ch = chal + p * (size_t)(K + 1) * 8;
    if ((int)lane < K) xs[lane] = fr_load(ch + 8 * (1 + lane));
    __syncthreads();
    uint32_t tw[8], yw[8], zw[8];
    for (int k = 0; k < 8; k++) {
        tw[k] = tip_w[8 * p + k];
        yw[k] = y_w[8 * p + k];
        zw[k] = point_w[8 * p + k];
    }
    uint32_t* row = rows + p * ((size_t)N + 1) * 8;
    if (!(ate::words_below_modulus<BN254Fr>(tw) && ate::words_below_modulus<BN254Fr>(yw) &&
          ate::words_below_modulus<BN254Fr>(zw))) {  // (uniform over the block)
        for (size_t i = lane; i <= N; i += 64) fr_store(fe_zero<BN254Fr>(), row + 8 * i);
        if (lane == 0) bad[p] = 1;
        return;
    }
    const FrE tip = fe_to_mont<BN254Fr>(fr_load(tw)), z = fe_to_mont<BN254Fr>(fr_load(zw));
    uint64_t idx = 0;
    const bool in_dom = point_in_domain(zw, N, &idx);
    Frac f = frac_zero();
    for (uint32_t i = lane; i < N; i += 64) {
        const FrE s = s_coeff(xs, K, i);
        fr_store(row_entry(tip, s), row + 8 * (size_t)i);
        if (!in_dom) f = frac_add_term(f, s, pw[i], z);
    }
    // outside the domain every scalar of the proof is multiplied by the sum's denominator instead
    // of the sum being divided by it (ipa_verify.hpp): a second pass over the lane's own entries
    FrE scale = fe_one<BN254Fr>();
    if (!in_dom) {
        for (uint32_t m = 1; m < 64; m <<= 1) f = frac_add(f, shfl_xor_pod(f, m));
        scale = f.den;
        for (uint32_t i = lane; i < N; i += 64)
            fr_store(fr_mul(fr_load(row + 8 * (size_t)i), scale), row + 8 * (size_t)i);
    }
    if (lane == 0) {
        const FrE cb = in_dom ? s_coeff(xs, K, (uint32_t)idx) : bary_dot_scaled(f, z, K, n_inv);
        const FrE prodx = var_scalars(xs, K, scale, vs + p * (size_t)(1 + 2 * K) * 8);
        fr_store(row_tail(prodx, fr_load(ch), fe_to_mont<BN254Fr>(fr_load(yw)), tip, cb, scale), row + 8 * (size_t)N);
        // (a zero scale would make every scalar zero and the sum the identity: the host has rejected
        // the domain elements that give one, so this is never taken)
        bad[p] = fe_is_zero<BN254Fr>(scale) ? 1 : 0;
    }
}

// IPA_LP lanes per proof; lane `sub` takes terms sub, sub + IPA_LP, .. of (C, L_0, R_0, ..). The
// point arrays are canonical on entry and hold the Montgomery form of every validated point on
// exit (each lane rewrites, and later re-reads, only its own terms). fixed_xy / fixed_inf: the
// fixed rows' commitments, canonical affine.
__global__ __launch_bounds__(64) void k_ipa_verify_curve(uint32_t* com_xy, const uint8_t* __restrict__ com_inf,
                                                         uint32_t* l_xy, const uint8_t* __restrict__ l_inf,
                                                         uint32_t* r_xy, const uint8_t* __restrict__ r_inf,
                                                         const uint32_t* __restrict__ vs,
                                                         const uint32_t* __restrict__ fixed_xy,
                                                         const uint8_t* __restrict__ fixed_inf,
                                                         const uint8_t* __restrict__ bad, int K, size_t n,
                                                         uint8_t* __restrict__ out) {
    const size_t gid = (size_t)blockIdx.x * 64 + threadIdx.x;
    const size_t p = gid / IPA_LP;
    const int sub = (int)(gid % IPA_LP);
    const int T = 1 + 2 * K;
    const bool active = p < n;
    const int count = active && sub < T ? (T - sub + IPA_LP - 1) / IPA_LP : 0;
    auto term_xy = [&](int t) -> uint32_t* {
        if (t == 0) return com_xy + 16 * p;
        const size_t at = 16 * (p * (size_t)K + (size_t)((t - 1) >> 1));
        return ((t - 1) & 1) ? r_xy + at : l_xy + at;
    };
    auto term_inf = [&](int t) -> bool {
        if (t == 0) return com_inf[p] != 0;
        const size_t at = p * (size_t)K + (size_t)((t - 1) >> 1);
        return (((t - 1) & 1) ? r_inf[at] : l_inf[at]) != 0;
    };
    int ok = active && !bad[p];
    if (ok)
        for (int j = 0; j < count; j++) {
            const int t = sub + j * IPA_LP;
            if (term_inf(t)) continue;
            uint32_t* q = term_xy(t);
            uint32_t w[16];
            for (int k = 0; k < 16; k++) w[k] = q[k];
            G1P P;
            if (!ate::g1_load(w, P)) {
                ok = 0;
                break;
            }
            for (int k = 0; k < 8; k++) {
                q[k] = P.x.v[k];
                q[8 + k] = P.y.v[k];
            }
        }
    for (uint32_t m = 1; m < (uint32_t)IPA_LP; m <<= 1) ok &= __shfl_xor(ok, m, 64);
    G1A A = BN254G1::zero();
    if (ok) {
        const uint32_t* sc = vs + p * (size_t)T * 8;
        A = var_partial_sum(
            count,
            [&](int j, G1P& P) {
                const int t = sub + j * IPA_LP;
                if (term_inf(t)) return false;
                const uint32_t* q = term_xy(t);
                for (int k = 0; k < 8; k++) {
                    P.x.v[k] = q[k];
                    P.y.v[k] = q[8 + k];
                }
                return true;
            },
            [&](int j, int b) { return ((sc[8 * (sub + j * IPA_LP) + (b >> 5)] >> (b & 31)) & 1u) != 0; });
    }
    for (uint32_t m = 1; m < (uint32_t)IPA_LP; m <<= 1) A = BN254G1::add(A, shfl_xor_pod(A, m));
    if (active && sub == 0) out[p] = ok && sum_is_identity(A, fixed_xy + 16 * p, fixed_inf[p] != 0) ? 1 : 0;
}

namespace {
bool canonical_fr(const uint64_t* w) { return ate::words_below_modulus<BN254Fr>(reinterpret_cast<const uint32_t*>(w)); }
}  // namespace

// (shared with vc_ipa_verify_batch's prior-transcript path, ipa_batch.hip)
void ipa_host_challenges(size_t lo, size_t cnt, int K, const uint64_t* com_xy, const uint8_t* com_inf,
                         const uint64_t* points, const uint64_t* y, const uint64_t* l_xy, const uint8_t* l_inf,
                         const uint64_t* r_xy, const uint8_t* r_inf, vc_transcript** transcripts, Fr* chal) {
    using F = BN254Fr;
    pool_for(0, cnt, 16, [&](size_t j) {
        const size_t p = lo + j;
        const bool own = !(transcripts && transcripts[p]);
        vc_transcript* tr = own ? vc_transcript_new("ipa") : transcripts[p];
        transcript_append_point(tr, com_xy + 8 * p, com_inf[p] != 0, "C");
        transcript_append_fr(tr, canon_to_mont<F>(points + 4 * p), "input point");
        transcript_append_fr(tr, canon_to_mont<F>(y + 4 * p), "output point");
        Fr* c = &chal[j * (size_t)(K + 1)];
        c[0] = transcript_digest(tr, "w");
        for (int k = 0; k < K; k++) {
            const size_t at = p * (size_t)K + (size_t)k;
            transcript_append_point(tr, l_xy + 8 * at, l_inf[at] != 0, "L");
            transcript_append_point(tr, r_xy + 8 * at, r_inf[at] != 0, "R");
            c[1 + k] = transcript_digest(tr, "x");
        }
        if (own) vc_transcript_free(tr);
    });
}

// ---- the device half of a chunk, for callers whose inputs are already in device memory
// (vc_ipa_verify_many below; the multiproof many-verifier, mp_verify.hip, whose challenges are hashed
// on the device from its own transcript state)
struct IpaVerifyWork {
    DevBuf rows, vs, fixed, pw, bad;
    size_t N = 0, chunk = 0;
    int K = 0;
    Fr n_inv;
    explicit IpaVerifyWork(vc_ctx* ctx) : rows(ctx), vs(ctx), fixed(ctx), pw(ctx), bad(ctx) {}
};
int ipa_verify_work_new(vc_ctx* ctx, size_t N, size_t chunk, IpaVerifyWork** out) {
    using F = BN254Fr;
    *out = nullptr;
    std::unique_ptr<IpaVerifyWork> w(new (std::nothrow) IpaVerifyWork(ctx));
    if (!w) return VC_E_OOM;
    w->N = N;
    w->chunk = chunk;
    while ((size_t(1) << w->K) < N) w->K++;
    const size_t T = 1 + 2 * (size_t)w->K;
    VK_TRY(w->rows.ensure(chunk * (N + 1) * 32));
    VK_TRY(w->vs.ensure(chunk * T * 32));
    VK_TRY(w->fixed.ensure(chunk * 65));  // the fixed rows' commitments and their flags
    VK_TRY(w->bad.ensure(chunk));
    VK_TRY(w->pw.ensure(N * 32));
    {  // the domain's powers, once
        std::vector<Fr> pw(N);
        const Fr omega = bn254_group_gen(N);
        Fr x = fe_one<F>();
        for (size_t i = 0; i < N; i++) {
            pw[i] = x;
            x = fe_mul<F>(x, omega);
        }
        VK_CHECK_HIP(hipMemcpyAsync(w->pw.p, pw.data(), N * 32, hipMemcpyHostToDevice, ctx->stream));
        VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    }
    w->n_inv = fe_inv_bin<F>(mont_from_u64<F>(N));
    *out = w.release();
    return VC_OK;
}
void ipa_verify_work_free(IpaVerifyWork* w) { delete w; }
// cnt <= chunk proofs: field, fixed commit, curve; verdict bytes at d_out. The point arrays are
// rewritten (k_ipa_verify_curve). laps: null, or three sums (field, fixed commit, curve, us) that
// are added to, with a stream wait at each.
int ipa_verify_dev(vc_ctx* ctx, Table* t, IpaVerifyWork* w, size_t cnt, const uint32_t* d_chal, const uint32_t* d_tip,
                   const uint32_t* d_y, const uint32_t* d_point, uint32_t* d_com, const uint8_t* d_cinf, uint32_t* d_l,
                   const uint8_t* d_linf, uint32_t* d_r, const uint8_t* d_rinf, uint8_t* d_out, double* laps) {
    hipStream_t st = ctx->stream;
    const size_t N = w->N;
    uint8_t* d_fxy = w->fixed.as<uint8_t>();
    uint8_t* d_finf = d_fxy + w->chunk * 64;
    uint8_t* d_bad = w->bad.as<uint8_t>();
    double c0 = 0, c1 = 0, c2 = 0;
    if (laps) {
        VK_CHECK_HIP(hipStreamSynchronize(st));
        c0 = clock_us();
    }
    VK_LAUNCH(ctx, "ipa_verify_field", k_ipa_verify_field, cnt, 64, 0, d_chal, d_tip, d_y, d_point, w->pw.as<FrE>(),
              w->n_inv, (uint32_t)N, w->K, w->rows.as<uint32_t>(), w->vs.as<uint32_t>(), d_bad);
    if (laps) {
        VK_CHECK_HIP(hipStreamSynchronize(st));
        c1 = clock_us();
    }
    VK_TRY(msm_batch_run(ctx, t, N + 1, w->rows.p, cnt, /*mont=*/1, d_fxy, d_finf));
    if (laps) {
        VK_CHECK_HIP(hipStreamSynchronize(st));
        c2 = clock_us();
    }
    VK_LAUNCH(ctx, "ipa_verify_curve", k_ipa_verify_curve, (cnt * IPA_LP + 63) / 64, 64, 0, d_com, d_cinf, d_l, d_linf,
              d_r, d_rinf, w->vs.as<uint32_t>(), reinterpret_cast<const uint32_t*>(d_fxy), d_finf, d_bad, w->K, cnt,
              d_out);
    if (laps) {
        VK_CHECK_HIP(hipStreamSynchronize(st));
        laps[0] += c1 - c0, laps[1] += c2 - c1, laps[2] += clock_us() - c2;
    }
    return VC_OK;
}

}  // namespace vk

using namespace vk;

extern "C" int vc_ipa_verify_many(vc_ctx* ctx, int table, size_t N, size_t n, const uint64_t* com_xy,
                                  const uint8_t* com_inf, const uint64_t* points, const uint64_t* l_xy,
                                  const uint8_t* l_inf, const uint64_t* r_xy, const uint8_t* r_inf,
                                  const uint64_t* tip, const uint64_t* y, vc_transcript** transcripts,
                                  uint8_t* results) {
    using F = BN254Fr;
    if (!ctx || ctx->curve != VC_CURVE_BN254) return VC_E_INVALID;
    if (N < 2 || (N & (N - 1)) || N > (size_t(1) << 28)) return VC_E_INVALID;
    if (n && (!com_xy || !com_inf || !points || !l_xy || !l_inf || !r_xy || !r_inf || !tip || !y || !results))
        return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    if (t->n < N + 1) return VC_E_INVALID;
    if (n == 0) return VC_OK;
    int K = 0;
    while ((size_t(1) << K) < N) K++;
    const size_t T = 1 + 2 * (size_t)K;
    // a point that is a domain element w^i but not below N makes the reference divide by zero
    // (scheme.hip barycentric_panics): the whole call fails before any GPU work. A point >= r is
    // proof content gone wrong (verdict 0, found by the field kernel), not judged here.
    std::atomic<bool> domain_err{false};
    pool_for(0, n, 256, [&](size_t p) {
        uint64_t idx;
        if (!canonical_fr(points + 4 * p)) return;
        if (point_in_domain(reinterpret_cast<const uint32_t*>(points + 4 * p), N, &idx)) return;
        if (fe_eq<F>(fe_pow_u64<F>(canon_to_mont<F>(points + 4 * p), N), fe_one<F>())) domain_err = true;
    });
    if (domain_err) return VC_E_DOMAIN;

    // proofs per chunk: the rows (chunk x (N + 1) x 32 B) within 256 MB, at most 16384 (two waves of
    // the curve kernel per SIMD). VKZG_IPA_VERIFY_CHUNK (read per call): a test forces small chunks.
    size_t chunk = std::min<size_t>(16384, std::max<size_t>(1, (size_t(1) << 28) / ((N + 1) * 32)));
    if (const char* e = getenv("VKZG_IPA_VERIFY_CHUNK"))
        if (atol(e) > 0) chunk = (size_t)atol(e);
    chunk = std::min(chunk, n);
    const bool timing = host_timing();

    DevBuf d_chal(ctx), d_fr(ctx), d_pts(ctx), d_flags(ctx), d_res(ctx);
    IpaVerifyWork* work_raw = nullptr;
    VK_TRY(ipa_verify_work_new(ctx, N, chunk, &work_raw));  // rows, scalars, fixed commitments, w^i
    std::unique_ptr<IpaVerifyWork, void (*)(IpaVerifyWork*)> work(work_raw, ipa_verify_work_free);
    VK_TRY(d_chal.ensure(chunk * (size_t)(K + 1) * 32));
    VK_TRY(d_fr.ensure(chunk * 3 * 32));              // tip | y | point
    VK_TRY(d_pts.ensure(chunk * T * 64));             // C | L | R
    VK_TRY(d_flags.ensure(chunk * T));                // identity flags of C | L | R
    VK_TRY(d_res.ensure(n));
    hipStream_t st = ctx->stream;
    uint32_t* d_tip = d_fr.as<uint32_t>();
    uint32_t* d_y = d_tip + chunk * 8;
    uint32_t* d_point = d_y + chunk * 8;
    uint32_t* d_com = d_pts.as<uint32_t>();
    uint32_t* d_l = d_com + chunk * 16;
    uint32_t* d_r = d_l + chunk * (size_t)K * 16;
    uint8_t* d_cinf = d_flags.as<uint8_t>();
    uint8_t* d_linf = d_cinf + chunk;
    uint8_t* d_rinf = d_linf + chunk * (size_t)K;

    // a chunk's challenges: [w, x_0 .. x_{K-1}] per proof (the transcripts advance as vc_ipa_verify's)
    double lap_tr = 0;
    auto run_transcripts = [&](size_t lo, size_t cnt, std::vector<Fr>& chal) {
        const double c0 = timing ? clock_us() : 0.0;
        chal.resize(cnt * (size_t)(K + 1));
        ipa_host_challenges(lo, cnt, K, com_xy, com_inf, points, y, l_xy, l_inf, r_xy, r_inf, transcripts, chal.data());
        if (timing) lap_tr += clock_us() - c0;
    };
    std::vector<Fr> chal[2];
    struct UploadEvent {  // the last upload of a challenge buffer, waited for before it is refilled
        hipEvent_t e = nullptr;
        ~UploadEvent() {
            if (e) (void)hipEventDestroy(e);
        }
    } up;
    VK_CHECK_HIP(hipEventCreateWithFlags(&up.e, hipEventDisableTiming));
    double laps[3] = {0, 0, 0};  // field, fixed commit, curve
    const double call0 = timing ? clock_us() : 0.0;
    run_transcripts(0, chunk, chal[0]);
    size_t nchunks = 0;
    for (size_t lo = 0; lo < n; lo += chunk, nchunks++) {
        const size_t cnt = std::min(chunk, n - lo), nxt = lo + cnt;
        std::vector<Fr>& ch = chal[nchunks & 1];
        // the next chunk's transcripts on a helper thread (which runs them over the host pool) while
        // this thread feeds the device
        std::future<void> ahead;
        if (nxt < n) {
            std::vector<Fr>& into = chal[(nchunks + 1) & 1];
            if (nchunks > 0) VK_CHECK_HIP(hipEventSynchronize(up.e));  // (its last upload has left it)
            ahead = std::async(std::launch::async, [&, nxt] { run_transcripts(nxt, std::min(chunk, n - nxt), into); });
        }
        struct Join {  // every return path waits for the helper (it reads this frame)
            std::future<void>& f;
            ~Join() {
                if (f.valid()) f.wait();
            }
        } join{ahead};
        VK_CHECK_HIP(hipMemcpyAsync(d_chal.p, ch.data(), cnt * (size_t)(K + 1) * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipEventRecord(up.e, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_tip, tip + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_y, y + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_point, points + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_com, com_xy + 8 * lo, cnt * 64, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_l, l_xy + 8 * lo * K, cnt * (size_t)K * 64, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_r, r_xy + 8 * lo * K, cnt * (size_t)K * 64, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_cinf, com_inf + lo, cnt, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_linf, l_inf + lo * K, cnt * (size_t)K, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_rinf, r_inf + lo * K, cnt * (size_t)K, hipMemcpyHostToDevice, st));
        VK_TRY(ipa_verify_dev(ctx, t, work.get(), cnt, d_chal.as<uint32_t>(), d_tip, d_y, d_point, d_com, d_cinf, d_l,
                              d_linf, d_r, d_rinf, d_res.as<uint8_t>() + lo, timing ? laps : nullptr));
    }
    VK_CHECK_HIP(hipMemcpyAsync(results, d_res.p, n, hipMemcpyDeviceToHost, st));
    VK_CHECK_HIP(hipStreamSynchronize(st));
    if (timing)
        fprintf(stderr,
                "[ipa_verify_many] n=%zu N=%zu chunks=%zu: transcripts %.1f us (one chunk ahead of the device), "
                "field %.1f us, fixed commit %.1f us, curve %.1f us, call %.1f us\n",
                n, N, nchunks, lap_tr, laps[0], laps[1], laps[2], clock_us() - call0);
    return VC_OK;
}

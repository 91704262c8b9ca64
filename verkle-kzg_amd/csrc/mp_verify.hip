// Multiproof batch verification on the GPU (vc_multiproof_verify_many_ipa / _kzg,
// vc_multiproof_claims_many): P independent multiproofs, one verdict (or one claim) each. Per chunk
// of proofs -- capped in proofs and in total queries, so the workspace does not grow with P -- the
// chunk's arrays are uploaded once and nothing of a proof crosses to the host until the verdicts
// (or claims) are copied back (the fixed commit's own normalisation excepted, as in ipa_many.hip):
//   transcript  k_mpv_transcript, a lane per proof: r from the byte-stream feeder over the proof's
//               (C, z, y) records (the block buffer a column of LDS), t after D; flags y_i >= r and
//               a t that is an integer below N;
//   coef        k_mpv_coef, a wave per proof: r^i / (t - z_i) as canonical words, one inversion per
//               proof (the lanes' own suffix products, the lanes' totals multiplied across the wave,
//               r^i stepping by r^64);
//   sums        k_mpv_esum<LP>, LP lanes per proof: validates the proof's C_i (rewritten in
//               Montgomery form), sums coef_i C_i over the lane's terms with one shared chain of 254
//               doublings, folds the LP partial sums with xor shuffles. LP = 8 for proofs of at most
//               MPV_SHORT_Q queries, a wave (LP = 64) for the longer ones: k_ipa_verify_curve's
//               trade-off, fewer lanes double less, more lanes shorten the serial chain;
//   claim       k_mpv_claim, a lane per proof: validates D, E to affine and compressed, E - D to
//               affine and compressed (two binary inversions of a lane's own);
//   inner       KZG: k_kzg_verify over (E - D, t, proof, y) (pairing.hip; verify_point takes no
//               transcript). IPA: k_mpv_inner_chal, a lane per proof, hashes [w, x_k] from the state
//               t "t" "E" E under the "multiproof" DST, then vc_ipa_verify_many's field kernel, fixed
//               commit and curve kernel (ipa_verify.hip ipa_verify_dev);
//   mask        k_mpv_mask: an entry flagged anywhere above gets the verdict 0.
// The arithmetic and the message layouts are csrc/mp_verify.hpp, the text
// tests/cpp/mp_verify_check.cpp runs on the host. Every status other than VC_OK is decided on the
// host before the first upload.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "ctx.hpp"
#include "ec29.hpp"
#include "kzg_many.hpp"
#include "mp_verify.hpp"
#include "scheme_internal.hpp"

namespace vk {

using namespace mpv;

constexpr size_t MPV_CHUNK_P = 8192;        // proofs per chunk (the inner IPA's rows: 16 MB at N = 256 .. the bound below)
constexpr size_t MPV_CHUNK_Q = size_t(1) << 18;  // queries per chunk: 137 B each of workspace, 36 MB
constexpr uint32_t MPV_SHORT_Q = 32;        // at most this many queries: 8 lanes per proof, else a wave

// what the front kernels share: the chunk's queries and proofs
struct MpvArgs {
    const uint32_t* qoff;  // cnt + 1 offsets into the chunk's query arrays
    uint32_t* com;         // 16 canonical words per query; Montgomery once k_mpv_esum has validated them
    const uint8_t* cinf;
    const uint32_t* z;     // two words per query
    const uint32_t* y;     // 8 canonical words per query
    uint32_t* coef;        // 8 words per query
    const uint32_t* dxy;   // 16 canonical words per proof
    const uint8_t* dinf;
    uint32_t *r, *tm, *tc; // per proof: r, t (Montgomery), t (canonical)
    G1A* E;
    uint32_t *cxy, *ec, *cc;  // per proof: E - D affine (16), E and E - D compressed (8 each)
    uint8_t* cflag;        // E - D is the identity
    uint8_t* bad;
    uint32_t cnt, N;
};

// (42-46 scalar registers are spilled to vector lanes around the unrolled compression, whose 64
// round constants and the kernel's pointers compete for them, whether the pointers come as MpvArgs or
// one by one: v_writelane / v_readlane beside ~2,000 vector instructions per block, no scratch)
__global__ __launch_bounds__(64) void k_mpv_transcript(MpvArgs A) {
    __shared__ uint32_t blk[16 * 64];
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= A.cnt) return;
    const uint32_t q0 = A.qoff[p], q = A.qoff[p + 1] - q0;
    bool y_ok = true;
    const FrE r = challenge_r(blk + threadIdx.x, 64, q, A.com + 16 * (size_t)q0, A.cinf + q0, A.z + 2 * (size_t)q0,
                              A.y + 8 * (size_t)q0, y_ok);
    const FrE rc = fe_from_mont<BN254Fr>(r);
    uint32_t dw[16], dc[8];
    for (int k = 0; k < 16; k++) dw[k] = A.dxy[16 * (size_t)p + k];
    compress_words(dw, A.dinf[p] != 0, dc);
    const FrE t = challenge_t(rc.v, dc);
    const FrE tc = fe_from_mont<BN254Fr>(t);
    uint64_t idx = 0;
    const bool in_dom = point_in_domain(tc.v, A.N, &idx);
    fr_store(r, A.r + 8 * (size_t)p);
    fr_store(t, A.tm + 8 * (size_t)p);
    fr_store(tc, A.tc + 8 * (size_t)p);
    A.bad[p] = (!y_ok || in_dom) ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_mpv_coef(MpvArgs A) {
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    const uint32_t q0 = A.qoff[p], q = A.qoff[p + 1] - q0;
    const FrE r = fr_load(A.r + 8 * (size_t)p), t = fr_load(A.tm + 8 * (size_t)p);
    const uint32_t* z = A.z + 2 * (size_t)q0;
    uint32_t* coef = A.coef + 8 * (size_t)q0;
    bool bad = false;
    FrE tot = coef_suffix_pass(q, lane, t, z, coef, bad);
    FrE oth = fe_one<BN254Fr>();
    for (uint32_t s = 1; s < 64; s <<= 1) {
        const FrE pt = shfl_xor_pod(tot, s);
        kzgm::others_step<BN254Fr>(tot, oth, pt);
    }
    // (tot is the proof's product on every lane: the inversion below is uniform over the wave)
    const FrE inv = fr_mul(fe_inv_bin<BN254Fr>(tot), oth);
    FrE r64 = r;
    for (int k = 0; k < 6; k++) r64 = fr_mul(r64, r64);
    coef_finish_pass(q, lane, t, z, r, r64, inv, coef);
    if (__any(bad) && lane == 0) A.bad[p] = 1;
}

// LP lanes per proof; lane `sub` takes queries sub, sub + LP, .. of proof ids[slot]
template <int LP>
__global__ __launch_bounds__(64) void k_mpv_esum(MpvArgs A, const uint32_t* __restrict__ ids, uint32_t n_ids) {
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
    const uint32_t slot = gid / LP, sub = gid % LP;
    const bool active = slot < n_ids;
    const uint32_t p = active ? ids[slot] : 0;
    const uint32_t q0 = active ? A.qoff[p] : 0, q = active ? A.qoff[p + 1] - q0 : 0;
    const int count = sub < q ? (int)((q - sub + LP - 1) / LP) : 0;
    uint32_t* com = A.com + 16 * (size_t)q0;
    const uint8_t* cinf = A.cinf + q0;
    int ok = active && !A.bad[p];
    if (ok)
        for (int j = 0; j < count; j++) {
            const uint32_t i = sub + (uint32_t)j * LP;
            if (cinf[i]) continue;
            uint32_t* pt = com + 16 * (size_t)i;
            uint32_t w[16];
            for (int k = 0; k < 16; k++) w[k] = pt[k];
            G1P P;
            if (!ate::g1_load(w, P)) {
                ok = 0;
                break;
            }
            for (int k = 0; k < 8; k++) {
                pt[k] = P.x.v[k];
                pt[8 + k] = P.y.v[k];
            }
        }
    for (uint32_t m = 1; m < (uint32_t)LP; m <<= 1) ok &= __shfl_xor(ok, m, 64);
    G1A S = BN254G1::zero();
    if (ok) {
        const uint32_t* sc = A.coef + 8 * (size_t)q0;
        S = var_partial_sum(
            count,
            [&](int j, G1P& P) {
                const uint32_t i = sub + (uint32_t)j * LP;
                if (cinf[i]) return false;
                const uint32_t* pt = com + 16 * (size_t)i;
                for (int k = 0; k < 8; k++) {
                    P.x.v[k] = pt[k];
                    P.y.v[k] = pt[8 + k];
                }
                return true;
            },
            [&](int j, int b) { return ((sc[8 * (size_t)(sub + (uint32_t)j * LP) + (b >> 5)] >> (b & 31)) & 1u) != 0; });
    }
    for (uint32_t m = 1; m < (uint32_t)LP; m <<= 1) S = BN254G1::add(S, shfl_xor_pod(S, m));
    if (active && sub == 0) {
        A.E[p] = S;
        if (!ok) A.bad[p] = 1;
    }
}

__global__ __launch_bounds__(64) void k_mpv_claim(MpvArgs A) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= A.cnt) return;
    bool bad = A.bad[p] != 0;
    const bool d_inf = A.dinf[p] != 0;
    G1P D{fe_zero<BN254Fq>(), fe_zero<BN254Fq>()};
    if (!bad && !d_inf) {
        uint32_t w[16];
        for (int k = 0; k < 16; k++) w[k] = A.dxy[16 * (size_t)p + k];
        bad = !ate::g1_load(w, D);
    }
    uint32_t e[8], cxy[16], c[8];
    bool c_inf = true;
    if (bad) {
        for (int k = 0; k < 16; k++) cxy[k] = 0;
        for (int k = 0; k < 8; k++) e[k] = c[k] = 0;
        A.bad[p] = 1;
    } else {
        claim_of(A.E[p], D, d_inf, e, cxy, c_inf, c);
    }
    for (int k = 0; k < 16; k++) A.cxy[16 * (size_t)p + k] = cxy[k];
    for (int k = 0; k < 8; k++) {
        A.ec[8 * (size_t)p + k] = e[k];
        A.cc[8 * (size_t)p + k] = c[k];
    }
    A.cflag[p] = c_inf ? 1 : 0;
}

// [w, x_0 .. x_{K-1}] of the inner IPA proofs, a lane per proof (an entry already flagged hashes
// whatever its words hold: its verdict is masked)
__global__ __launch_bounds__(64) void k_mpv_inner_chal(MpvArgs A, int K, const uint32_t* __restrict__ ipa_y,
                                                       const uint32_t* __restrict__ l_xy,
                                                       const uint8_t* __restrict__ l_inf,
                                                       const uint32_t* __restrict__ r_xy,
                                                       const uint8_t* __restrict__ r_inf, uint32_t* __restrict__ chal) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= A.cnt) return;
    uint32_t t[8], e[8], c[8], y[8];
    for (int k = 0; k < 8; k++) {
        t[k] = A.tc[8 * (size_t)p + k];
        e[k] = A.ec[8 * (size_t)p + k];
        c[k] = A.cc[8 * (size_t)p + k];
        y[k] = ipa_y[8 * (size_t)p + k];
    }
    const size_t at = (size_t)p * (size_t)K;
    inner_challenges(K, t, e, c, y, l_xy + 16 * at, l_inf + at, r_xy + 16 * at, r_inf + at,
                     chal + (size_t)p * (size_t)(K + 1) * 8);
}

__global__ void k_mpv_mask(const uint8_t* __restrict__ bad, uint32_t n, uint8_t* __restrict__ out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) out[p] = (out[p] && !bad[p]) ? 1 : 0;
}

namespace {

struct Args {
    int mode;  // 0: claims, 1: IPA, 2: KZG
    int table;
    const vc_kzg_vk* vk;
    size_t N, P;
    const uint64_t* q_ptr;
    size_t Q;
    const uint64_t *com_xy, *z, *y, *d_xy;
    const uint8_t *com_inf, *d_inf;
    const uint64_t *l_xy, *r_xy, *tip, *ipa_y, *kzg_xy, *kzg_y;
    const uint8_t *l_inf, *r_inf, *kzg_inf;
    uint64_t *c_xy, *t;
    uint8_t *c_inf, *malformed, *results;
};

int run(vc_ctx* ctx, Table* tb, const Args& a) {
    const size_t N = a.N, P = a.P;
    int K = 0;
    while ((size_t(1) << K) < N) K++;
    auto q_lo = [&](size_t p) { return a.q_ptr ? (size_t)a.q_ptr[p] : p * a.Q; };
    size_t cap_p = MPV_CHUNK_P, cap_q = MPV_CHUNK_Q;
    if (a.mode == 1) cap_p = std::min(cap_p, std::max<size_t>(1, (size_t(1) << 28) / ((N + 1) * 32)));
    // VKZG_MPV_CHUNK_P / VKZG_MPV_CHUNK_Q (read per call): a test lowers the proof cap, or makes the
    // query cap end the chunks
    auto lowered = [](const char* e, size_t cap) {
        const long v = e ? atol(e) : 0;
        return v > 0 ? std::min<size_t>((size_t)v, cap) : cap;
    };
    cap_p = lowered(getenv("VKZG_MPV_CHUNK_P"), cap_p);
    cap_q = lowered(getenv("VKZG_MPV_CHUNK_Q"), cap_q);
    cap_p = std::min(cap_p, P);
    const size_t buf_q = std::min(std::max<size_t>(cap_q, VC_MPV_Q_MAX), q_lo(P) - q_lo(0));  // (a chunk takes one proof at least)
    const bool timing = host_timing();
    const double call0 = timing ? clock_us() : 0.0;
    hipStream_t st = ctx->stream;

    DevBuf d_com(ctx), d_y(ctx), d_coef(ctx), d_z(ctx), d_cinf(ctx), d_qoff(ctx), d_ids(ctx), d_dxy(ctx), d_fr(ctx), d_E(ctx),
        d_claim(ctx), d_flags(ctx), d_res(ctx), d_inner(ctx), d_iflags(ctx), d_chal(ctx);
    VK_TRY(d_com.ensure(buf_q * 64));
    VK_TRY(d_y.ensure(buf_q * 32));
    VK_TRY(d_coef.ensure(buf_q * 32));
    VK_TRY(d_z.ensure(buf_q * 8));
    VK_TRY(d_cinf.ensure(buf_q));
    VK_TRY(d_qoff.ensure((cap_p + 1) * 4));
    VK_TRY(d_ids.ensure(cap_p * 4));
    VK_TRY(d_dxy.ensure(cap_p * 64));
    VK_TRY(d_fr.ensure(cap_p * 3 * 32));     // r | t | t canonical
    VK_TRY(d_E.ensure(cap_p * sizeof(G1A)));
    VK_TRY(d_claim.ensure(cap_p * 128));     // E - D affine | E compressed | E - D compressed
    VK_TRY(d_flags.ensure(cap_p * 3));       // D's flags | the claims' flags | bad
    VK_TRY(d_res.ensure(cap_p));
    MpvArgs A{};
    A.qoff = d_qoff.as<uint32_t>();
    A.com = d_com.as<uint32_t>();
    A.cinf = d_cinf.as<uint8_t>();
    A.z = d_z.as<uint32_t>();
    A.y = d_y.as<uint32_t>();
    A.coef = d_coef.as<uint32_t>();
    A.dxy = d_dxy.as<uint32_t>();
    A.r = d_fr.as<uint32_t>();
    A.tm = A.r + cap_p * 8;
    A.tc = A.tm + cap_p * 8;
    A.E = d_E.as<G1A>();
    A.cxy = d_claim.as<uint32_t>();
    A.ec = A.cxy + cap_p * 16;
    A.cc = A.ec + cap_p * 8;
    uint8_t* d_dinf = d_flags.as<uint8_t>();
    A.dinf = d_dinf;
    A.cflag = d_dinf + cap_p;
    A.bad = A.cflag + cap_p;
    A.N = (uint32_t)N;
    // the inner proofs: IPA L | R, tip | y and their flags, the challenges; KZG pi, y and flags
    IpaVerifyWork* work_raw = nullptr;
    std::unique_ptr<IpaVerifyWork, void (*)(IpaVerifyWork*)> work(nullptr, ipa_verify_work_free);
    uint32_t *d_l = nullptr, *d_r = nullptr, *d_tip = nullptr, *d_iy = nullptr, *d_pi = nullptr;
    uint8_t *d_linf = nullptr, *d_rinf = nullptr, *d_pinf = nullptr;
    if (a.mode == 1) {
        VK_TRY(ipa_verify_work_new(ctx, N, cap_p, &work_raw));
        work.reset(work_raw);
        VK_TRY(d_inner.ensure(cap_p * (2 * (size_t)K * 64 + 64)));
        VK_TRY(d_iflags.ensure(cap_p * 2 * (size_t)K));
        VK_TRY(d_chal.ensure(cap_p * (size_t)(K + 1) * 32));
        d_l = d_inner.as<uint32_t>();
        d_r = d_l + cap_p * (size_t)K * 16;
        d_tip = d_r + cap_p * (size_t)K * 16;
        d_iy = d_tip + cap_p * 8;
        d_linf = d_iflags.as<uint8_t>();
        d_rinf = d_linf + cap_p * (size_t)K;
    } else if (a.mode == 2) {
        VK_TRY(d_inner.ensure(cap_p * 96));
        VK_TRY(d_iflags.ensure(cap_p));
        d_pi = d_inner.as<uint32_t>();
        d_iy = d_pi + cap_p * 16;
        d_pinf = d_iflags.as<uint8_t>();
    }

    double lap_up = 0, lap_tr = 0, lap_coef = 0, lap_sum = 0, lap_claim = 0, lap_inner = 0, lap_back = 0;
    double ipa_laps[3] = {0, 0, 0};
    auto lap = [&](double& into, double& since) -> int {  // (timing only: waits for the stream)
        if (!timing) return VC_OK;
        VK_CHECK_HIP(hipStreamSynchronize(st));
        const double now = clock_us();
        into += now - since;
        since = now;
        return VC_OK;
    };
    std::vector<uint32_t> qoff, ids_short, ids_long;
    size_t nchunks = 0;
    for (size_t lo = 0; lo < P; nchunks++) {
        size_t cnt = 0;
        const size_t qbase = q_lo(lo);
        qoff.assign(1, 0);
        ids_short.clear();
        ids_long.clear();
        while (lo + cnt < P && cnt < cap_p) {
            const size_t q = q_lo(lo + cnt + 1) - q_lo(lo + cnt);
            if (cnt > 0 && qoff.back() + q > cap_q) break;
            (q <= MPV_SHORT_Q ? ids_short : ids_long).push_back((uint32_t)cnt);
            qoff.push_back(qoff.back() + (uint32_t)q);
            cnt++;
        }
        const size_t qn = qoff.back();
        A.cnt = (uint32_t)cnt;
        double c0 = timing ? clock_us() : 0.0;
        VK_CHECK_HIP(hipMemcpyAsync(d_com.p, a.com_xy + 8 * qbase, qn * 64, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_cinf.p, a.com_inf + qbase, qn, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_z.p, a.z + qbase, qn * 8, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_y.p, a.y + 4 * qbase, qn * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_qoff.p, qoff.data(), (cnt + 1) * 4, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_dxy.p, a.d_xy + 8 * lo, cnt * 64, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_dinf, a.d_inf + lo, cnt, hipMemcpyHostToDevice, st));
        uint32_t* d_short = d_ids.as<uint32_t>();
        uint32_t* d_long = d_short + ids_short.size();
        if (!ids_short.empty())
            VK_CHECK_HIP(hipMemcpyAsync(d_short, ids_short.data(), ids_short.size() * 4, hipMemcpyHostToDevice, st));
        if (!ids_long.empty())
            VK_CHECK_HIP(hipMemcpyAsync(d_long, ids_long.data(), ids_long.size() * 4, hipMemcpyHostToDevice, st));
        if (a.mode == 1) {
            const size_t k = (size_t)K;
            VK_CHECK_HIP(hipMemcpyAsync(d_l, a.l_xy + 8 * lo * k, cnt * k * 64, hipMemcpyHostToDevice, st));
            VK_CHECK_HIP(hipMemcpyAsync(d_r, a.r_xy + 8 * lo * k, cnt * k * 64, hipMemcpyHostToDevice, st));
            VK_CHECK_HIP(hipMemcpyAsync(d_linf, a.l_inf + lo * k, cnt * k, hipMemcpyHostToDevice, st));
            VK_CHECK_HIP(hipMemcpyAsync(d_rinf, a.r_inf + lo * k, cnt * k, hipMemcpyHostToDevice, st));
            VK_CHECK_HIP(hipMemcpyAsync(d_tip, a.tip + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
            VK_CHECK_HIP(hipMemcpyAsync(d_iy, a.ipa_y + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
        } else if (a.mode == 2) {
            VK_CHECK_HIP(hipMemcpyAsync(d_pi, a.kzg_xy + 8 * lo, cnt * 64, hipMemcpyHostToDevice, st));
            VK_CHECK_HIP(hipMemcpyAsync(d_pinf, a.kzg_inf + lo, cnt, hipMemcpyHostToDevice, st));
            VK_CHECK_HIP(hipMemcpyAsync(d_iy, a.kzg_y + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
        }
        VK_TRY(lap(lap_up, c0));
        const size_t lane_blocks = (cnt + 63) / 64;
        VK_LAUNCH(ctx, "mpv_transcript", k_mpv_transcript, lane_blocks, 64, 0, A);
        VK_TRY(lap(lap_tr, c0));
        VK_LAUNCH(ctx, "mpv_coef", k_mpv_coef, cnt, 64, 0, A);
        VK_TRY(lap(lap_coef, c0));
        if (!ids_short.empty())
            VK_LAUNCH(ctx, "mpv_esum8", k_mpv_esum<8>, (ids_short.size() * 8 + 63) / 64, 64, 0, A, d_short,
                      (uint32_t)ids_short.size());
        if (!ids_long.empty())
            VK_LAUNCH(ctx, "mpv_esum64", k_mpv_esum<64>, ids_long.size(), 64, 0, A, d_long, (uint32_t)ids_long.size());
        VK_TRY(lap(lap_sum, c0));
        VK_LAUNCH(ctx, "mpv_claim", k_mpv_claim, lane_blocks, 64, 0, A);
        VK_TRY(lap(lap_claim, c0));
        if (a.mode == 0) {
            VK_CHECK_HIP(hipMemcpyAsync(a.c_xy + 8 * lo, A.cxy, cnt * 64, hipMemcpyDeviceToHost, st));
            VK_CHECK_HIP(hipMemcpyAsync(a.c_inf + lo, A.cflag, cnt, hipMemcpyDeviceToHost, st));
            VK_CHECK_HIP(hipMemcpyAsync(a.t + 4 * lo, A.tc, cnt * 32, hipMemcpyDeviceToHost, st));
            VK_CHECK_HIP(hipMemcpyAsync(a.malformed + lo, A.bad, cnt, hipMemcpyDeviceToHost, st));
        } else {
            uint8_t* d_out = d_res.as<uint8_t>();
            if (a.mode == 1) {
                VK_LAUNCH(ctx, "mpv_inner_chal", k_mpv_inner_chal, lane_blocks, 64, 0, A, K, d_iy, d_l, d_linf, d_r, d_rinf,
                          d_chal.as<uint32_t>());
                VK_TRY(ipa_verify_dev(ctx, tb, work.get(), cnt, d_chal.as<uint32_t>(), d_tip, d_iy, A.tc, A.cxy, A.cflag,
                                      d_l, d_linf, d_r, d_rinf, d_out, timing ? ipa_laps : nullptr));
            } else {
                VK_TRY(kzg_verify_dev(ctx, a.vk, cnt, A.cxy, A.cflag, A.tc, d_pi, d_pinf, d_iy, d_out));
            }
            VK_LAUNCH(ctx, "mpv_mask", k_mpv_mask, (cnt + 255) / 256, 256, 0, A.bad, (uint32_t)cnt, d_out);
            VK_TRY(lap(lap_inner, c0));
            VK_CHECK_HIP(hipMemcpyAsync(a.results + lo, d_out, cnt, hipMemcpyDeviceToHost, st));
        }
        // (the chunk's host vectors and the workspace are reused by the next chunk)
        VK_CHECK_HIP(hipStreamSynchronize(st));
        if (timing) lap_back += clock_us() - c0;
        lo += cnt;
    }
    if (timing)
        fprintf(stderr,
                "[mp_verify_many] mode=%d P=%zu N=%zu queries=%zu chunks=%zu: upload %.1f us, transcript %.1f us, "
                "coefficients %.1f us, sums %.1f us, claims %.1f us, inner %.1f us (IPA: field %.1f us, fixed commit "
                "%.1f us, curve %.1f us), read-back %.1f us, call %.1f us\n",
                a.mode, P, N, q_lo(P) - q_lo(0), nchunks, lap_up, lap_tr, lap_coef, lap_sum, lap_claim, lap_inner,
                ipa_laps[0], ipa_laps[1], ipa_laps[2], lap_back, clock_us() - call0);
    return VC_OK;
}

// every status other than VC_OK, then the run
int entry(vc_ctx* ctx, const Args& a) {
    if (!ctx || ctx->curve != VC_CURVE_BN254) return VC_E_INVALID;
    if (a.mode == 2 && (!a.vk || kzg_vk_curve(a.vk) != VC_CURVE_BN254)) return VC_E_INVALID;
    const size_t N = a.N, P = a.P;
    if (N < 2 || (N & (N - 1)) || N > (size_t(1) << 28) || P >= (size_t(1) << 31)) return VC_E_INVALID;
    if (P) {
        if (!a.com_xy || !a.com_inf || !a.z || !a.y || !a.d_xy || !a.d_inf) return VC_E_INVALID;
        if (a.mode == 0 && (!a.c_xy || !a.c_inf || !a.t || !a.malformed)) return VC_E_INVALID;
        if (a.mode == 1 && (!a.l_xy || !a.l_inf || !a.r_xy || !a.r_inf || !a.tip || !a.ipa_y || !a.results))
            return VC_E_INVALID;
        if (a.mode == 2 && (!a.kzg_xy || !a.kzg_inf || !a.kzg_y || !a.results)) return VC_E_INVALID;
        if (a.q_ptr) {
            for (size_t p = 0; p < P; p++)
                if (a.q_ptr[p + 1] <= a.q_ptr[p] || a.q_ptr[p + 1] - a.q_ptr[p] > VC_MPV_Q_MAX) return VC_E_INVALID;
        } else if (a.Q == 0 || a.Q > VC_MPV_Q_MAX) {
            return VC_E_INVALID;
        }
    }
    Guard g(ctx);
    Table* tb = nullptr;
    if (a.mode == 1) {
        tb = ctx->table(a.table);
        if (!tb) return VC_E_TABLE;
        if (tb->n < N + 1) return VC_E_INVALID;
    }
    if (P == 0) return VC_OK;
    const size_t q0 = a.q_ptr ? (size_t)a.q_ptr[0] : 0, q1 = a.q_ptr ? (size_t)a.q_ptr[P] : P * a.Q;
    for (size_t i = q0; i < q1; i++)
        if (a.z[i] >= N) return VC_E_DOMAIN;
    return run(ctx, tb, a);
}

}  // namespace
}  // namespace vk

using namespace vk;

extern "C" int vc_multiproof_claims_many(vc_ctx* ctx, size_t N, size_t P, const uint64_t* q_ptr, size_t Q,
                                         const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z,
                                         const uint64_t* y, const uint64_t* d_xy, const uint8_t* d_inf, uint64_t* c_xy,
                                         uint8_t* c_inf, uint64_t* t, uint8_t* malformed) {
    Args a{};
    a.mode = 0, a.N = N, a.P = P, a.q_ptr = q_ptr, a.Q = Q;
    a.com_xy = com_xy, a.com_inf = com_inf, a.z = z, a.y = y, a.d_xy = d_xy, a.d_inf = d_inf;
    a.c_xy = c_xy, a.c_inf = c_inf, a.t = t, a.malformed = malformed;
    return entry(ctx, a);
}

extern "C" int vc_multiproof_verify_many_ipa(vc_ctx* ctx, int table, size_t N, size_t P, const uint64_t* q_ptr, size_t Q,
                                             const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z,
                                             const uint64_t* y, const uint64_t* d_xy, const uint8_t* d_inf,
                                             const uint64_t* l_xy, const uint8_t* l_inf, const uint64_t* r_xy,
                                             const uint8_t* r_inf, const uint64_t* tip, const uint64_t* ipa_y,
                                             uint8_t* results) {
    Args a{};
    a.mode = 1, a.table = table, a.N = N, a.P = P, a.q_ptr = q_ptr, a.Q = Q;
    a.com_xy = com_xy, a.com_inf = com_inf, a.z = z, a.y = y, a.d_xy = d_xy, a.d_inf = d_inf;
    a.l_xy = l_xy, a.l_inf = l_inf, a.r_xy = r_xy, a.r_inf = r_inf, a.tip = tip, a.ipa_y = ipa_y;
    a.results = results;
    return entry(ctx, a);
}

extern "C" int vc_multiproof_verify_many_kzg(vc_ctx* ctx, const vc_kzg_vk* vk, size_t N, size_t P, const uint64_t* q_ptr,
                                             size_t Q, const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z,
                                             const uint64_t* y, const uint64_t* d_xy, const uint8_t* d_inf,
                                             const uint64_t* kzg_xy, const uint8_t* kzg_inf, const uint64_t* kzg_y,
                                             uint8_t* results) {
    Args a{};
    a.mode = 2, a.vk = vk, a.N = N, a.P = P, a.q_ptr = q_ptr, a.Q = Q;
    a.com_xy = com_xy, a.com_inf = com_inf, a.z = z, a.y = y, a.d_xy = d_xy, a.d_inf = d_inf;
    a.kzg_xy = kzg_xy, a.kzg_inf = kzg_inf, a.kzg_y = kzg_y;
    a.results = results;
    return entry(ctx, a);
}

// IPA prover, verifier and the commitment proof (reference: vector-commit/src/ipa/mod.rs).
// IPA prover without point folding: the reference folds the generators every round
// (vec_add_and_distribute on points, utils.rs:31-38 -- m full scalar multiplications per
// round). Here the folded generator g^(k)_j is kept as scalar coefficients over the ORIGINAL
// CRS (coeff_i, the prover-side twin of the verifier's points_coeffs), so each round's
// L and R are two width-(N+1) fixed-base commitments (q is base N) served by the
// precomputed window tables of fb_table.hip. Same group elements, no point folding.
#include "ipa_rounds.hpp"
#include "protocol.hpp"

namespace vk {

using ipar::inner;

// Closes round r of proof p: L and R (commits 2 p and 2 p + 1 of the round's batch) go into the
// proof and the transcript, which gives the challenge x, and a (b, the host coefficients: null
// where there are none) are folded by it (ipa_rounds.hpp). Returns x.
static Fr close_round(size_t r, size_t p, const uint64_t* oxy, const uint8_t* oinf, vc_ipa_proof* proofs,
                      vc_transcript* tr, size_t N, std::vector<Fr>& a, std::vector<Fr>* b, Fr* coeff) {
    const uint64_t* Lxy = oxy + (2 * p) * 8;
    const uint64_t* Rxy = oxy + (2 * p + 1) * 8;
    memcpy(proofs[p].l_xy + r * 8, Lxy, 64);
    memcpy(proofs[p].r_xy + r * 8, Rxy, 64);
    proofs[p].l_inf[r] = oinf[2 * p];
    proofs[p].r_inf[r] = oinf[2 * p + 1];
    transcript_append_point(tr, Lxy, oinf[2 * p], "L");
    transcript_append_point(tr, Rxy, oinf[2 * p + 1], "R");
    const Fr x = transcript_digest(tr, "x");
    const size_t m = N >> r;
    ipar::round_fold(x, N, m, m / 2, a, b, coeff);
    return x;
}

// the challenges x_0 .. x_{K-1} of a proof, off a transcript that stands before its first L
static std::vector<Fr> read_challenges(vc_transcript* tr, const vc_ipa_proof* pr) {
    std::vector<Fr> xs(pr->rounds);
    for (size_t k = 0; k < xs.size(); k++) {
        transcript_append_point(tr, pr->l_xy + 8 * k, pr->l_inf[k], "L");
        transcript_append_point(tr, pr->r_xy + 8 * k, pr->r_inf[k], "R");
        xs[k] = transcript_digest(tr, "x");
    }
    return xs;
}

// the verifiers' variable part: (prod x) C + sum_k P_k L_k + P_k x_k^2 R_k over the points (C, L_0,
// R_0, ..) with the scalars vs of ipar::verifier_scalars -- one small MSM (msm_points)
static int var_part(vc_ctx* ctx, const uint64_t* cxy, uint8_t cinf, const vc_ipa_proof* pr, const std::vector<Fr>& vs,
                    Acc* out) {
    const size_t K = pr->rounds;
    std::vector<uint64_t> vxy(8 * (1 + 2 * K));
    std::vector<uint8_t> vinf(1 + 2 * K);
    memcpy(&vxy[0], cxy, 64);
    vinf[0] = cinf;
    for (size_t k = 0; k < K; k++) {
        memcpy(&vxy[8 * (1 + 2 * k)], pr->l_xy + 8 * k, 64);
        memcpy(&vxy[8 * (2 + 2 * k)], pr->r_xy + 8 * k, 64);
        vinf[1 + 2 * k] = pr->l_inf[k];
        vinf[2 + 2 * k] = pr->r_inf[k];
    }
    return msm_points(ctx, vxy.data(), vinf.data(), vs, out);
}

// ---------------------------------------------------------------- IPA prove (a8/a9)
struct IpaState {
    std::vector<Fr> a, b, coeff;
    Fr eval, w;
    vc_transcript* tr;
    bool own;
};

int ipa_prove_impl(vc_ctx* ctx, Table* t, size_t N, const std::vector<std::vector<Fr>>& data,
                   const std::vector<Acc>& coms, const std::vector<Fr>& points, vc_transcript** trs,
                   vc_ipa_proof* proofs) {
    const size_t B = data.size();
    if (!is_pow2(N) || t->n < N + 1) return VC_E_INVALID;
    size_t K = 0;
    while ((1ull << K) < N) K++;
    Fr omega = bn254_group_gen(N);
    std::vector<IpaState> st(B);
    for (size_t p = 0; p < B; p++) {
        if (proofs[p].rounds < K || !proof_ok(&proofs[p])) return VC_E_INVALID;
        if (barycentric_panics(N, points[p])) return VC_E_DOMAIN;
    }
    // the per-proof host work (barycentric weights, transcripts, scalar rows, folds: ~600 field
    // multiplies per proof per round) is independent across proofs: up to 16 host threads
    auto par_for = [&](auto fn) { pool_for(0, B, 16, fn); };  // the persistent host pool (host/pool.hpp)
    par_for([&](size_t p) {
        IpaState& s = st[p];
        s.a = data[p];
        s.b = barycentric(N, points[p], omega);
        s.eval = inner(s.a.data(), s.b.data(), N);
        s.own = !(trs && trs[p]);
        s.tr = s.own ? vc_transcript_new("ipa") : trs[p];
        uint64_t cxy[8];
        uint8_t cinf;
        aff_of(coms[p], cxy, &cinf);
        transcript_append_point(s.tr, cxy, cinf, "C");
        transcript_append_fr(s.tr, points[p], "input point");
        transcript_append_fr(s.tr, s.eval, "output point");
        s.w = transcript_digest(s.tr, "w");
        s.coeff.assign(N, fe_one<F>());
    });
    // L (R) of a round has non-zeros only at the N / 2 bases i with i mod m >= m / 2 (< m / 2) and
    // at q. (Rows compacted to those N / 2 + 1 bases on the latency path -- half the threads and half
    // the block partials the host adds -- measured slower, prove 0.80 vs 0.77 ms, kernel 62 vs 56 us
    // per round: profiles/r05/ipa_compact/. The zero lanes of the full rows make the first adds of
    // the block tree identity adds, which the compacted rows replace by real ones. Removed.)
    const size_t W = N + 1;
    // the rows on the device (IpaRows, the latency path's commit kernel): the host keeps a, b and
    // the q' <a, b> terms; the coefficient rows live in device memory and are folded there. Off the
    // latency path the host builds every row.
    const bool dev_rows = fb_small_path(ctx, t, N + 1, 2 * B);
    DevBuf d_coeff(ctx);
    std::vector<Fr> ones;  // round 0's coefficients (the upload reads it until the first round ends)
    Fr *pa = nullptr, *px = nullptr, *pq = nullptr;
    const uint8_t* dbase = nullptr;
    if (dev_rows) {
        VK_TRY(d_coeff.ensure(2 * B * N * 32));
        ones.assign(B * N, fe_one<F>());
        VK_CHECK_HIP(hipMemcpyAsync(d_coeff.p, ones.data(), B * N * 32, hipMemcpyHostToDevice, ctx->stream));
        VK_TRY(ctx->pin_ipa.ensure((B * N + 3 * B) * 32));
        pa = ctx->pin_ipa.as<Fr>();
        px = pa + B * N;
        pq = px + B;
        dbase = static_cast<const uint8_t*>(ctx->pin_ipa.dp);
    }
    std::vector<Fr> sc(dev_rows ? 0 : 2 * B * W);
    std::vector<uint64_t> oxy(2 * B * 8);
    std::vector<uint8_t> oinf(2 * B);
    double lap_fill = 0, lap_commit = 0, lap_fold = 0;
    for (size_t r = 0; r < K; r++) {
        const size_t m = N >> r, half = m / 2;
        const double c0 = host_timing() ? clock_us() : 0.0;
        double c1 = 0.0;
        if (dev_rows) {
            par_for([&](size_t p) {
                IpaState& s = st[p];
                memcpy(pa + p * N, s.a.data(), m * 32);
                ipar::q_terms(s.a.data(), s.b.data(), s.w, half, &pq[2 * p], &pq[2 * p + 1]);
            });
            IpaRows ir;
            ir.a = reinterpret_cast<const uint32_t*>(dbase);
            ir.x = reinterpret_cast<const uint32_t*>(dbase + (size_t)B * N * 32);
            ir.q = reinterpret_cast<const uint32_t*>(dbase + (size_t)(B * N + B) * 32);
            ir.coeff_in = reinterpret_cast<const uint32_t*>(d_coeff.as<uint8_t>() + (r & 1) * B * N * 32);
            ir.coeff_out = reinterpret_cast<uint32_t*>(d_coeff.as<uint8_t>() + ((r + 1) & 1) * B * N * 32);
            ir.N = (uint32_t)N;
            ir.m = (uint32_t)m;
            ir.h = (uint32_t)half;
            ir.fold = r > 0 ? 1u : 0u;
            ir.m_prev = (uint32_t)(2 * m);
            ir.h_prev = (uint32_t)m;
            c1 = host_timing() ? clock_us() : 0.0;
            VK_TRY(ctx->ws[WS_MISC].ensure(2 * B * 65));
            uint8_t* dxy = ctx->ws[WS_MISC].as<uint8_t>();
            bool on_host = false;
            VK_TRY(msm_batch_run(ctx, t, N + 1, nullptr, 2 * B, 1, dxy, dxy + 2 * B * 64, oxy.data(), oinf.data(),
                                 &on_host, nullptr, nullptr, &ir));
            if (!on_host) {  // (the latency path returns host results: not expected)
                VK_CHECK_HIP(hipMemcpyAsync(oxy.data(), dxy, 2 * B * 64, hipMemcpyDeviceToHost, ctx->stream));
                VK_CHECK_HIP(hipMemcpyAsync(oinf.data(), dxy + 2 * B * 64, 2 * B, hipMemcpyDeviceToHost, ctx->stream));
                VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
            }
        } else {
            // L (even commits): bases i with i mod m >= half, R (odd): i mod m < half, then q
            par_for([&](size_t p) {
                IpaState& s = st[p];
                ipar::round_rows(s.a.data(), r == 0 ? nullptr : s.coeff.data(), N, m, half, &sc[(2 * p) * W],
                                 &sc[(2 * p + 1) * W], s.b.data(), &s.w);
            });
            c1 = host_timing() ? clock_us() : 0.0;
            VK_TRY(commit_batch(ctx, t, W, sc.data(), 2 * B, oxy.data(), oinf.data()));
        }
        const double c2 = host_timing() ? clock_us() : 0.0;
        // (device rows: the coefficients stay there, the next round's kernel folds them by px[p])
        par_for([&](size_t p) {
            IpaState& s = st[p];
            const Fr x = close_round(r, p, oxy.data(), oinf.data(), proofs, s.tr, N, s.a, &s.b,
                                     dev_rows ? nullptr : s.coeff.data());
            if (dev_rows) px[p] = x;
        });
        if (host_timing()) {
            const double c3 = clock_us();
            lap_fill += c1 - c0, lap_commit += c2 - c1, lap_fold += c3 - c2;
        }
    }
    if (host_timing())
        fprintf(stderr, "[ipa_prove] %zu proofs x %zu rounds: rows %.1f us, L/R commits %.1f us, transcript + folds %.1f us\n",
                B, K, lap_fill, lap_commit, lap_fold);
    for (size_t p = 0; p < B; p++) {
        proofs[p].rounds = K;
        canon_of(st[p].a[0], proofs[p].tip);
        canon_of(st[p].eval, proofs[p].y);
        if (st[p].own) vc_transcript_free(st[p].tr);
    }
    return VC_OK;
}

// ---------------------------------------------------------------- IPA verify (a10)
int ipa_verify_impl(vc_ctx* ctx, Table* t, size_t N, const Acc& com, const Fr& point, const vc_ipa_proof* pr,
                    vc_transcript* tr_in, int* result) {
    if (!is_pow2(N) || t->n < N + 1) return VC_E_INVALID;
    size_t K = pr->rounds;
    if ((1ull << K) != N) return VC_E_INVALID;  // gens = g[0..2^rounds], zip with points_coeffs
    const double t0 = host_timing() ? clock_us() : 0.0;
    Fr omega = bn254_group_gen(N);
    if (barycentric_panics(N, point)) return VC_E_DOMAIN;
    std::vector<Fr> b = barycentric(N, point, omega);
    bool own = tr_in == nullptr;
    vc_transcript* tr = own ? vc_transcript_new("ipa") : tr_in;
    uint64_t cxy[8];
    uint8_t cinf;
    aff_of(com, cxy, &cinf);
    Fr y = fr_of(pr->y), tip = fr_of(pr->tip);
    transcript_append_point(tr, cxy, cinf, "C");
    transcript_append_fr(tr, point, "input point");
    transcript_append_fr(tr, y, "output point");
    Fr w = transcript_digest(tr, "w");
    const std::vector<Fr> xs = read_challenges(tr, pr);
    if (own) vc_transcript_free(tr);
    std::vector<Fr> s, vs;  // points_coeffs; the scalars of C, L_k, R_k
    const Fr prodx = ipar::verifier_scalars(xs.data(), K, s, vs);
    Fr cb = inner(b.data(), s.data(), N);
    // fixed part over (g, q): -tip*s_i, (prodx*w*y - w*tip*<b,s>)
    std::vector<Fr> fs(N + 1);
    for (size_t i = 0; i < N; i++) fs[i] = fe_neg<F>(fe_mul<F>(tip, s[i]));
    fs[N] = fe_sub<F>(fe_mul<F>(fe_mul<F>(prodx, w), y), fe_mul<F>(fe_mul<F>(w, tip), cb));
    // the fixed part on the GPU, the variable part's Straus (<= HOST_MSM_MAX points: host pool)
    // while its kernel runs
    uint64_t axy[8];
    uint8_t ainf;
    Acc vb;
    int vst = VC_OK;
    double t_straus = 0.0;
    bool ran = false;
    const bool on_host = vs.size() <= HOST_MSM_MAX;
    const std::function<void()> straus = [&] {
        ran = true;
        const double s0 = host_timing() ? clock_us() : 0.0;
        vst = var_part(ctx, cxy, cinf, pr, vs, &vb);
        if (host_timing()) t_straus = clock_us() - s0;
    };
    const double t1 = host_timing() ? clock_us() : 0.0;
    VK_TRY(commit_batch(ctx, t, N + 1, fs.data(), 1, axy, &ainf, on_host ? &straus : nullptr));
    if (!ran) straus();
    VK_TRY(vst);
    if (host_timing())
        fprintf(stderr, "ipa_verify host_prep_us=%.1f commit_and_straus_us=%.1f (straus %.1f)\n", t1 - t0,
                clock_us() - t1, t_straus);
    Acc tot = C::add(acc_of(axy, ainf), vb);
    *result = C::is_zero(tot) ? 1 : 0;
    return VC_OK;
}

}  // namespace vk

using namespace vk;

extern "C" {

int vc_ipa_commit(vc_ctx* ctx, int table, size_t N, const uint64_t* data, size_t batch, uint64_t* out_xy,
                  uint8_t* out_inf) {
    return vc_msm_batch(ctx, table, N, data, batch, 0, out_xy, out_inf);
}

int vc_ipa_prove(vc_ctx* ctx, int table, size_t N, const uint64_t* data, const uint64_t* com_xy,
                 const uint8_t* com_inf, const uint64_t* points, size_t batch, vc_transcript** trs,
                 vc_ipa_proof* proofs) {
    if (!ctx || !data || !com_xy || !com_inf || !points || !proofs || ctx->curve != VC_CURVE_BN254)
        return VC_E_INVALID;
    for (size_t p = 0; p < batch; p++)
        if (!proof_ok(&proofs[p])) return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    std::vector<std::vector<Fr>> d(batch, std::vector<Fr>(N));
    std::vector<Acc> coms(batch);
    std::vector<Fr> pts(batch);
    for (size_t p = 0; p < batch; p++) {
        for (size_t i = 0; i < N; i++) d[p][i] = fr_of(data + (p * N + i) * 4);
        coms[p] = acc_of(com_xy + 8 * p, com_inf[p]);
        pts[p] = fr_of(points + 4 * p);
    }
    return ipa_prove_impl(ctx, t, N, d, coms, pts, trs, proofs);
}

int vc_ipa_verify(vc_ctx* ctx, int table, size_t N, const uint64_t* com_xy, uint8_t com_inf, const uint64_t* point,
                  const vc_ipa_proof* proof, vc_transcript* tr, int* result) {
    if (!ctx || !point || !proof_ok(proof) || !result || (!com_xy && !com_inf) || ctx->curve != VC_CURVE_BN254)
        return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    uint64_t zero[8] = {0};
    return ipa_verify_impl(ctx, t, N, acc_of(com_inf ? zero : com_xy, com_inf), fr_of(point), proof, tr, result);
}

// ---------------------------------------------------------------- IPA commitment proof
// prove_commitment (ipa/mod.rs:199-234): the IPA rounds with neither the evaluation vector b
// nor q. Same representation as ipa_prove_impl -- the folded generators are coefficients over
// the first n CRS points -- so each round is one batch of 2B width-n fixed-base commits.
int vc_ipa_prove_commitment(vc_ctx* ctx, int table, size_t n, const uint64_t* data, const uint64_t* com_xy,
                            const uint8_t* com_inf, size_t batch, vc_ipa_proof* proofs) {
    if (!ctx || !data || !com_xy || !com_inf || !proofs || ctx->curve != VC_CURVE_BN254) return VC_E_INVALID;
    // n = data.max() + 1; the assert in vec_add_and_distribute (utils.rs:37) fires on any
    // odd split above 1, i.e. unless n is a power of two
    if (!is_pow2(n)) return VC_E_INVALID;
    size_t K = 0;
    while ((1ull << K) < n) K++;
    for (size_t p = 0; p < batch; p++)
        if (!proof_ok(&proofs[p]) || proofs[p].rounds < K) return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    if (t->n < n) return VC_E_INVALID;  // key.g[0..max + 1] out of bounds
    std::vector<std::vector<Fr>> a(batch, std::vector<Fr>(n));
    std::vector<std::vector<Fr>> coeff(batch, std::vector<Fr>(n, fe_one<F>()));
    std::vector<vc_transcript*> trs(batch);
    for (size_t p = 0; p < batch; p++) {
        for (size_t i = 0; i < n; i++) a[p][i] = fr_of(data + (p * n + i) * 4);
        trs[p] = vc_transcript_new("ipa");
        transcript_append_point(trs[p], com_xy + 8 * p, com_inf[p], "C");
        (void)transcript_digest(trs[p], "x");
    }
    std::vector<Fr> sc(2 * batch * n);
    std::vector<uint64_t> oxy(2 * batch * 8);
    std::vector<uint8_t> oinf(2 * batch);
    int st = VC_OK;
    for (size_t r = 0; r < K && st == VC_OK; r++) {
        const size_t m = n >> r, half = m / 2;
        // L = <gens_R, data_L>, R = <gens_L, data_R>
        for (size_t p = 0; p < batch; p++)
            ipar::round_rows(a[p].data(), r == 0 ? nullptr : coeff[p].data(), n, m, half, &sc[(2 * p) * n],
                             &sc[(2 * p + 1) * n]);
        st = commit_batch(ctx, t, n, sc.data(), 2 * batch, oxy.data(), oinf.data());
        if (st != VC_OK) break;
        // data <- data_L + x data_R ; gens <- gens_R + x gens_L (coefficients)
        for (size_t p = 0; p < batch; p++)
            close_round(r, p, oxy.data(), oinf.data(), proofs, trs[p], n, a[p], nullptr, coeff[p].data());
    }
    for (size_t p = 0; p < batch; p++) {
        if (st == VC_OK) {
            proofs[p].rounds = K;
            canon_of(a[p][0], proofs[p].tip);
            memset(proofs[p].y, 0, sizeof(proofs[p].y));
        }
        vc_transcript_free(trs[p]);
    }
    return st;
}

// verify_commitment_proof (ipa/mod.rs:237-265): c_K = L_K + x_K c_{K-1} + x_K^2 R_K unrolled to
// (prod x) C + sum_k P_k (L_k + x_k^2 R_k), P_k = prod_{j>k} x_j (one small variable-base MSM),
// checked against tip * <g[0..2^K], points_coeffs> (one fixed-base commit): their difference
// must be the identity.
int vc_ipa_verify_commitment_proof(vc_ctx* ctx, int table, const uint64_t* com_xy, uint8_t com_inf,
                                   const vc_ipa_proof* pr, int* result) {
    if (!ctx || !proof_ok(pr) || !result || (!com_xy && !com_inf) || ctx->curve != VC_CURVE_BN254)
        return VC_E_INVALID;
    const size_t K = pr->rounds;
    if (K >= 40) return VC_E_INVALID;
    const size_t n = 1ull << K;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    if (t->n < n) return VC_E_INVALID;  // key.g[0..2^rounds] out of bounds
    uint64_t zero[8] = {0};
    const uint64_t* cxy = com_inf ? zero : com_xy;
    vc_transcript* tr = vc_transcript_new("ipa");
    transcript_append_point(tr, cxy, com_inf, "C");
    (void)transcript_digest(tr, "x");
    const std::vector<Fr> xs = read_challenges(tr, pr);
    vc_transcript_free(tr);
    std::vector<Fr> s, vs;
    ipar::verifier_scalars(xs.data(), K, s, vs);
    Fr tip = fr_of(pr->tip);
    std::vector<Fr> fs(n);
    for (size_t i = 0; i < n; i++) fs[i] = fe_neg<F>(fe_mul<F>(tip, s[i]));
    uint64_t axy[8];
    uint8_t ainf;
    VK_TRY(commit_batch(ctx, t, n, fs.data(), 1, axy, &ainf));
    Acc vb;
    VK_TRY(var_part(ctx, cxy, com_inf, pr, vs, &vb));
    Acc tot = C::add(acc_of(axy, ainf), vb);
    *result = C::is_zero(tot) ? 1 : 0;
    return VC_OK;
}

}  // extern "C"

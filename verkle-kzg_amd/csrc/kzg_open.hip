// KZG openings (reference: vector-commit/src/kzg/mod.rs): one point, all points (FK), the
// range-sharded open and the SRS set-up.
#include "kzg_point.hpp"
#include "poly.hpp"
#include "protocol.hpp"

namespace vk {

static int lg2_of(size_t n) {
    int lg = 0;
    while (((size_t)1 << lg) < n) lg++;
    return lg;
}

// The status a single open takes from its point alone (kzg_point.hpp: the rules of the batch,
// vc_kzg_prove_many), decided on the host before any GPU work so that a failing call writes no
// output: VC_E_INVALID for a point >= r, VC_E_DOMAIN for point == size and for a domain element
// that is not below size (z^size == 1, r - 1 among them). size: a power of two below 2^31.
template <class Fr_>
static int open_point_status(size_t size, const uint64_t* point) {
    uint32_t cls = 0;
    return kzgm::point_status<Fr_>(reinterpret_cast<const uint32_t*>(point), (uint32_t)size, lg2_of(size), &cls);
}

// ---------------------------------------------------------------- KZG (a3/a4/a5/a6/a7)
// evals: host (d_evals == false) or device canonical scalars; out_acc != nullptr returns the
// un-normalised proof accumulator of window slice `part` of `parts` (multi-GPU) instead of
// the affine proof
template <class C_, class Fr_>
static int kzg_prove_t(vc_ctx* ctx, Table* t, size_t size, const uint64_t* evals, size_t max, const uint64_t* point,
                       uint64_t* proof_xy, uint8_t* proof_inf, uint64_t* y_out, uint64_t* q_out, bool d_evals = false,
                       int part = 0, int parts = 1, uint32_t* out_acc = nullptr, uint64_t* com_xy = nullptr,
                       uint8_t* com_inf = nullptr) {
    if (!is_pow2(size) || (size >> 31) || max > size) return VC_E_INVALID;
    if (t && t->n < size) return VC_E_RANGE;
    VK_TRY(open_point_status<Fr_>(size, point));
    DevBuf d_f(ctx), d_q(ctx), pw(ctx), tmp(ctx), part_buf(ctx);
    VK_TRY(d_f.ensure(size * 32));
    VK_TRY(d_q.ensure(size * 32));
    VK_TRY(tmp.ensure(size * 32));
    const void* ev_dev = tmp.p;
    if (d_evals) ev_dev = evals;
    else if (max > 0) VK_CHECK_HIP(hipMemcpyAsync(tmp.p, evals, max * 32, hipMemcpyHostToDevice, ctx->stream));
    VK_TRY(canon_to_mont_dev<Fr_>(ctx, ev_dev, size, max, d_f.as<fe<Fr_>>()));
    fe<Fr_> pm = canon_to_mont<Fr_>(point);
    fe<Fr_> omega = group_gen_t<Fr_>(size, fr_generator<Fr_>());
    // y arrives in page-locked memory once the stream has passed the quotient (read after a sync)
    VK_TRY(ctx->pin_y.ensure(sizeof(fe<Fr_>)));
    fe<Fr_>* yp = ctx->pin_y.as<fe<Fr_>>();
    VK_TRY(kzg_quotient_dev<Fr_>(ctx, size, d_f.as<fe<Fr_>>(), max, pm, omega, d_q.as<fe<Fr_>>(), yp, pw, tmp,
                                 part_buf));
    struct YOut {  // every return path below has synchronised the stream (or fails)
        vc_ctx* c;
        const fe<Fr_>* yp;
        uint64_t* out;
        ~YOut() {
            if (hipStreamSynchronize(c->stream) == hipSuccess) mont_to_canon<Fr_>(*yp, out);
        }
    } y_fin{ctx, yp, y_out};
    if (q_out) {
        VK_TRY(mont_to_canon_dev<Fr_>(ctx, d_q.as<fe<Fr_>>(), size, tmp.p));
        VK_CHECK_HIP(hipMemcpyAsync(q_out, tmp.p, size * 32, hipMemcpyDeviceToHost, ctx->stream));
        VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (t && com_xy) {  // commitment + proof: the two MSMs over the SRS as one batched pipeline
        const void* sc[2] = {d_f.p, d_q.p};
        const int mt[2] = {1, 1};
        const int words = point_words(ctx->curve);
        std::vector<uint32_t> acc(2 * (size_t)words);
        VK_TRY(msm_run_many(ctx, t, sc, mt, size, 2, acc.data()));
        VK_TRY(acc_to_affine(ctx->curve, acc.data(), com_xy, com_inf));
        VK_TRY(acc_to_affine(ctx->curve, acc.data() + words, proof_xy, proof_inf));
    } else if (t && out_acc) {
        VK_TRY(msm_run(ctx, t, 0, d_q.p, size, 1, out_acc, part, parts));
    } else if (t && t->fb_c != 0 && size <= 1024) {
        // a small proof MSM over a table that has fixed-base window tables (vc_fixed_base_precompute):
        // the batched commit's latency path -- one launch, the block partials added on the host --
        // instead of a Pippenger pipeline of ~12 latency-bound launches (benches/kzg.rs: 32 terms)
        const size_t xyb = (size_t)C_::F::N * 8;  // canonical affine x, y
        VK_TRY(ctx->ws[WS_MISC].ensure(xyb + 1));
        uint8_t* dxy = ctx->ws[WS_MISC].as<uint8_t>();
        bool on_host = false;
        VK_TRY(msm_batch_run(ctx, t, size, d_q.p, 1, 1, dxy, dxy + xyb, proof_xy, proof_inf, &on_host));
        if (!on_host) {
            VK_CHECK_HIP(hipMemcpyAsync(proof_xy, dxy, xyb, hipMemcpyDeviceToHost, ctx->stream));
            VK_CHECK_HIP(hipMemcpyAsync(proof_inf, dxy + xyb, 1, hipMemcpyDeviceToHost, ctx->stream));
            VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        }
    } else if (t) {
        std::vector<uint32_t> acc(point_words(ctx->curve));
        VK_TRY(msm_run(ctx, t, 0, d_q.p, size, 1, acc.data()));
        VK_TRY(acc_to_affine(ctx->curve, acc.data(), proof_xy, proof_inf));
    }
    return VC_OK;
}

// ---------------------------------------------------------------- FK all-point openings (f4)
// KZG::prove_all_points (kzg/mod.rs:200-235): radix-2 FFTs over G1 (a butterfly multiplies a
// point by a twiddle: one double-and-add scalar multiplication) and over Fr, natural-order in and
// out (bit reversal, then iterative Cooley-Tukey), as ark-poly's Radix2EvaluationDomain computes
// them (fft: y_i = sum_j a_j w^(ij); ifft: a_j = n^-1 sum_i y_i w^(-ij)). Dead code in the
// reference (no caller; its test at :299 has no #[test]); see DESIGN.md for both modes.
template <class C, class Fr_>
__device__ typename C::Acc pt_mul_fe(const typename C::Acc& p, const fe<Fr_>& k_mont) {
    const fe<Fr_> k = fe_from_mont<Fr_>(k_mont);
    typename C::Acc r = C::zero();
    bool started = false;
    for (int i = Fr_::N * 32 - 1; i >= 0; i--) {
        const bool bit = (k.v[i >> 5] >> (i & 31)) & 1u;
        if (started) r = C::dbl(r);
        if (bit) {
            r = started ? C::add(r, p) : p;
            started = true;
        }
    }
    return r;
}
__device__ __forceinline__ uint32_t bitrev32(uint32_t i, int lg) { return lg ? (__brev(i) >> (32 - lg)) : 0u; }

template <class T>
__global__ void k_bitrev(const T* __restrict__ in, T* __restrict__ out, uint32_t n, int lg) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[bitrev32(i, lg)] = in[i];
}
// one stage (blocks of 2 half): a[i0], a[i1] <- u + w v, u - w v with w = tw[j * step]
template <class C, class Fr_>
__global__ void k_pt_stage(typename C::Acc* __restrict__ a, uint32_t n, uint32_t half, const fe<Fr_>* __restrict__ tw,
                           uint32_t step) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n / 2) return;
    const uint32_t blk = g / half, j = g % half;
    const uint32_t i0 = blk * 2 * half + j, i1 = i0 + half;
    const typename C::Acc u = a[i0];
    const typename C::Acc v = j == 0 ? a[i1] : pt_mul_fe<C, Fr_>(a[i1], tw[j * step]);
    a[i0] = C::add(u, v);
    a[i1] = C::add(u, C::neg(v));
}
template <class Fr_>
__global__ void k_fr_stage(fe<Fr_>* __restrict__ a, uint32_t n, uint32_t half, const fe<Fr_>* __restrict__ tw,
                           uint32_t step) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n / 2) return;
    const uint32_t blk = g / half, j = g % half;
    const uint32_t i0 = blk * 2 * half + j, i1 = i0 + half;
    const fe<Fr_> u = a[i0], v = fe_mul<Fr_>(a[i1], tw[j * step]);
    a[i0] = fe_add<Fr_>(u, v);
    a[i1] = fe_sub<Fr_>(u, v);
}
// a[i] <- a[i] * (s ? s[i] : k)
template <class C, class Fr_>
__global__ void k_pt_scale(typename C::Acc* __restrict__ a, uint32_t n, const fe<Fr_>* __restrict__ s, fe<Fr_> k) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = pt_mul_fe<C, Fr_>(a[i], s ? s[i] : k);
}
template <class Fr_>
__global__ void k_fr_scale(fe<Fr_>* __restrict__ a, uint32_t n, fe<Fr_> k) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = fe_mul<Fr_>(a[i], k);
}
template <class C>
__global__ void k_aff_to_acc(const typename C::Aff* __restrict__ in, const uint8_t* __restrict__ inf, uint32_t n,
                             typename C::Acc* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = inf[i] ? C::zero() : C::from_aff(in[i], false);
}
// out[i] = src[map(i)] or the identity: reversed prefix (mode 0's s_hat) / reversed shifted
// prefix (mode 1's S') / a window (mode 1's h)
template <class C>
__global__ void k_pt_gather(const typename C::Acc* __restrict__ src, uint32_t n, int64_t base, int64_t dir,
                            uint32_t valid, typename C::Acc* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i < valid ? src[base + dir * (int64_t)i] : C::zero();
}

// in-place FFT (inverse: iFFT incl. the 1/n) of n = 2^k points / field elements in a DevBuf
template <class C, class Fr_>
static int pt_fft(vc_ctx* ctx, DevBuf& a, size_t n, bool inverse) {
    using Acc = typename C::Acc;
    if (n <= 1) return VC_OK;
    const int lg = lg2_of(n);
    const fe<Fr_> w = group_gen_t<Fr_>(n, fr_generator<Fr_>());
    DevBuf tw(ctx), tmp(ctx);
    VK_TRY(tw.ensure(n / 2 * sizeof(fe<Fr_>)));
    VK_TRY(tmp.ensure(n * sizeof(Acc)));
    VK_TRY(domain_powers<Fr_>(ctx, inverse ? fe_inv_bin<Fr_>(w) : w, n / 2, tw.as<fe<Fr_>>()));
    const unsigned g = (unsigned)((n + 255) / 256), g2 = (unsigned)((n / 2 + 255) / 256);
    VK_LAUNCH(ctx, "fk_bitrev", (k_bitrev<Acc>), g, 256, 0, a.as<Acc>(), tmp.as<Acc>(), (uint32_t)n, lg);
    for (uint32_t half = 1; half < n; half <<= 1)
        VK_LAUNCH(ctx, "fk_pt_stage", (k_pt_stage<C, Fr_>), g2, 256, 0, tmp.as<Acc>(), (uint32_t)n, half,
                  tw.as<fe<Fr_>>(), (uint32_t)(n / (2 * half)));
    if (inverse)
        VK_LAUNCH(ctx, "fk_pt_scale", (k_pt_scale<C, Fr_>), g, 256, 0, tmp.as<Acc>(), (uint32_t)n,
                  (const fe<Fr_>*)nullptr, fe_inv_bin<Fr_>(mont_from_u64<Fr_>(n)));
    VK_CHECK_HIP(hipMemcpyAsync(a.p, tmp.p, n * sizeof(Acc), hipMemcpyDeviceToDevice, ctx->stream));
    VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));  // tw / tmp go back to the pool
    return VC_OK;
}
template <class Fr_>
static int fr_fft(vc_ctx* ctx, DevBuf& a, size_t n, bool inverse) {
    if (n <= 1) return VC_OK;
    const int lg = lg2_of(n);
    const fe<Fr_> w = group_gen_t<Fr_>(n, fr_generator<Fr_>());
    DevBuf tw(ctx), tmp(ctx);
    VK_TRY(tw.ensure(n / 2 * sizeof(fe<Fr_>)));
    VK_TRY(tmp.ensure(n * sizeof(fe<Fr_>)));
    VK_TRY(domain_powers<Fr_>(ctx, inverse ? fe_inv_bin<Fr_>(w) : w, n / 2, tw.as<fe<Fr_>>()));
    const unsigned g = (unsigned)((n + 255) / 256), g2 = (unsigned)((n / 2 + 255) / 256);
    VK_LAUNCH(ctx, "fk_bitrev", (k_bitrev<fe<Fr_>>), g, 256, 0, a.as<fe<Fr_>>(), tmp.as<fe<Fr_>>(), (uint32_t)n, lg);
    for (uint32_t half = 1; half < n; half <<= 1)
        VK_LAUNCH(ctx, "fk_fr_stage", (k_fr_stage<Fr_>), g2, 256, 0, tmp.as<fe<Fr_>>(), (uint32_t)n, half,
                  tw.as<fe<Fr_>>(), (uint32_t)(n / (2 * half)));
    if (inverse)
        VK_LAUNCH(ctx, "fk_fr_scale", (k_fr_scale<Fr_>), g, 256, 0, tmp.as<fe<Fr_>>(), (uint32_t)n,
                  fe_inv_bin<Fr_>(mont_from_u64<Fr_>(n)));
    VK_CHECK_HIP(hipMemcpyAsync(a.p, tmp.p, n * sizeof(fe<Fr_>), hipMemcpyDeviceToDevice, ctx->stream));
    VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return VC_OK;
}

// mode 0: the reference's prove_all_points exactly; mode 1: the FK proofs it was meant to return
template <class C, class Fr_>
static int fk_all_t(vc_ctx* ctx, Table* t, size_t size, const uint64_t* evals, size_t ne, int mode,
                    uint64_t* out_xy, uint8_t* out_inf, uint64_t* out_y, size_t* count) {
    using Acc = typename C::Acc;
    if (!is_pow2(size) || t->n < size) return VC_E_INVALID;
    if (ne == 0) return VC_E_DOMAIN;  // the reference: coeffs[degree] of the zero polynomial panics
    const int NL = aff_limbs64(ctx->curve);
    // the Lagrange SRS as projective points
    DevBuf L(ctx);
    VK_TRY(L.ensure(size * sizeof(Acc)));
    VK_LAUNCH(ctx, "fk_aff_to_acc", (k_aff_to_acc<C>), (size + 255) / 256, 256, 0, t->bases.as<typename C::Aff>(),
              t->inf.as<uint8_t>(), (uint32_t)size, L.as<Acc>());
    auto upload_evals = [&](DevBuf& dst, size_t n) -> int {  // evals padded with zeros to n, Montgomery
        DevBuf raw(ctx);
        VK_TRY(dst.ensure(n * sizeof(fe<Fr_>)));
        VK_TRY(raw.ensure(n * 32));
        const size_t m = std::min(ne, n);
        VK_CHECK_HIP(hipMemcpyAsync(raw.p, evals, m * 32, hipMemcpyHostToDevice, ctx->stream));
        VK_TRY(canon_to_mont_dev<Fr_>(ctx, raw.p, n, m, dst.as<fe<Fr_>>()));
        VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        return VC_OK;
    };
    DevBuf out(ctx);  // the D output points
    size_t D = 0;
    if (mode == 0) {
        // data.interpolate() over the data's own domain (LagrangeBasis::from_vec: next_pow2(len))
        size_t m = 1;
        while (m < ne) m <<= 1;
        DevBuf cf(ctx);
        VK_TRY(upload_evals(cf, m));
        VK_TRY(fr_fft<Fr_>(ctx, cf, m, true));
        std::vector<fe<Fr_>> coeffs(m);
        VK_CHECK_HIP(hipMemcpy(coeffs.data(), cf.p, m * sizeof(fe<Fr_>), hipMemcpyDeviceToHost));
        size_t deg = m;
        while (deg > 0 && fe_is_zero<Fr_>(coeffs[deg - 1])) deg--;
        if (deg == 0) return VC_E_DOMAIN;  // zero polynomial: coeffs[degree] out of bounds
        const size_t d = deg - 1;          // poly.degree()
        D = 1;
        while (D < 2 * d) D <<= 1;  // D::new(degree * 2)
        if (D > ne || d > size) return VC_E_DOMAIN;  // data[i] / g1[0..degree] out of bounds
        // c_hat = [c_d, 0^(d+1), c_0 .. c_{d-1}], resized to the domain by fft_in_place
        std::vector<fe<Fr_>> chat(D, fe_zero<Fr_>());
        std::vector<fe<Fr_>> full;
        full.push_back(coeffs[d]);
        full.insert(full.end(), d + 1, fe_zero<Fr_>());
        full.insert(full.end(), coeffs.begin(), coeffs.begin() + d);
        for (size_t i = 0; i < D && i < full.size(); i++) chat[i] = full[i];
        DevBuf yv(ctx);
        VK_TRY(yv.ensure(D * sizeof(fe<Fr_>)));
        VK_CHECK_HIP(hipMemcpy(yv.p, chat.data(), D * sizeof(fe<Fr_>), hipMemcpyHostToDevice));
        VK_TRY(fr_fft<Fr_>(ctx, yv, D, false));
        // g1 = ifft(lagrange_commitments) over the key's domain; s_hat = reverse(g1[0..d]) || O
        VK_TRY((pt_fft<C, Fr_>(ctx, L, size, true)));
        VK_TRY(out.ensure(D * sizeof(Acc)));
        VK_LAUNCH(ctx, "fk_gather", (k_pt_gather<C>), (D + 255) / 256, 256, 0, L.as<Acc>(), (uint32_t)D,
                  (int64_t)d - 1, (int64_t)-1, (uint32_t)d, out.as<Acc>());
        VK_TRY((pt_fft<C, Fr_>(ctx, out, D, false)));  // v
        VK_LAUNCH(ctx, "fk_pt_scale", (k_pt_scale<C, Fr_>), (D + 255) / 256, 256, 0, out.as<Acc>(), (uint32_t)D,
                  yv.as<fe<Fr_>>(), fe_zero<Fr_>());  // u = v .* y
        VK_TRY((pt_fft<C, Fr_>(ctx, out, D, true)));    // h_hat
    } else if (mode == 1) {
        const size_t n = size;
        D = n;
        if (ne > n) return VC_E_RANGE;
        DevBuf c2(ctx);
        VK_TRY(upload_evals(c2, 2 * n));  // zero-padded to 2n; the first n entries are the data
        // coefficients: iFFT over the key domain of the first n entries (the rest stays zero)
        {
            DevBuf cn(ctx);
            VK_TRY(cn.ensure(n * sizeof(fe<Fr_>)));
            VK_CHECK_HIP(hipMemcpyAsync(cn.p, c2.p, n * sizeof(fe<Fr_>), hipMemcpyDeviceToDevice, ctx->stream));
            VK_TRY(fr_fft<Fr_>(ctx, cn, n, true));
            VK_CHECK_HIP(hipMemcpyAsync(c2.p, cn.p, n * sizeof(fe<Fr_>), hipMemcpyDeviceToDevice, ctx->stream));
        }
        VK_TRY(fr_fft<Fr_>(ctx, c2, 2 * n, false));
        // monomial SRS S = fft(L) (setup made L = ifft(S)); S'[i] = S[n - 2 - i] for i <= n - 2
        VK_TRY((pt_fft<C, Fr_>(ctx, L, n, false)));
        DevBuf V(ctx);
        VK_TRY(V.ensure(2 * n * sizeof(Acc)));
        VK_LAUNCH(ctx, "fk_gather", (k_pt_gather<C>), (2 * n + 255) / 256, 256, 0, L.as<Acc>(), (uint32_t)(2 * n),
                  (int64_t)n - 2, (int64_t)-1, (uint32_t)(n - 1), V.as<Acc>());
        VK_TRY((pt_fft<C, Fr_>(ctx, V, 2 * n, false)));
        VK_LAUNCH(ctx, "fk_pt_scale", (k_pt_scale<C, Fr_>), (2 * n + 255) / 256, 256, 0, V.as<Acc>(),
                  (uint32_t)(2 * n), c2.as<fe<Fr_>>(), fe_zero<Fr_>());
        VK_TRY((pt_fft<C, Fr_>(ctx, V, 2 * n, true)));  // the Toeplitz product, h_j at j + n - 1
        VK_TRY(out.ensure(n * sizeof(Acc)));
        VK_LAUNCH(ctx, "fk_gather", (k_pt_gather<C>), (n + 255) / 256, 256, 0, V.as<Acc>(), (uint32_t)n,
                  (int64_t)n - 1, (int64_t)1, (uint32_t)n, out.as<Acc>());
        VK_TRY((pt_fft<C, Fr_>(ctx, out, n, false)));  // proofs at w^i
    } else {
        return VC_E_INVALID;
    }
    DevBuf dxy(ctx), dinf(ctx);
    VK_TRY(dxy.ensure(D * 2 * NL * 8));
    VK_TRY(dinf.ensure(D));
    VK_TRY(normalize_to_canon(ctx, ctx->curve, out.p, D, dxy.p, dinf.as<uint8_t>()));
    VK_CHECK_HIP(hipMemcpy(out_xy, dxy.p, D * 2 * NL * 8, hipMemcpyDeviceToHost));
    VK_CHECK_HIP(hipMemcpy(out_inf, dinf.p, D, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < D; i++)
        for (int k = 0; k < 4; k++) out_y[4 * i + k] = i < ne ? evals[4 * i + k] : 0;
    *count = D;
    return VC_OK;
}

// kzg_prove_t of the context's curve (the arguments after q_out as kzg_prove_t's)
template <class... Rest>
static int kzg_prove_any(vc_ctx* ctx, Table* t, size_t size, const uint64_t* evals, size_t max, const uint64_t* point,
                         uint64_t* proof_xy, uint8_t* proof_inf, uint64_t* y, uint64_t* q_out, Rest... rest) {
    if (ctx->curve == VC_CURVE_BN254)
        return kzg_prove_t<BN254G1, BN254Fr>(ctx, t, size, evals, max, point, proof_xy, proof_inf, y, q_out, rest...);
    if (ctx->curve == VC_CURVE_BLS12_381)
        return kzg_prove_t<BLS381G1, BLS381Fr>(ctx, t, size, evals, max, point, proof_xy, proof_inf, y, q_out, rest...);
    return VC_E_INVALID;
}

// the Lagrange SRS l_j(s) G of n points as accumulators: G = (gx, gy), the domain from `root`
template <class C_, class Fr_>
static int kzg_srs_acc(vc_ctx* ctx, size_t max_items, size_t n, const uint64_t* secret, uint32_t root, const uint64_t* gx,
                       const uint64_t* gy, DevBuf& acc) {
    VK_TRY(acc.ensure(n * sizeof(typename C_::Acc)));
    typename C_::Aff gen;
    gen.x = canon_to_mont<typename C_::F>(gx);
    gen.y = canon_to_mont<typename C_::F>(gy);
    return kzg_srs_dev<C_, Fr_>(ctx, max_items, n, canon_to_mont<Fr_>(secret), group_gen_t<Fr_>(n, root), gen,
                                acc.as<typename C_::Acc>());
}

// the multiproof's inner KZG proof (multiproof.hip): host evaluations, the whole domain
int kzg_open_bn254(vc_ctx* ctx, Table* t, size_t size, const uint64_t* evals, const uint64_t* point,
                   uint64_t* proof_xy, uint8_t* proof_inf, uint64_t* y) {
    return kzg_prove_t<BN254G1, BN254Fr>(ctx, t, size, evals, size, point, proof_xy, proof_inf, y, nullptr);
}

}  // namespace vk

using namespace vk;

extern "C" {

int vc_kzg_setup(vc_ctx* ctx, size_t max_items, const uint64_t* secret, int* table_id, size_t* size) {
    if (!ctx || !secret || !table_id || max_items == 0) return VC_E_INVALID;
    Guard g(ctx);
    size_t n = 1;
    while (n < max_items) n <<= 1;
    DevBuf acc(ctx);
    Table* t = new Table();
    int st = VC_OK;
    if (ctx->curve == VC_CURVE_BN254) {
        const uint64_t gx[4] = {1, 0, 0, 0}, gy[4] = {2, 0, 0, 0};
        st = kzg_srs_acc<BN254G1, BN254Fr>(ctx, max_items, n, secret, 5, gx, gy, acc);
    } else if (ctx->curve == VC_CURVE_BLS12_381) {
        const uint64_t gx[6] = {0xfb3af00adb22c6bbull, 0x6c55e83ff97a1aefull, 0xa14e3a3f171bac58ull,
                                0xc3688c4f9774b905ull, 0x2695638c4fa9ac0full, 0x17f1d3a73197d794ull};
        const uint64_t gy[6] = {0x0caa232946c5e7e1ull, 0xd03cc744a2888ae4ull, 0x00db18cb2c04b3edull,
                                0xfcf5e095d5d00af6ull, 0xa09e30ed741d8ae4ull, 0x08b3f481e3aaa0f1ull};
        st = kzg_srs_acc<BLS381G1, BLS381Fr>(ctx, max_items, n, secret, 7, gx, gy, acc);
    } else {
        st = VC_E_INVALID;
    }
    if (st == VC_OK) st = table_from_acc(ctx, t, acc.p, n);
    if (st != VC_OK) {
        delete t;
        return st;
    }
    t->subgroup = 1;  // l_j(s) * G
    ctx->tables.push_back(t);
    *table_id = (int)ctx->tables.size() - 1;
    if (size) *size = n;
    return VC_OK;
}

int vc_kzg_prove(vc_ctx* ctx, int table, size_t size, const uint64_t* evals, size_t max, const uint64_t* point,
                 uint64_t* proof_xy, uint8_t* proof_inf, uint64_t* y) {
    if (!ctx || (max && !evals) || !point || !proof_xy || !proof_inf || !y) return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    return kzg_prove_any(ctx, t, size, evals, max, point, proof_xy, proof_inf, y, nullptr);
}

int vc_kzg_prove_device(vc_ctx* ctx, int table, size_t size, const void* d_evals, size_t max,
                        const uint64_t* point, uint64_t* proof_xy, uint8_t* proof_inf, uint64_t* y) {
    if (!ctx || (max && !d_evals) || !point || !proof_xy || !proof_inf || !y) return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    const uint64_t* ev = reinterpret_cast<const uint64_t*>(d_evals);
    return kzg_prove_any(ctx, t, size, ev, max, point, proof_xy, proof_inf, y, nullptr, true);
}

int vc_kzg_commit_prove_device(vc_ctx* ctx, int table, size_t size, const void* d_evals, size_t max,
                               const uint64_t* point, uint64_t* com_xy, uint8_t* com_inf, uint64_t* proof_xy,
                               uint8_t* proof_inf, uint64_t* y) {
    if (!ctx || (max && !d_evals) || !point || !com_xy || !com_inf || !proof_xy || !proof_inf || !y)
        return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    const uint64_t* ev = reinterpret_cast<const uint64_t*>(d_evals);
    return kzg_prove_any(ctx, t, size, ev, max, point, proof_xy, proof_inf, y, nullptr, true, 0, 1, (uint32_t*)nullptr,
                         com_xy, com_inf);
}

int vc_kzg_prove_device_part(vc_ctx* ctx, int table, size_t size, const void* d_evals, size_t max,
                             const uint64_t* point, int part, int parts, uint32_t* out_acc, uint64_t* y) {
    if (!ctx || (max && !d_evals) || !point || !out_acc || !y || parts < 1 || part < 0 || part >= parts)
        return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    const uint64_t* ev = reinterpret_cast<const uint64_t*>(d_evals);
    return kzg_prove_any(ctx, t, size, ev, max, point, nullptr, nullptr, y, nullptr, true, part, parts, out_acc);
}

int vc_kzg_prove_all_points(vc_ctx* ctx, int table, size_t size, const uint64_t* evals, size_t n_evals, int mode,
                            uint64_t* out_xy, uint8_t* out_inf, uint64_t* out_y, size_t* count) {
    if (!ctx || (n_evals && !evals) || !out_xy || !out_inf || !out_y || !count) return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    if (ctx->curve == VC_CURVE_BN254)
        return fk_all_t<BN254G1, BN254Fr>(ctx, t, size, evals, n_evals, mode, out_xy, out_inf, out_y, count);
    if (ctx->curve == VC_CURVE_BLS12_381)
        return fk_all_t<BLS381G1, BLS381Fr>(ctx, t, size, evals, n_evals, mode, out_xy, out_inf, out_y, count);
    return VC_E_INVALID;
}

int vc_kzg_quotient(vc_ctx* ctx, size_t size, const uint64_t* evals, size_t max, const uint64_t* point,
                    uint64_t* q_out, uint64_t* y) {
    if (!ctx || (max && !evals) || !point || !q_out || !y) return VC_E_INVALID;
    Guard g(ctx);
    return kzg_prove_any(ctx, nullptr, size, evals, max, point, nullptr, nullptr, y, q_out);
}

}  // extern "C"

namespace vk {
// ---------------------------------------------------------------- range-sharded KZG open
// One member's share of KZG::prove_point (kzg/mod.rs:136-154) split by index range (SURVEY 8(e)
// C4): the member uploads only f on [lo, hi), computes q there, and its MSM covers the SRS points
// [lo, hi) (a point range on the table's radix copies). The global sum of each case leaves as one
// field partial (phase 1), the members' total comes back (phase 2). vc_group_kzg_prove drives it.
struct KzgShare {
    vc_ctx* ctx = nullptr;
    Table* t = nullptr;
    size_t n = 0, lo = 0, L = 0, nvalid = 0, m = 0;
    bool in_domain = false;
    uint32_t point[8] = {0}, omega[8] = {0};  // Montgomery Fr words
    uint64_t y_in[4] = {0};                   // in domain: y = f_m (canonical)
    DevBuf f, q, inv, part;
    explicit KzgShare(vc_ctx* c) : ctx(c), f(c), q(c), inv(c), part(c) {}
};

template <class C_, class Fr_>
static int kzg_share_begin_t(vc_ctx* ctx, Table* t, size_t size, const uint64_t* evals, size_t max,
                             const uint64_t* point, size_t lo, size_t hi, KzgShare* s, uint64_t* partial) {
    using Fe = fe<Fr_>;
    if (!is_pow2(size) || (size >> 31) || max > size || lo > hi || hi > size) return VC_E_INVALID;
    if (t->n < size) return VC_E_RANGE;
    VK_TRY(open_point_status<Fr_>(size, point));  // every member sees the same point: all fail alike
    s->ctx = ctx;
    s->t = t;
    s->n = size;
    s->lo = lo;
    s->L = hi - lo;
    s->nvalid = max > lo ? std::min(max, hi) - lo : 0;
    const Fe pm = canon_to_mont<Fr_>(point);
    const Fe omega = group_gen_t<Fr_>(size, fr_generator<Fr_>());
    memcpy(s->point, pm.v, 32);
    memcpy(s->omega, omega.v, 32);
    // prove_point: `point <= size` -> the in-domain branch with index to_usize(point)
    const Fe pc = fe_from_mont<Fr_>(pm);
    bool small = true;
    for (int i = 2; i < Fr_::N; i++) small &= pc.v[i] == 0;
    const uint64_t pv = (uint64_t)pc.v[0] | ((uint64_t)pc.v[1] << 32);
    s->in_domain = small && pv <= size;
    if (s->in_domain && pv == size) return VC_E_DOMAIN;  // vanishing_at(size) out of bounds
    s->m = s->in_domain ? (size_t)pv : 0;
    Fe fm = fe_zero<Fr_>();
    if (s->in_domain && s->m < max) {  // y = evaluate(point): the stored value, or 0 in [max, size]
        memcpy(s->y_in, evals + 4 * s->m, 32);
        fm = canon_to_mont<Fr_>(evals + 4 * s->m);
    }
    const size_t L = std::max<size_t>(s->L, 1);
    VK_TRY(s->f.ensure(L * 32));
    VK_TRY(s->q.ensure(L * 32));
    VK_TRY(s->inv.ensure(L * 32));
    if (s->nvalid)
        VK_CHECK_HIP(hipMemcpyAsync(s->q.p, evals + 4 * lo, s->nvalid * 32, hipMemcpyHostToDevice, ctx->stream));
    // (an empty share, size < G, has nothing to convert: no launch with a grid of zero blocks)
    if (s->L) VK_TRY(canon_to_mont_dev<Fr_>(ctx, s->q.p, s->L, s->nvalid, s->f.as<Fe>()));
    Fe part;
    VK_TRY(kzg_range_part<Fr_>(ctx, size, s->f.as<Fe>(), s->nvalid, lo, s->L, pm, omega, s->in_domain, s->m, fm,
                               s->q.as<Fe>(), s->inv.as<Fe>(), s->part, &part));
    memcpy(partial, part.v, 32);
    return VC_OK;
}

template <class C_, class Fr_>
static int kzg_share_finish_t(KzgShare* s, const uint64_t* total, uint32_t* out_acc, uint64_t* y) {
    using Fe = fe<Fr_>;
    vc_ctx* ctx = s->ctx;
    Fe tot, pm, omega, ym = fe_zero<Fr_>();
    memcpy(tot.v, total, 32);
    memcpy(pm.v, s->point, 32);
    memcpy(omega.v, s->omega, 32);
    VK_TRY(kzg_range_finish<Fr_>(ctx, s->n, s->f.as<Fe>(), s->nvalid, s->lo, s->L, pm, omega, s->in_domain, s->m, tot,
                                 s->q.as<Fe>(), s->inv.as<Fe>(), &ym));
    if (s->in_domain) memcpy(y, s->y_in, 32);
    else mont_to_canon<Fr_>(ym, y);
    if (s->L == 0) {  // an empty share adds the identity
        typename C_::Acc z = C_::zero();
        memcpy(out_acc, &z, sizeof z);
        return VC_OK;
    }
    return msm_run(ctx, s->t, s->lo, s->q.p, s->L, 1, out_acc);
}

int kzg_share_begin(vc_ctx* ctx, int table, size_t size, const uint64_t* evals, size_t max, const uint64_t* point,
                    size_t lo, size_t hi, KzgShare** out, uint64_t* partial) {
    if (!ctx || !out || !point || !partial || (max && !evals)) return VC_E_INVALID;
    *out = nullptr;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    KzgShare* s = new KzgShare(ctx);
    int st = VC_E_INVALID;
    if (ctx->curve == VC_CURVE_BN254)
        st = kzg_share_begin_t<BN254G1, BN254Fr>(ctx, t, size, evals, max, point, lo, hi, s, partial);
    else if (ctx->curve == VC_CURVE_BLS12_381)
        st = kzg_share_begin_t<BLS381G1, BLS381Fr>(ctx, t, size, evals, max, point, lo, hi, s, partial);
    if (st != VC_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        delete s;  // (the pooled buffers return to the pool under the lock held here)
        return st;
    }
    *out = s;
    return VC_OK;
}

int kzg_share_finish(KzgShare* s, const uint64_t* total, uint32_t* out_acc, uint64_t* y) {
    if (!s || !total || !out_acc || !y) return VC_E_INVALID;
    Guard g(s->ctx);
    if (s->ctx->curve == VC_CURVE_BN254) return kzg_share_finish_t<BN254G1, BN254Fr>(s, total, out_acc, y);
    return kzg_share_finish_t<BLS381G1, BLS381Fr>(s, total, out_acc, y);
}

void kzg_share_free(KzgShare* s) {
    if (!s) return;
    {
        Guard g(s->ctx);  // the pooled buffers go back to their context's pool under its lock
        (void)hipStreamSynchronize(s->ctx->stream);
        s->f.release();
        s->q.release();
        s->inv.release();
        s->part.release();
    }
    delete s;
}

// sum of G range partials (Montgomery Fr words of the context's scalar field)
template <class Fr_>
static int share_sum_t(const uint64_t* parts, int G, uint64_t* total) {
    fe<Fr_> a = fe_zero<Fr_>(), b;
    for (int k = 0; k < G; k++) {
        memcpy(b.v, parts + 4 * (size_t)k, 32);
        a = fe_add<Fr_>(a, b);
    }
    memcpy(total, a.v, 32);
    return VC_OK;
}
int kzg_share_sum(int curve, const uint64_t* parts, int G, uint64_t* total) {
    if (curve == VC_CURVE_BN254) return share_sum_t<BN254Fr>(parts, G, total);
    if (curve == VC_CURVE_BLS12_381) return share_sum_t<BLS381Fr>(parts, G, total);
    return VC_E_INVALID;
}

}  // namespace vk

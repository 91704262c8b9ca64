// Protocol layer on the GPU engine (reference: vector-commit/src/{ipa,kzg}/mod.rs,
// multiproof.rs, lagrange_basis.rs, precompute.rs). Serial Fiat-Shamir stays on the host
// (scheme_host.cpp); every MSM, batch of commitments, quotient and big field pass runs on
// the device. This file: the host helpers the protocols share (ipa.hip, kzg_open.hip,
// multiproof.hip; declared in scheme_internal.hpp) and to_data_item.
#include "protocol.hpp"

namespace vk {

// ---------------------------------------------------------------- host point helpers
Acc acc_of(const uint64_t* xy, bool inf) {
    if (inf) return C::zero();
    Acc a;
    a.x = canon_to_mont<BN254Fq>(xy);
    a.y = canon_to_mont<BN254Fq>(xy + 4);
    a.zz = fe_one<BN254Fq>();
    a.zzz = fe_one<BN254Fq>();
    return a;
}
void aff_of(const Acc& a, uint64_t* xy, uint8_t* inf) {
    acc_to_affine(VC_CURVE_BN254, reinterpret_cast<const uint32_t*>(&a), xy, inf);
}

std::vector<Fr> host_batch_inv(const std::vector<Fr>& v) {
    std::vector<Fr> pre(v.size());
    Fr acc = fe_one<F>();
    for (size_t i = 0; i < v.size(); i++) {
        pre[i] = acc;
        if (!fe_is_zero<F>(v[i])) acc = fe_mul<F>(acc, v[i]);
    }
    Fr inv = fe_inv_bin<F>(acc);
    std::vector<Fr> out(v.size());
    for (size_t i = v.size(); i-- > 0;) {
        if (fe_is_zero<F>(v[i])) {
            out[i] = fe_zero<F>();
            continue;
        }
        out[i] = fe_mul<F>(inv, pre[i]);
        inv = fe_mul<F>(inv, v[i]);
    }
    return out;
}

// compute_barycentric_coefficients' one-hot branch (precompute.rs:75-79): the point is below
// `size` as an integer (ipav::point_in_domain is this test on canonical words)
static bool one_hot_index(size_t size, const Fr& point, uint64_t* idx) {
    Fr pc = fe_from_mont<F>(point);
    bool small = true;
    for (int i = 2; i < 8; i++) small &= pc.v[i] == 0;
    *idx = (uint64_t)pc.v[0] | ((uint64_t)pc.v[1] << 32);
    return small && *idx < size;
}

// PrecomputedLagrange::compute_barycentric_coefficients (precompute.rs:72-90)
std::vector<Fr> barycentric(size_t size, const Fr& point, const Fr& omega) {
    std::vector<Fr> res(size, fe_zero<F>());
    uint64_t pv;
    if (one_hot_index(size, point, &pv)) {
        res[pv] = fe_one<F>();
        return res;
    }
    Fr t = fe_mul<F>(fe_sub<F>(fe_pow_u64<F>(point, size), fe_one<F>()), fe_inv_bin<F>(fr_u64(size)));
    std::vector<Fr> pw(size), den(size);
    Fr w = fe_one<F>();
    for (size_t i = 0; i < size; i++) {
        pw[i] = w;
        den[i] = fe_sub<F>(point, w);
        w = fe_mul<F>(w, omega);
    }
    std::vector<Fr> inv = host_batch_inv(den);
    for (size_t i = 0; i < size; i++) res[i] = fe_mul<F>(fe_mul<F>(t, pw[i]), inv[i]);
    return res;
}

// compute_barycentric_coefficients divides by (point - w^i) for every i (precompute.rs:85,
// ark-ff Div = inverse().unwrap()): a point that is a domain element w^i but not below `size`
// as an integer (the one-hot branch, :75-79) makes the reference panic. host_batch_inv maps 1/0
// to 0, which would give all-zero weights and let verify accept y = 0 for any commitment, so
// the callers map this case to VC_E_DOMAIN instead (as the KZG B.4 panic).
bool barycentric_panics(size_t size, const Fr& point) {
    uint64_t pv;
    if (one_hot_index(size, point, &pv)) return false;
    // point^size == 1  <=>  point is one of the size-th roots of unity w^i
    return fe_eq<F>(fe_pow_u64<F>(point, size), fe_one<F>());
}

// width-w fixed-base commitments of Montgomery scalars (host) -> canonical affine (host)
// overlap: host work run while the commit kernel runs (fb_commit_t)
int commit_batch(vc_ctx* ctx, Table* t, size_t width, const Fr* sc, size_t batch, uint64_t* out_xy, uint8_t* out_inf,
                 const std::function<void()>* overlap) {
    const size_t in_bytes = batch * width * 32, out_bytes = batch * 65;
    VK_TRY(ctx->ws[WS_MISC].ensure(out_bytes));
    uint8_t* dxy = ctx->ws[WS_MISC].as<uint8_t>();
    uint8_t* dinf = dxy + batch * 64;
    // pinned staging both ways (the IPA rounds call this 8 times per proof: pageable copies went
    // through bounce buffers), points and flags read back in one copy; the scalars are uploaded by
    // msm_batch_run, or read in place by its latency path
    VK_TRY(ctx->pin_io.ensure(std::max(in_bytes, out_bytes)));
    memcpy(ctx->pin_io.p, sc, in_bytes);
    bool on_host = false;
    VK_TRY(msm_batch_run(ctx, t, width, nullptr, batch, 1, dxy, dinf, out_xy, out_inf, &on_host, &ctx->pin_io,
                         overlap));
    if (on_host) return VC_OK;
    VK_CHECK_HIP(hipMemcpyAsync(ctx->pin_io.p, dxy, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(out_xy, ctx->pin_io.p, batch * 64);
    memcpy(out_inf, static_cast<const uint8_t*>(ctx->pin_io.p) + batch * 64, batch);
    return VC_OK;
}

// Straus on the host pool for the verifiers' few-point MSMs (IPA verify: C and the 2K proof
// points L_k / R_k, 17 at N = 256): on the GPU every term pays the Pippenger pipeline's fixed
// latency (upload, sort, accumulate, fix-up, reductions: ~0.25 ms for 17 points); here each pool
// thread takes a slice of the points -- 4-bit windows over 15 precomputed multiples, 252 shared
// doublings -- and the slices are added (~0.1 ms). The points are checked as bases_fill checks
// them (canonical coordinates, on the curve: VC_E_NOT_ON_CURVE).
int host_msm(const uint64_t* xy, const uint8_t* inf, const Fr* sc, size_t n, Acc* out) {
    using Fq = BN254Fq;
    std::vector<Acc> base(n, C::zero());
    for (size_t i = 0; i < n; i++) {
        if (inf[i]) continue;
        fe<Fq> x, y;
        memcpy(x.v, xy + 8 * i, 32);
        memcpy(y.v, xy + 8 * i + 4, 32);
        if (!fe_eq<Fq>(fe_reduce_once<Fq>(x), x) || !fe_eq<Fq>(fe_reduce_once<Fq>(y), y)) return VC_E_NOT_ON_CURVE;
        x = fe_to_mont<Fq>(x);
        y = fe_to_mont<Fq>(y);
        fe<Fq> b = fe_zero<Fq>();
        b.v[0] = (uint32_t)C::COEFF_B;
        if (!fe_eq<Fq>(fe_add<Fq>(fe_mul<Fq>(fe_sqr<Fq>(x), x), fe_to_mont<Fq>(b)), fe_sqr<Fq>(y)))
            return VC_E_NOT_ON_CURVE;
        base[i].x = x;
        base[i].y = y;
        base[i].zz = fe_one<Fq>();
        base[i].zzz = fe_one<Fq>();
    }
    HostPool& pool = host_pool();
    const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>(pool.size(), n));
    std::vector<Acc> part(T, C::zero());
    pool.run([&](unsigned k) {
        if (k >= T) return;
        const size_t lo = n * k / T, hi = n * (k + 1) / T;
        std::vector<Acc> mult((hi - lo) * 16);
        std::vector<Fr> can(hi - lo);
        for (size_t i = lo; i < hi; i++) {
            Acc* m = &mult[(i - lo) * 16];
            m[1] = base[i];
            m[2] = C::dbl(base[i]);
            for (int j = 3; j < 16; j++) m[j] = C::add(m[j - 1], base[i]);
            can[i - lo] = fe_from_mont<F>(sc[i]);
        }
        Acc acc = C::zero();
        for (int w = 63; w >= 0; w--) {  // nibbles of the 256-bit canonical scalars, top first
            if (!C::is_zero(acc))
                for (int d = 0; d < 4; d++) acc = C::dbl(acc);
            for (size_t i = lo; i < hi; i++) {
                const uint32_t nib = (can[i - lo].v[w >> 3] >> (4 * (w & 7))) & 15u;
                if (nib) acc = C::add(acc, mult[(i - lo) * 16 + nib]);
            }
        }
        part[k] = acc;
    });
    Acc r = C::zero();
    for (const Acc& p : part) r = C::add(r, p);
    *out = r;
    return VC_OK;
}

// variable-base MSM over host points (ctx scratch table) with Montgomery scalars -> Acc
// filled: the points are in ctx->scratch already (bases_fill run by the caller)
int msm_points(vc_ctx* ctx, const uint64_t* xy, const uint8_t* inf, const std::vector<Fr>& sc, Acc* out,
               bool filled) {
    size_t n = sc.size();
    if (n <= HOST_MSM_MAX) return host_msm(xy, inf, sc.data(), n, out);
    const double c0 = host_timing() ? clock_us() : 0.0;
    if (!filled) VK_TRY(bases_fill(ctx, &ctx->scratch, xy, inf, n));
    if (host_timing()) {
        VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        fprintf(stderr, "msm_points n=%zu bases_fill_us=%.1f\n", n, clock_us() - c0);
    }
    DevBuf d(ctx);
    VK_TRY(d.ensure(std::max<size_t>(n, 1) * 32));
    VK_CHECK_HIP(hipMemcpyAsync(d.p, sc.data(), n * 32, hipMemcpyHostToDevice, ctx->stream));
    VK_TRY(msm_run(ctx, &ctx->scratch, 0, d.p, n, 1, reinterpret_cast<uint32_t*>(out)));
    return VC_OK;
}

// ---------------------------------------------------------------- to_data_item (a13)
__global__ void k_to_data_item(const fe<BN254Fq>* __restrict__ xy, const uint8_t* __restrict__ inf, size_t n,
                               fe<F>* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = to_data_item_canon(xy[2 * i], xy[2 * i + 1], inf[i] != 0);
}

int to_data_item_device(vc_ctx* ctx, const void* d_xy, const uint8_t* d_inf, size_t n, void* d_items) {
    if (n == 0) return VC_OK;
    VK_LAUNCH(ctx, "to_data_item", k_to_data_item, (n + 255) / 256, 256, 0, static_cast<const fe<BN254Fq>*>(d_xy),
              d_inf, n, static_cast<fe<F>*>(d_items));
    return VC_OK;
}

}  // namespace vk

using namespace vk;

extern "C" {

int vc_to_data_item_batch(vc_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, uint64_t* out) {
    if (!ctx || (n && (!xy || !inf || !out))) return VC_E_INVALID;
    if (ctx->curve != VC_CURVE_BN254) return VC_E_INVALID;
    Guard g(ctx);
    if (n == 0) return VC_OK;
    DevBuf dxy(ctx), dinf(ctx), dout(ctx);
    VK_TRY(dxy.ensure(n * 64));
    VK_TRY(dinf.ensure(n));
    VK_TRY(dout.ensure(n * 32));
    VK_CHECK_HIP(hipMemcpyAsync(dxy.p, xy, n * 64, hipMemcpyHostToDevice, ctx->stream));
    VK_CHECK_HIP(hipMemcpyAsync(dinf.p, inf, n, hipMemcpyHostToDevice, ctx->stream));
    VK_TRY(to_data_item_device(ctx, dxy.p, dinf.as<uint8_t>(), n, dout.p));
    VK_CHECK_HIP(hipMemcpyAsync(out, dout.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return VC_OK;
}

}  // extern "C"

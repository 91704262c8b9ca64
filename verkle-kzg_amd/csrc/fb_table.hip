// Fixed-base window tables (the commits over them: commit.hip). The bases never change, so each
// base G_i gets a window table
//     T[i][w][k] = (k+1) * 2^(c*w) * G_i     (affine, Montgomery; k < 2^(c-1))
// held in HBM (width 256, c = 8: 67 MB BN254 / 100 MB Bandersnatch -- L3-resident; c = 16:
// 8.6-13 GB, which only a 288 GB part can afford). Also here: a table's bases from projective
// accumulators (table_from_acc) and the first bases' table of their own (lead_table).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "batch_inv.hpp"
#include "commit_internal.hpp"
#include "ec29.hpp"

namespace vk {

// Table entry: FbE<C> (ec29.hpp).

// copy one window's NBw normalised multiples into the table: tab[i*stride + off(w) + k] =
// aff[i*NBw + k], in the packed-29 form the commit loops read
template <class C>
__global__ void k_fb_place(const typename C::Aff* __restrict__ aff, uint32_t n, uint32_t NBw, FbGeom g, int w,
                           FbE<C>* __restrict__ tab) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (size_t)n * NBw) return;
    size_t i = j / NBw, k = j - i * NBw;
    using FC = typename Fast29<C>::type;
    typename C::Aff packed;
    FC::pack_aff(aff[j], &packed);  // canonical x R'
    tab[i * g.stride() + g.off(w) + k].u = FC::load(&packed);
}

template <class C>
__device__ typename C::Acc mul_small_fb(const typename C::Acc& p, uint32_t k) {
    typename C::Acc r = C::zero();
    if (k == 0) return r;
    int top = 31 - __builtin_clz(k);
    r = p;
    for (int i = top - 1; i >= 0; i--) {
        r = C::dbl(r);
        if ((k >> i) & 1) r = C::add(r, p);
    }
    return r;
}

// Q[i] = 2^(c*w) * G_i for the given window (chained: caller passes the previous window)
template <class C>
__global__ void k_fb_shift(typename C::Acc* __restrict__ Q, const typename C::Aff* __restrict__ bases,
                           uint32_t n, int c, int first) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typename C::Acc q;
    if (first) q = C::from_aff(bases[i], false);
    else {
        q = Q[i];
        for (int k = 0; k < c; k++) q = C::dbl(q);
    }
    Q[i] = q;
}

// tmp[i][k] = (k+1) * Q[i], chunks of CH consecutive k per thread
template <class C>
__global__ void k_fb_fill(const typename C::Acc* __restrict__ Q, uint32_t n, uint32_t NBk, uint32_t CH,
                          typename C::Acc* __restrict__ tmp) {
    uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t nch = (NBk + CH - 1) / CH;
    uint32_t i = gid / nch, ch = gid % nch;
    if (i >= n) return;
    typename C::Acc q = Q[i];
    uint32_t k0 = ch * CH, k1 = min(k0 + CH, NBk);
    typename C::Acc p = mul_small_fb<C>(q, k0 + 1);
    for (uint32_t k = k0; k < k1; k++) {
        tmp[(size_t)i * NBk + k] = p;
        p = C::add(p, q);
    }
}

// One workgroup normalises 256 consecutive accumulators with one field inversion of its own, on a
// lane (batch_inv.hpp; ~130 us, which a table build does not mind: the commits' outputs go through
// normalize.hip's split form)
template <class C>
__global__ void __launch_bounds__(256) k_normalize(const typename C::Acc* __restrict__ in, size_t count,
                                                  typename C::Aff* __restrict__ out_aff,
                                                  uint32_t* __restrict__ out_canon,
                                                  uint8_t* __restrict__ out_inf) {
    using F = typename C::F;
    __shared__ fe<F> pre[256];
    __shared__ fe<F> suf[256];
    __shared__ fe<F> tinv;
    size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    typename C::Acc a = j < count ? in[j] : C::zero();
    block_scan256<F>((j < count && !norm_as_one<C>(a)) ? denom<C>(a) : fe_one<F>(), pre, suf);
    if (threadIdx.x == 0) tinv = fe_inv_bin<F>(pre[255]);
    __syncthreads();
    const fe<F> iz = fe_mul<F>(tinv, scan_others<F>(pre, suf));
    if (j >= count) return;
    fe<F> x, y;
    bool ident;
    acc_affine<C>(a, iz, x, y, ident);
    store_affine<C>(j, x, y, ident, out_aff, out_canon, out_inf);
}

// windows = 0: uniform c-bit windows; otherwise `windows` windows of c or c + 1 bits (the last
// bits + 1 - c windows wide), which must cover the scalar's bits + 1
template <class C>
static int fb_precompute_t(vc_ctx* ctx, Table* t, int c, int windows) {
    using Acc = typename C::Acc;
    using Aff = typename C::Aff;
    using Fr = ScalarOf<C>;
    if (c < 4 || c > 20 || windows < 0) return VC_E_INVALID;
    const uint32_t n = (uint32_t)t->n;
    int W = (Fr::BITS + 1 + c - 1) / c, big = 0;
    if (windows > 0 && windows < W) {
        big = Fr::BITS + 1 - c * windows;
        if (big > windows || c == 20) return VC_E_INVALID;  // needs wider windows than c + 1
        W = windows;
    }
    const FbGeom g{c, W, big};
    const uint32_t NBk = 1u << (c - 1), NBmax = big ? 2 * NBk : NBk;
    if (t->fb_c == c && t->fb_W == W && t->fb_big == big && t->fb.p) return VC_OK;
    t->fb.release();
    t->fb_c = 0;
    t->fb_auto = false;  // (commit.hip fb_commit_t marks its own first-use builds)
    VK_TRY(t->fb.ensure(std::max<size_t>((size_t)n * g.stride(), 1) * sizeof(FbE<C>)));
    DevBuf Q, tmp, aff_w;
    VK_TRY(Q.ensure(std::max<uint32_t>(n, 1) * sizeof(Acc)));
    VK_TRY(tmp.ensure(std::max<size_t>((size_t)n * NBmax, 1) * sizeof(Acc)));
    VK_TRY(aff_w.ensure(std::max<size_t>((size_t)n * NBmax, 1) * sizeof(Aff)));
    for (int w = 0; w < W; w++) {
        const uint32_t NBw = 1u << (g.width(w) - 1);
        const uint32_t CH = NBw >= 64 ? 64 : NBw;
        const uint32_t nch = (NBw + CH - 1) / CH;
        // Q = 2^(bits below window w) G: the previous window's width more doublings
        VK_LAUNCH(ctx, "fb_shift", (k_fb_shift<C>), (n + 255) / 256, 256, 0, Q.as<Acc>(),
                  t->bases.as<Aff>(), n, w == 0 ? 0 : g.width(w - 1), w == 0 ? 1 : 0);
        VK_LAUNCH(ctx, "fb_fill", (k_fb_fill<C>), ((size_t)n * nch + 127) / 128, 128, 0, Q.as<Acc>(), n,
                  NBw, CH, tmp.as<Acc>());
        size_t cnt = (size_t)n * NBw;
        VK_LAUNCH(ctx, "fb_normalize", (k_normalize<C>), (cnt + 255) / 256, 256, 0, tmp.as<Acc>(), cnt,
                  aff_w.as<Aff>(), (uint32_t*)nullptr, (uint8_t*)nullptr);
        VK_LAUNCH(ctx, "fb_place", (k_fb_place<C>), (cnt + 255) / 256, 256, 0, aff_w.as<Aff>(), n, NBw, g, w,
                  t->fb.as<FbE<C>>());
    }
    VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    t->fb_c = c;
    t->fb_W = W;
    t->fb_big = big;
    return VC_OK;
}

// table <- normalised projective accumulators (device), e.g. a freshly computed SRS
template <class C>
static int table_from_acc_t(vc_ctx* ctx, Table* t, const void* d_acc, size_t n) {
    t->curve = ctx->curve;
    t->n = n;
    t->fb_c = t->fb_W = t->fb_big = 0;
    t->fb_auto = false;
    t->fb.release();
    delete t->lead;
    t->lead = nullptr;
    t->lead_k = t->lead_c = 0;
    t->fast_ok = t->phi_ok = t->win_ok = 0;
    VK_TRY(t->bases.ensure(std::max<size_t>(n, 1) * sizeof(typename C::Aff)));
    VK_TRY(t->inf.ensure(std::max<size_t>(n, 1)));
    if (n == 0) return VC_OK;
    VK_LAUNCH(ctx, "normalize_table", (k_normalize<C>), (n + 255) / 256, 256, 0,
              reinterpret_cast<const typename C::Acc*>(d_acc), n, t->bases.as<typename C::Aff>(),
              (uint32_t*)nullptr, t->inf.as<uint8_t>());
    VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return VC_OK;
}
int table_from_acc(vc_ctx* ctx, Table* t, const void* d_acc, size_t n) {
    switch (ctx->curve) {
        case VC_CURVE_BN254: return table_from_acc_t<BN254G1>(ctx, t, d_acc, n);
        case VC_CURVE_BLS12_381: return table_from_acc_t<BLS381G1>(ctx, t, d_acc, n);
        case VC_CURVE_BANDERSNATCH: return table_from_acc_t<Bandersnatch>(ctx, t, d_acc, n);
    }
    return VC_E_INVALID;
}

template <class C>
static int lead_table_t(vc_ctx* ctx, Table* t, int k, int c, Table** out) {
    using Aff = typename C::Aff;
    *out = nullptr;
    if (k <= 0 || (size_t)k > t->n) return VC_E_INVALID;
    if (t->lead && t->lead_k == k && t->lead_c == c) {
        *out = t->lead;
        return VC_OK;
    }
    delete t->lead;
    t->lead = nullptr;
    // only where it leaves the device 4 GB free (as the first-use tables, fb_default_c): otherwise
    // no lead table and the caller keeps t; it then counts in the context's fb_auto_used()
    {
        static_assert(sizeof(FbE<C>) == 128, "fb_auto_bytes counts 128-byte entries");
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
            fb_auto_bytes<ScalarOf<C>>((size_t)k, c) > (double)free_b - 4e9)
            return VC_OK;
    }
    Table* s = new Table();
    s->curve = t->curve;
    s->n = (size_t)k;
    s->subgroup = t->subgroup;
    int st = s->bases.ensure((size_t)k * sizeof(Aff));
    if (st == VC_OK) st = s->inf.ensure((size_t)k);
    if (st == VC_OK && (hipMemcpyAsync(s->bases.p, t->bases.p, (size_t)k * sizeof(Aff), hipMemcpyDeviceToDevice,
                                       ctx->stream) != hipSuccess ||
                        hipMemcpyAsync(s->inf.p, t->inf.p, (size_t)k, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess))
        st = VC_E_HIP;
    if (st == VC_OK) st = fixed_base_precompute(ctx, s, c);
    if (st != VC_OK) {
        delete s;
        (void)hipGetLastError();
        return st == VC_E_OOM ? VC_OK : st;  // out of memory: no lead table, the caller keeps t
    }
    t->lead = s;
    t->lead_k = k;
    t->lead_c = c;
    *out = s;
    return VC_OK;
}
int lead_table(vc_ctx* ctx, Table* t, int k, int c, Table** out) {
    switch (t->curve) {
        case VC_CURVE_BN254: return lead_table_t<BN254G1>(ctx, t, k, c, out);
        case VC_CURVE_BLS12_381: return lead_table_t<BLS381G1>(ctx, t, k, c, out);
        case VC_CURVE_BANDERSNATCH: return lead_table_t<Bandersnatch>(ctx, t, k, c, out);
    }
    *out = nullptr;
    return VC_E_INVALID;
}

int fixed_base_precompute(vc_ctx* ctx, Table* t, int c, int windows) {
    switch (t->curve) {
        case VC_CURVE_BN254: return fb_precompute_t<BN254G1>(ctx, t, c, windows);
        case VC_CURVE_BLS12_381: return fb_precompute_t<BLS381G1>(ctx, t, c, windows);
        case VC_CURVE_BANDERSNATCH: return fb_precompute_t<Bandersnatch>(ctx, t, c, windows);
    }
    return VC_E_INVALID;
}

}  // namespace vk

// Table preparation of the Pippenger MSM (msm.hip), once per table: the packed-29 copies of the
// bases, the GLV subgroup check and endomorphism images, the shared-window copies (Table::win).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <type_traits>
#include "ec.hpp"
#include "ec29.hpp"
#include "msm_digits.hpp"  // GlvK
#include "msm_internal.hpp"

namespace vk {
// ec.hpp affine points -> packed-29 form (the tables the accumulate / commit loops read)
template <class C>
__global__ void __launch_bounds__(256) k_to_fast(const typename C::Aff* __restrict__ in, size_t n,
                                                typename C::Aff* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fast29<C>::type::pack_aff(in[i], out + i);
}

// ... or straight to radix-2^29 limbs (the shared-window copies: the accumulate reads them with
// no unpacking), in the signed limb form (x, y, -y)
template <class C>
__global__ void __launch_bounds__(256) k_to_limbs_n(const typename C::Aff* __restrict__ in, size_t n,
                                                   typename Fast29<C>::type::AffN* __restrict__ out) {
    using FC = typename Fast29<C>::type;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typename C::Aff a = in[i], packed;
    FC::pack_aff(a, &packed);
    const typename FC::Aff l = FC::load(&packed);
    a.y = fe_neg<typename C::F>(a.y);
    FC::pack_aff(a, &packed);
    typename FC::AffN o;
    o.x = l.x;
    o.y = l.y;
    o.ny = FC::load(&packed).y;
    out[i] = o;
}

// ... and to the pair layout (x, y) | (x, -y), one 128-B record each
template <class C>
__global__ void __launch_bounds__(256) k_to_limbs_p(const typename C::Aff* __restrict__ in, size_t n,
                                                   typename Fast29<C>::type::AffP* __restrict__ out) {
    using FC = typename Fast29<C>::type;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typename C::Aff a = in[i], packed;
    FC::pack_aff(a, &packed);
    const typename FC::Aff l = FC::load(&packed);
    a.y = fe_neg<typename C::F>(a.y);
    FC::pack_aff(a, &packed);
    typename FC::AffP o;
#pragma unroll
    for (int k = 0; k < FC::PADW; k++) o.pad[k] = 0;
    o.x = l.x;
    o.y = l.y;
    out[2 * i] = o;
    o.y = FC::load(&packed).y;
    out[2 * i + 1] = o;
}

template <class C>
__global__ void __launch_bounds__(256) k_glv_phi(const typename C::Aff* __restrict__ bases, uint32_t n,
                                                fe<typename C::F> beta, typename C::Aff* __restrict__ phi) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typename C::Aff p = bases[i];
    p.x = fe_mul<typename C::F>(p.x, beta);
    phi[i] = p;
}

// bad |= some base with phi^2(P) + z^2 P != 0 (phi^2 = (beta^2 x, y) has eigenvalue lambda^2 = -z^2)
template <class C>
__global__ void __launch_bounds__(256) k_glv_check(const typename C::Aff* __restrict__ bases,
                                                  const uint8_t* __restrict__ inf, uint32_t n,
                                                  fe<typename C::F> beta2, uint64_t z2lo, uint64_t z2hi,
                                                  uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || inf[i]) return;
    typename C::Aff p = bases[i];
    typename C::Acc acc = C::zero();
    for (int b = 127; b >= 0; b--) {
        acc = C::dbl(acc);
        const uint64_t w = b >= 64 ? z2hi : z2lo;
        if ((w >> (b & 63)) & 1) acc = C::madd(acc, p, false);
    }
    p.x = fe_mul<typename C::F>(p.x, beta2);
    acc = C::madd(acc, p, false);
    if (!C::is_zero(acc)) atomicOr(bad, 1u);
}

GlvK glv_consts() {
    return GlvK{{0x00000000ffffffffull, 0xac45a4010001a402ull},
                {0x63f6e522f6cfee30ull, 0x7c6becf1e01faaddull, 0x1ull},
                {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull}};
}
static const uint64_t GLV_BETA[6] = {0x8bfd00000000aaacull, 0x409427eb4f49fffdull, 0x897d29650fb85f9bull,
                                     0xaa0d857d89759ad4ull, 0xec02408663d4de85ull, 0x1a0111ea397fe699ull};
static const uint64_t GLV_BETA2[6] = {0x2e01fffffffefffeull, 0xde17d813620a0002ull, 0xddb3a93be6f89688ull,
                                      0xba69c6076a0f77eaull, 0x5f19672fdf76ce51ull, 0x0ull};
static fe<BLS381Fq> bls_fq_mont(const uint64_t* w) {
    fe<BLS381Fq> r;
    memcpy(r.v, w, sizeof(r.v));
    return fe_to_mont<BLS381Fq>(r);
}
static const uint64_t GLV_Z2[2] = {0x0000000100000000ull, 0xac45a4010001a402ull};  // z^2 = lambda + 1

// is every base of t in the prime-order subgroup? (checked once per table, cached)
int glv_table_ok(vc_ctx* ctx, Table* t, bool* ok) {
    using C = BLS381G1;
    if (t->subgroup < 0) {
        VK_TRY(ctx->ws[WS_GLV_FLAG].ensure(4));
        uint32_t* d_bad = ctx->ws[WS_GLV_FLAG].as<uint32_t>();
        VK_CHECK_HIP(hipMemsetAsync(d_bad, 0, 4, ctx->stream));
        if (t->n > 0)
            VK_LAUNCH(ctx, "glv_check", (k_glv_check<C>), (t->n + 255) / 256, 256, 0, t->bases.as<C::Aff>(),
                      t->inf.as<uint8_t>(), (uint32_t)t->n, bls_fq_mont(GLV_BETA2), GLV_Z2[0], GLV_Z2[1],
                      d_bad);
        uint32_t bad = 0;
        VK_CHECK_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream));
        VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        t->subgroup = bad ? 0 : 1;
    }
    *ok = t->subgroup == 1;
    return VC_OK;
}

// the packed-29 copies of a table's bases (and of phi(bases) for GLV MSMs), made once
template <class C>
int fast_tables(vc_ctx* ctx, Table* t, bool with_phi) {
    using Aff = typename C::Aff;
    const size_t need = (with_phi ? 2 : 1) * std::max<size_t>(t->n, 1) * sizeof(Aff);
    if (t->fast.cap < need) {
        t->fast_ok = t->phi_ok = 0;
        t->fast.release();
        VK_TRY(t->fast.ensure(need));
    }
    if (!t->fast_ok && t->n > 0) {
        VK_LAUNCH(ctx, "to_fast", (k_to_fast<C>), (t->n + 255) / 256, 256, 0, t->bases.as<Aff>(), t->n,
                  t->fast.as<Aff>());
        t->fast_ok = 1;
    }
    if constexpr (std::is_same<C, BLS381G1>::value) {
        if (with_phi && !t->phi_ok && t->n > 0) {
            DevBuf phi;
            VK_TRY(phi.ensure(t->n * sizeof(Aff)));
            VK_LAUNCH(ctx, "glv_phi", (k_glv_phi<C>), (t->n + 255) / 256, 256, 0, t->bases.as<Aff>(), (uint32_t)t->n,
                      bls_fq_mont(GLV_BETA), phi.as<Aff>());
            VK_LAUNCH(ctx, "to_fast", (k_to_fast<C>), (t->n + 255) / 256, 256, 0, phi.as<Aff>(), t->n,
                      t->fast.as<Aff>() + t->n);
            VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));  // before phi's buffer is freed
            t->phi_ok = 1;
        }
    }
    return VC_OK;
}

// out[i] = mul 2^c in[i] (mul odd and small; identity bases stay the identity)
template <class C>
__global__ void __launch_bounds__(256) k_win_next(const typename C::Aff* __restrict__ in,
                                                 const uint8_t* __restrict__ inf, uint32_t n, int c, uint32_t mul,
                                                 typename C::Acc* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typename C::Acc a = inf[i] ? C::zero() : C::from_aff(in[i], false);
    if (!inf[i] && mul > 1) {  // double-and-add; k P != +-P for 1 < k < r, so no exceptional add
        const typename C::Aff p = in[i];
        for (int b = 30 - __builtin_clz(mul); b >= 0; b--) {
            a = C::dbl(a);
            if ((mul >> b) & 1) a = C::madd(a, p, false);
        }
    }
    for (int k = 0; k < c; k++) a = C::dbl(a);
    out[i] = a;
}

// Shared-window copies of a GLV table (Table::win): for w < W, 2^(c w) P_i at [w][i] and
// 2^(c w) phi(P_i) at [w][n + i], in radix-2^29 limbs. A GLV MSM over the whole table then sends every
// window's digits to one set of 2^(c-1) buckets -- the same mixed adds, but one bucket reduction
// instead of W and no doublings in the host fold. 2 W n points (1.6 GB at n = 2^20, c = 16),
// built once per table and window size: W - 1 steps of c doublings + a batch normalisation.
// mul > 1: radix B = mul 2^c (the radix-B shared windows): the copy of window w holds B^w P.
// pair: the radix shared-window copies in the pair layout (SW29::AffP: one aligned 128-B record per
// signed copy, 3.76 GB at 2^20 instead of 2.47). Default on: the 2^20 accumulate 2.15 ms against
// 2.17-2.38 with the (x, y, -y) records (profiles/r04/pair_ab.txt)
template <class C>
int win_tables(vc_ctx* ctx, Table* t, int c, int W, int ts, uint32_t mul, bool pair) {
    using Aff = typename C::Aff;
    using Acc = typename C::Acc;
    if (t->win_ok && t->win_c == c && t->win_W == W && t->win_ts == ts && t->win_m == (int)mul &&
        t->win_pair == (pair ? 1 : 0))
        return VC_OK;
    const size_t n = t->n;
    t->win_ok = 0;
    using FA = typename Fast29<C>::type::AffN;  // signed limb form (k_to_limbs_n)
    using FP = typename Fast29<C>::type::AffP;  // pair layout (k_to_limbs_p)
    // radix-2^29 limbs, not the packed-29 form (unpacking cost the accumulate ~84 of 5,044
    // instructions per add, the limb form 16 B more per gather); the limb form holds x, y and -y
    // (168 B) so the accumulate never negates
    t->win_pair = pair ? 1 : 0;
    VK_TRY(t->win.ensure((size_t)W * 2 * n * (pair ? 2 * sizeof(FP) : sizeof(FA))));
    Table cur;  // 2^(c w) P (affine, Montgomery): normalised by table_from_acc (fb_table.hip)
    DevBuf nxt, acc;
    VK_TRY(nxt.ensure(n * sizeof(Aff)));
    VK_TRY(acc.ensure(n * sizeof(Acc)));
    FA* win = t->win.as<FA>();
    const unsigned g = (unsigned)((n + 255) / 256);
    for (int w = 0; w < W; w++) {
        const Aff* src = t->bases.as<Aff>();
        if (w > 0) {
            // the top window's copy is 2^(c w - ts) P (its digits are scaled by 2^ts, GlvDigits)
            VK_LAUNCH(ctx, "win_next", (k_win_next<C>), g, 256, 0, w == 1 ? t->bases.as<Aff>() : cur.bases.as<Aff>(),
                      t->inf.as<uint8_t>(), (uint32_t)n, w == W - 1 ? c - ts : c, mul, acc.as<Acc>());
            VK_TRY(table_from_acc(ctx, &cur, acc.p, n));
            src = cur.bases.as<Aff>();
        }
        VK_LAUNCH(ctx, "glv_phi", (k_glv_phi<C>), g, 256, 0, src, (uint32_t)n, bls_fq_mont(GLV_BETA), nxt.as<Aff>());
        if (pair) {
            FP* wp = t->win.as<FP>();
            VK_LAUNCH(ctx, "to_limbs", (k_to_limbs_p<C>), g, 256, 0, src, n, wp + 2 * ((size_t)w * 2 * n));
            VK_LAUNCH(ctx, "to_limbs", (k_to_limbs_p<C>), g, 256, 0, nxt.as<Aff>(), n, wp + 2 * ((size_t)w * 2 * n + n));
        } else {
            VK_LAUNCH(ctx, "to_limbs", (k_to_limbs_n<C>), g, 256, 0, src, n, win + (size_t)w * 2 * n);
            VK_LAUNCH(ctx, "to_limbs", (k_to_limbs_n<C>), g, 256, 0, nxt.as<Aff>(), n, win + (size_t)w * 2 * n + n);
        }
    }
    VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));  // before the staging buffers are freed
    t->win_ok = 1;
    t->win_c = c;
    t->win_W = W;
    t->win_ts = ts;
    t->win_m = (int)mul;
    return VC_OK;
}

template int fast_tables<BN254G1>(vc_ctx*, Table*, bool);
template int fast_tables<BLS381G1>(vc_ctx*, Table*, bool);
template int fast_tables<Bandersnatch>(vc_ctx*, Table*, bool);
template int win_tables<BLS381G1>(vc_ctx*, Table*, int, int, int, uint32_t, bool);  // (GLV tables only)
}  // namespace vk

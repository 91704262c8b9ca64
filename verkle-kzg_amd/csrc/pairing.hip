// Batched KZG verification on the GPU (vc_kzg_verify_many): one lane per opening, one verdict
// per opening, one text for both curves (C: a curve of kzg_curves.hpp; the key's curve selects
// the instantiation). A lane validates its inputs (Fr values below r, G1 coordinates below p, on
// the curve and, on BLS12-381, in the subgroup of order r), maps its point (omega^point below the
// domain size), forms A = y G - C - p pi, runs the two-pairing Miller loop over the key's tabulated
// lines on (pi, [s]_2) and (A, H) with one accumulator, the final exponentiation, and writes one
// byte. The arithmetic is pairing_common.hpp with pairing.hpp / pairing_bls.hpp, the text the host
// verifier runs (pairing_host.cpp). A key's tables stay in the context (22.5 KB for BN254, 26 KB
// for BLS12-381) until the context is destroyed.
//
// Shape: an Fq12 is 96 or 144 words and the loops hold several, so the kernel is declared for one
// wave per SIMD (the whole unified VGPR + AGPR file for a lane) rather than squeezed to fit two.
// The tower's multiplies are out-of-line functions with one copy each per curve and the loops are
// rolled, so the code stays small; nothing recurses, and the stack is static.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "pairing_internal.hpp"
#include "scheme_internal.hpp"

namespace vk {

using namespace ate;

template <class C>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_kzg_verify(
    const uint32_t* __restrict__ com_xy, const uint8_t* __restrict__ com_inf, const uint32_t* __restrict__ proof_xy,
    const uint8_t* __restrict__ proof_inf, const uint32_t* __restrict__ y, const uint32_t* __restrict__ points,
    fe<typename C::Fr> omega, uint64_t size, const LineCoefT<typename C::Fq>* __restrict__ lines, size_t n,
    uint8_t* __restrict__ out) {
    using Fq = typename C::Fq;
    using Fr = typename C::Fr;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t res = 0;
    uint32_t yw[8], pt[8];
    for (int k = 0; k < 8; k++) {
        yw[k] = y[8 * i + k];
        pt[k] = points[8 * i + k];
    }
    if (words_below_modulus<Fr>(yw) && words_below_modulus<Fr>(pt)) {
        const bool c_inf = com_inf[i] != 0, pi_inf = proof_inf[i] != 0;
        SWAff<Fq> Cm{fe_zero<Fq>(), fe_zero<Fq>()}, pi = Cm;
        uint32_t w[C::PW];
        bool ok = true;
        if (!c_inf) {
            for (int k = 0; k < C::PW; k++) w[k] = com_xy[C::PW * i + k];
            ok = g1_load(w, Cm);
        }
        if (ok && !pi_inf) {
            for (int k = 0; k < C::PW; k++) w[k] = proof_xy[C::PW * i + k];
            ok = g1_load(w, pi);
        }
        if (ok) {
            uint32_t pw[8];
            kzg_eval_point(omega, size, pt, pw);
            res = kzg_check(Cm, c_inf, pi, pi_inf, yw, pw, lines, lines + C::PC::ATE_LINES) ? 1 : 0;
        }
    }
    out[i] = res;
}

namespace {
// the key's line tables in device memory, uploaded once per (context, key uid)
template <class C>
int cached_lines(vc_ctx* ctx, const KzgKey<C>& key, const LineCoefT<typename C::Fq>** out) {
    auto& slot = ctx->dcache["kzg_vk:" + std::to_string(key.uid)];
    if (!slot) {
        auto b = std::make_unique<DevBuf>();
        VK_TRY(b->ensure(sizeof key.lines));
        VK_CHECK_HIP(hipMemcpyAsync(b->p, key.lines, sizeof key.lines, hipMemcpyHostToDevice, ctx->stream));
        VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        slot = std::move(b);
    }
    *out = slot->template as<LineCoefT<typename C::Fq>>();
    return VC_OK;
}

template <class C>
int verify_many(vc_ctx* ctx, const KzgKey<C>& key, size_t n, const uint64_t* com_xy, const uint8_t* com_inf,
                const uint64_t* points, const uint64_t* proof_xy, const uint8_t* proof_inf, const uint64_t* y,
                uint8_t* results) {
    if (!ctx || ctx->curve != C::CURVE) return VC_E_INVALID;
    if (n && (!com_xy || !com_inf || !points || !proof_xy || !proof_inf || !y || !results)) return VC_E_INVALID;
    Guard g(ctx);
    if (n == 0) return VC_OK;
    const LineCoefT<typename C::Fq>* d_lines = nullptr;
    VK_TRY(cached_lines<C>(ctx, key, &d_lines));
    constexpr size_t PB = C::PW * 4;  // bytes of a G1 point
    DevBuf dcom(ctx), dproof(ctx), dy(ctx), dp(ctx), dflags(ctx), dout(ctx);  // dp: the points
    VK_TRY(dcom.ensure(n * PB));
    VK_TRY(dproof.ensure(n * PB));
    VK_TRY(dy.ensure(n * 32));
    VK_TRY(dp.ensure(n * 32));
    VK_TRY(dflags.ensure(2 * n));
    VK_TRY(dout.ensure(n));
    uint8_t* fl = dflags.as<uint8_t>();
    hipStream_t st = ctx->stream;
    VK_CHECK_HIP(hipMemcpyAsync(dcom.p, com_xy, n * PB, hipMemcpyHostToDevice, st));
    VK_CHECK_HIP(hipMemcpyAsync(dproof.p, proof_xy, n * PB, hipMemcpyHostToDevice, st));
    VK_CHECK_HIP(hipMemcpyAsync(dy.p, y, n * 32, hipMemcpyHostToDevice, st));
    VK_CHECK_HIP(hipMemcpyAsync(dp.p, points, n * 32, hipMemcpyHostToDevice, st));
    VK_CHECK_HIP(hipMemcpyAsync(fl, com_inf, n, hipMemcpyHostToDevice, st));
    VK_CHECK_HIP(hipMemcpyAsync(fl + n, proof_inf, n, hipMemcpyHostToDevice, st));
    VK_LAUNCH(ctx, C::VERIFY_LAUNCH, k_kzg_verify<C>, (n + 63) / 64, 64, 0, dcom.as<uint32_t>(), fl,
              dproof.as<uint32_t>(), fl + n, dy.as<uint32_t>(), dp.as<uint32_t>(), key.omega, (uint64_t)key.size, d_lines,
              n, dout.as<uint8_t>());
    VK_CHECK_HIP(hipMemcpyAsync(results, dout.p, n, hipMemcpyDeviceToHost, st));
    VK_CHECK_HIP(hipStreamSynchronize(st));
    return VC_OK;
}
}  // namespace

// the kernel alone over device arrays (scheme_internal.hpp): the multiproof many-verifier's claims
int kzg_verify_dev(vc_ctx* ctx, const vc_kzg_vk* vk, size_t n, const uint32_t* d_com, const uint8_t* d_cinf,
                   const uint32_t* d_points, const uint32_t* d_proof, const uint8_t* d_pinf, const uint32_t* d_y,
                   uint8_t* d_out) {
    using C = BN254Kzg;
    if (!ctx || !vk || vk->curve != VC_CURVE_BN254 || ctx->curve != VC_CURVE_BN254) return VC_E_INVALID;
    if (n == 0) return VC_OK;
    const KzgKey<C>& key = kzg_key<C>(vk);
    const LineCoefT<C::Fq>* d_lines = nullptr;
    VK_TRY(cached_lines<C>(ctx, key, &d_lines));
    VK_LAUNCH(ctx, C::VERIFY_LAUNCH, k_kzg_verify<C>, (n + 63) / 64, 64, 0, d_com, d_cinf, d_proof, d_pinf, d_y, d_points,
              key.omega, (uint64_t)key.size, d_lines, n, d_out);
    return VC_OK;
}

}  // namespace vk

using namespace vk;

extern "C" int vc_kzg_verify_many(vc_ctx* ctx, const vc_kzg_vk* vk, size_t n, const uint64_t* com_xy,
                                  const uint8_t* com_inf, const uint64_t* points, const uint64_t* proof_xy,
                                  const uint8_t* proof_inf, const uint64_t* y, uint8_t* results) {
    if (!vk) return VC_E_INVALID;
    if (vk->curve == VC_CURVE_BLS12_381)  // the key's curve decides
        return verify_many(ctx, kzg_key<BLS381Kzg>(vk), n, com_xy, com_inf, points, proof_xy, proof_inf, y, results);
    return verify_many(ctx, kzg_key<BN254Kzg>(vk), n, com_xy, com_inf, points, proof_xy, proof_inf, y, results);
}

// KZG batch verification for a BLS12-381 key (vc_kzg_batch_fold / vc_kzg_verify_batch dispatch
// here on the key's curve): n openings, one combined verdict. The shape is kzg_batch.hip's. The
// entries fold with the weights rho^i into two points (csrc/kzg_batch_bls.hpp) and one two-pairing
// check follows on the host (blsk::pair_check). Per chunk of at most 2^20 entries the device path is
//   upload  C | pi, y | point and the identity flags, as vc_kzg_verify_many uploads them;
//   prep    k_kzg_bls_batch_prep, a lane per entry: validates the entry (the subgroup test
//           included), writes its two points into the context's scratch table
//           [C_0 .. C_{n-1} | pi_0 .. pi_{n-1}] (Montgomery affine: the kernel is the table's fill)
//           and the scalar rows [rho^i | rho^i p_i] beside it, and folds rho^i y_i over the wave and
//           the block;
//   MSMs    msm_run over the second half with the first half's rows (P1's part) and over all 2n
//           points (the variable part of P2).
// New ground against BN254: at 4,096 points and more the BLS12-381 MSM splits its scalars by the
// GLV endomorphism and reads copies derived from the table (the packed copies and phi's, the
// subgroup verdict). The scratch table is refilled on every chunk, and every refill goes through
// bases_reserve -> reserve_t, which drops all of that state (subgroup = -1, fast_ok = phi_ok =
// win_ok = 0), so no derived copy outlives the bases it was made from. The prep kernel has
// validated the subgroup of every point it writes and writes the identity for a malformed entry,
// so the MSM's own subgroup check over the table passes and the GLV route is taken.
// A malformed entry sets the call's bad flag; the flag is read before the MSMs, which a malformed
// batch skips. The rows are positive and the variable part is subtracted on the host:
// P2 = (sum rho^i y_i) G - var. The chunks' accumulators and Fr partials are added on the host, the
// weights continue across chunks (`first`), so the workspace is sized by the chunk.
// The host path (ctx == NULL) runs kzg_batch_bls.hpp's fold_range over the host pool, a slice per
// thread: the oracle check of the fold on a machine without a GPU, not a product path.
#include <hip/hip_runtime.h>
#include <sys/random.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "ec29.hpp"
#include "host/pool.hpp"
#include "kzg_batch_bls.hpp"
#include "pairing_bls_internal.hpp"
#include "pairing_internal.hpp"

namespace vk {

// scheme_host.cpp
void expand_message_xmd(const uint8_t* msg, size_t n, const uint8_t* dst, size_t dlen, size_t out_len, uint8_t* out);

using namespace kzgb_bls;

constexpr uint32_t KBB_BLOCK = 256;  // lanes per block of the prep kernel (four waves)
constexpr size_t KBB_CHUNK_MAX = size_t(1) << 20;
constexpr int PW = 2 * NL;  // 32-bit words of a G1 point in the ABI

// Entry i < n of the chunk is entry first + i of the call. bases / inf: the scratch table, 2n
// entries; rows: 2n Montgomery scalars; part: one Montgomery Fr per block; bad: the call's flag
// (zeroed by the host; every malformed lane stores the same 1).
__global__ __launch_bounds__(KBB_BLOCK) void k_kzg_bls_batch_prep(
    const uint32_t* __restrict__ com_xy, const uint8_t* __restrict__ com_inf, const uint32_t* __restrict__ proof_xy,
    const uint8_t* __restrict__ proof_inf, const uint32_t* __restrict__ y, const uint32_t* __restrict__ points, FrE rho,
    FrE omega, uint64_t size, uint64_t first, uint32_t n, G1P* __restrict__ bases, uint8_t* __restrict__ inf,
    uint32_t* __restrict__ rows, uint32_t* __restrict__ part, uint32_t* __restrict__ bad) {
    __shared__ FrE wave_sum[KBB_BLOCK / 64];
    const uint32_t i = blockIdx.x * KBB_BLOCK + threadIdx.x;
    FrE wy = fe_zero<BLS381Fr>();
    if (i < n) {
        uint32_t yw[8], pt[8];
        for (int k = 0; k < 8; k++) {
            yw[k] = y[8 * (size_t)i + k];
            pt[k] = points[8 * (size_t)i + k];
        }
        bool c_inf = com_inf[i] != 0, pi_inf = proof_inf[i] != 0;
        G1P C, pi;
        FrE w = fe_zero<BLS381Fr>(), wp = w;
        if (entry_check(com_xy + PW * (size_t)i, c_inf, proof_xy + PW * (size_t)i, pi_inf, yw, pt, C, pi)) {
            w = pow_index(rho, first + i);
            entry_scalars(w, omega, size, yw, pt, wp, wy);
        } else {
            *bad = 1u;
            C = G1P{fe_zero<BLS381Fq>(), fe_zero<BLS381Fq>()};
            pi = C;
            c_inf = pi_inf = true;
        }
        bases[i] = C;
        bases[(size_t)n + i] = pi;
        inf[i] = c_inf ? 1 : 0;
        inf[(size_t)n + i] = pi_inf ? 1 : 0;
        for (int k = 0; k < 8; k++) {
            rows[8 * (size_t)i + k] = w.v[k];
            rows[8 * ((size_t)n + i) + k] = wp.v[k];
        }
    }
    // sum rho^i y_i: over the wave by shuffles, over the block's waves through LDS
    for (uint32_t m = 1; m < 64; m <<= 1) wy = fe_add<BLS381Fr>(wy, shfl_xor_pod(wy, m));
    if ((threadIdx.x & 63u) == 0) wave_sum[threadIdx.x >> 6] = wy;
    __syncthreads();
    if (threadIdx.x == 0) {
        FrE s = wave_sum[0];
        for (uint32_t k = 1; k < KBB_BLOCK / 64; k++) s = fe_add<BLS381Fr>(s, wave_sum[k]);
        for (int k = 0; k < 8; k++) part[8 * (size_t)blockIdx.x + k] = s.v[k];
    }
}

namespace {
const uint32_t* w32(const uint64_t* p) { return reinterpret_cast<const uint32_t*>(p); }

struct Batch {
    const vc_kzg_vk* vk;
    size_t n;
    const uint64_t *com_xy, *points, *proof_xy, *y;
    const uint8_t *com_inf, *proof_inf;
};

// the host pool, a contiguous slice per thread, the slices' sums added at the end
int fold_host(const Batch& b, const FrE& rho, Sums* total, bool* malformed) {
    HostPool& pool = host_pool();
    const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>(pool.size(), b.n));
    std::vector<Sums> part(T, sums_zero());
    std::vector<uint8_t> ok(T, 1);
    pool.run([&](unsigned k) {
        if (k >= T) return;
        ok[k] = fold_range(b.n * k / T, b.n * (k + 1) / T, w32(b.com_xy), b.com_inf, w32(b.points), w32(b.proof_xy),
                           b.proof_inf, w32(b.y), rho, b.vk->bls->omega, b.vk->size, part[k])
                    ? 1
                    : 0;
    });
    *total = sums_zero();
    *malformed = false;
    for (unsigned k = 0; k < T; k++) {
        if (!ok[k]) *malformed = true;
        else *total = sums_add(*total, part[k]);
    }
    return VC_OK;
}

int fold_device(vc_ctx* ctx, const Batch& b, const FrE& rho, Sums* total, bool* malformed) {
    size_t chunk = KBB_CHUNK_MAX;
    // VKZG_KZG_BATCH_CHUNK (read per call): a test forces small chunks
    if (const char* e = getenv("VKZG_KZG_BATCH_CHUNK"))
        if (atol(e) > 0) chunk = std::min<size_t>((size_t)atol(e), KBB_CHUNK_MAX);
    chunk = std::min(chunk, b.n);
    const size_t max_blocks = (chunk + KBB_BLOCK - 1) / KBB_BLOCK;
    constexpr size_t PB = PW * 4;  // bytes of a G1 point
    DevBuf d_pts(ctx), d_fr(ctx), d_flags(ctx), d_rows(ctx), d_part(ctx);
    VK_TRY(d_pts.ensure(chunk * 2 * PB));        // C | pi
    VK_TRY(d_fr.ensure(chunk * 64));             // y | point
    VK_TRY(d_flags.ensure(chunk * 2));           // identity flags of C | pi
    VK_TRY(d_rows.ensure(chunk * 64));           // rho^i | rho^i p_i
    VK_TRY(d_part.ensure(max_blocks * 32 + 4));  // the blocks' Fr partials, then the bad flag
    hipStream_t st = ctx->stream;
    uint32_t* d_com = d_pts.as<uint32_t>();
    uint32_t* d_proof = d_com + chunk * PW;
    uint32_t* d_y = d_fr.as<uint32_t>();
    uint32_t* d_point = d_y + chunk * 8;
    uint8_t* d_cinf = d_flags.as<uint8_t>();
    uint8_t* d_pinf = d_cinf + chunk;
    uint32_t* d_bad = d_part.as<uint32_t>() + max_blocks * 8;
    std::vector<uint32_t> part(max_blocks * 8 + 1);
    Table* t = &ctx->scratch;
    *total = sums_zero();
    *malformed = false;
    for (size_t lo = 0; lo < b.n; lo += chunk) {
        const size_t cnt = std::min(chunk, b.n - lo), blocks = (cnt + KBB_BLOCK - 1) / KBB_BLOCK;
        VK_CHECK_HIP(hipMemcpyAsync(d_com, b.com_xy + NL * lo, cnt * PB, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_proof, b.proof_xy + NL * lo, cnt * PB, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_y, b.y + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_point, b.points + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_cinf, b.com_inf + lo, cnt, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_pinf, b.proof_inf + lo, cnt, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemsetAsync(d_bad, 0, 4, st));
        // the refill: drops everything derived from the previous chunk's (or call's) bases
        VK_TRY(bases_reserve(ctx, t, 2 * cnt));
        VK_LAUNCH(ctx, "kzg_bls_batch_prep", k_kzg_bls_batch_prep, blocks, KBB_BLOCK, 0, d_com, d_cinf, d_proof, d_pinf,
                  d_y, d_point, rho, b.vk->bls->omega, (uint64_t)b.vk->size, (uint64_t)lo, (uint32_t)cnt,
                  t->bases.as<G1P>(), t->inf.as<uint8_t>(), d_rows.as<uint32_t>(), d_part.as<uint32_t>(), d_bad);
        // the partials and the flag: the blocks' words, then (not adjacent when blocks < max_blocks) the flag
        VK_CHECK_HIP(hipMemcpyAsync(part.data(), d_part.p, blocks * 32, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipMemcpyAsync(&part[max_blocks * 8], d_bad, 4, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipStreamSynchronize(st));
        if (part[max_blocks * 8]) {
            *malformed = true;
            return VC_OK;
        }
        Sums s = sums_zero();
        for (size_t k = 0; k < blocks; k++) s.sy = fe_add<BLS381Fr>(s.sy, fr_words(&part[8 * k]));
        VK_TRY(msm_run(ctx, t, cnt, d_rows.p, cnt, 1, reinterpret_cast<uint32_t*>(&s.p1)));
        VK_TRY(msm_run(ctx, t, 0, d_rows.p, 2 * cnt, 1, reinterpret_cast<uint32_t*>(&s.var)));
        *total = sums_add(*total, s);
    }
    return VC_OK;
}

// rho Montgomery
int fold_impl(vc_ctx* ctx, const Batch& b, const FrE& rho, G1A* P1, G1A* P2, bool* malformed) {
    Sums total;
    if (ctx) {
        Guard g(ctx);
        VK_TRY(fold_device(ctx, b, rho, &total, malformed));
    } else {
        VK_TRY(fold_host(b, rho, &total, malformed));
    }
    if (!*malformed) fold_finish(total, *P1, *P2);
    return VC_OK;
}
bool args_ok(vc_ctx* ctx, const Batch& b) {
    if (!b.vk || !b.vk->bls || (ctx && ctx->curve != VC_CURVE_BLS12_381)) return false;
    return b.n == 0 || (b.com_xy && b.com_inf && b.points && b.proof_xy && b.proof_inf && b.y);
}
FrE rho_mont(const uint64_t* rho_fr) { return fe_to_mont<BLS381Fr>(fr_words(w32(rho_fr))); }
}  // namespace

int blsk::batch_challenge(const uint8_t seed[32], uint64_t* rho_fr) {
    if (!seed || !rho_fr) return VC_E_INVALID;
    static const char dst[] = "vkzg-kzg-batch";
    // DefaultFieldHasher<Sha256, 128> for a 255-bit modulus: ceil((255 + 128) / 8) = 48 bytes, as for BN254
    uint8_t u[48];
    expand_message_xmd(seed, 32, reinterpret_cast<const uint8_t*>(dst), sizeof dst - 1, sizeof u, u);
    mont_to_canon<BLS381Fr>(fe_from_be_bytes_mod<BLS381Fr>(u, sizeof u), rho_fr);
    return VC_OK;
}

int blsk::batch_fold(vc_ctx* ctx, const vc_kzg_vk* vk, size_t n, const uint64_t* com_xy, const uint8_t* com_inf,
                     const uint64_t* points, const uint64_t* proof_xy, const uint8_t* proof_inf, const uint64_t* y,
                     const uint64_t* rho_fr, uint64_t* p1_xy, uint8_t* p1_inf, uint64_t* p2_xy, uint8_t* p2_inf,
                     int* malformed) {
    const Batch b{vk, n, com_xy, points, proof_xy, y, com_inf, proof_inf};
    if (!args_ok(ctx, b) || !rho_fr || !p1_xy || !p1_inf || !p2_xy || !p2_inf || !malformed) return VC_E_INVALID;
    if (!bls::words_below_modulus<BLS381Fr>(w32(rho_fr))) return VC_E_INVALID;
    G1A P[2] = {BLS381G1::zero(), BLS381G1::zero()};  // (n = 0: both sums are empty)
    bool bad = false;
    if (n) VK_TRY(fold_impl(ctx, b, rho_mont(rho_fr), &P[0], &P[1], &bad));
    *malformed = bad ? 1 : 0;
    if (bad) return VC_OK;
    uint64_t xy[2 * NL];
    uint8_t inf[2];
    VK_TRY(acc_to_affine_batch(VC_CURVE_BLS12_381, reinterpret_cast<const uint32_t*>(P), 2, xy, inf));
    memcpy(p1_xy, xy, NL * 8);
    memcpy(p2_xy, xy + NL, NL * 8);
    *p1_inf = inf[0];
    *p2_inf = inf[1];
    return VC_OK;
}

int blsk::verify_batch(vc_ctx* ctx, const vc_kzg_vk* vk, size_t n, const uint64_t* com_xy, const uint8_t* com_inf,
                       const uint64_t* points, const uint64_t* proof_xy, const uint8_t* proof_inf, const uint64_t* y,
                       const uint8_t* seed32, int* result, uint8_t* results) {
    const Batch b{vk, n, com_xy, points, proof_xy, y, com_inf, proof_inf};
    if (!args_ok(ctx, b) || !result || (results && !ctx)) return VC_E_INVALID;
    *result = 1;
    if (n == 0) return VC_OK;
    uint8_t seed[32];
    if (seed32) {
        memcpy(seed, seed32, 32);
    } else {
        for (size_t got = 0; got < sizeof seed;) {
            const ssize_t r = getrandom(seed + got, sizeof seed - got, 0);
            if (r < 0) return VC_E_INVALID;
            got += (size_t)r;
        }
    }
    uint64_t rho_c[4];
    VK_TRY(batch_challenge(seed, rho_c));
    G1A P1, P2;
    bool bad = false;
    VK_TRY(fold_impl(ctx, b, rho_mont(rho_c), &P1, &P2, &bad));
    const bool ok = !bad && pair_check(vk, P1, P2);
    *result = ok ? 1 : 0;
    if (!results) return VC_OK;
    if (ok) {
        memset(results, 1, n);
        return VC_OK;
    }
    return verify_many(ctx, vk, n, com_xy, com_inf, points, proof_xy, proof_inf, y, results);
}

}  // namespace vk

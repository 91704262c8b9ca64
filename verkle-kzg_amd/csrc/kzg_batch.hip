// KZG batch verification (vc_kzg_verify_batch): n openings, one combined verdict, one text for
// both curves (C: a curve of kzg_curves.hpp; the key's curve selects the instantiation). The
// entries fold with the weights rho^i into two points (csrc/kzg_batch.hpp) and one two-pairing
// check follows on the host (kzgb::pair_check over the key's tables). Per chunk of at most 2^20
// entries the device path is
//   upload  C | pi, y | point and the identity flags, as vc_kzg_verify_many uploads them;
//   prep    k_kzg_batch_prep, a lane per entry: validates the entry (on BLS12-381 the subgroup
//           test included), writes its two points into the context's scratch table
//           [C_0 .. C_{n-1} | pi_0 .. pi_{n-1}] (Montgomery affine: the kernel is the table's fill,
//           so no entry ever reaches bases_fill's check) and the scalar rows [rho^i | rho^i p_i]
//           beside it, and folds rho^i y_i over the wave and the block;
//   MSMs    msm_run over the second half with the first half's rows (P1's part) and over all 2n
//           points (the variable part of P2).
// The refill. An MSM may read copies derived from its table: at 4,096 points and more the
// BLS12-381 MSM splits its scalars by the GLV endomorphism and reads the packed copies, phi's and
// the subgroup verdict. The scratch table is refilled on every chunk, and every refill goes through
// bases_reserve -> reserve_t, which drops all of that state (subgroup = -1, fast_ok = phi_ok =
// win_ok = 0), so no derived copy outlives the bases it was made from: the condition holds for any
// curve with derived copies. The prep kernel has validated the subgroup of every point it writes
// and writes the identity for a malformed entry, so the MSM's own subgroup check over the table
// passes and the GLV route is taken.
// A malformed entry sets the call's bad flag and enters the table as the identity with zero rows;
// the flag is read before the MSMs, which a malformed batch skips. The rows are positive and the
// variable part is subtracted on the host: P2 = (sum rho^i y_i) G - var. The chunks' accumulators
// and Fr partials are added on the host, the weights continue across chunks (`first`), so the
// workspace is sized by the chunk.
// The host path (ctx == NULL) runs kzg_batch.hpp's fold_range over the host pool, a slice per
// thread: the oracle check of the fold on a machine without a GPU, not a product path.
#include <hip/hip_runtime.h>
#include <sys/random.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "ec29.hpp"
#include "host/pool.hpp"
#include "kzg_batch.hpp"
#include "pairing_internal.hpp"
#include "scheme_internal.hpp"

namespace vk {

using namespace kzgb;

constexpr uint32_t KB_BLOCK = 256;  // lanes per block of the prep kernel (four waves)
constexpr size_t KB_CHUNK_MAX = size_t(1) << 20;

// Entry i < n of the chunk is entry first + i of the call. bases / inf: the scratch table, 2n
// entries; rows: 2n Montgomery scalars; part: one Montgomery Fr per block; bad: the call's flag
// (zeroed by the host; every malformed lane stores the same 1).
template <class C>
__global__ __launch_bounds__(KB_BLOCK) void k_kzg_batch_prep(
    const uint32_t* __restrict__ com_xy, const uint8_t* __restrict__ com_inf, const uint32_t* __restrict__ proof_xy,
    const uint8_t* __restrict__ proof_inf, const uint32_t* __restrict__ y, const uint32_t* __restrict__ points,
    FrOf<C> rho, FrOf<C> omega, uint64_t size, uint64_t first, uint32_t n, G1POf<C>* __restrict__ bases,
    uint8_t* __restrict__ inf, uint32_t* __restrict__ rows, uint32_t* __restrict__ part, uint32_t* __restrict__ bad) {
    using Fr = typename C::Fr;
    __shared__ FrOf<C> wave_sum[KB_BLOCK / 64];
    const uint32_t i = blockIdx.x * KB_BLOCK + threadIdx.x;
    FrOf<C> wy = fe_zero<Fr>();
    if (i < n) {
        uint32_t yw[8], pt[8];
        for (int k = 0; k < 8; k++) {
            yw[k] = y[8 * (size_t)i + k];
            pt[k] = points[8 * (size_t)i + k];
        }
        bool c_inf = com_inf[i] != 0, pi_inf = proof_inf[i] != 0;
        G1POf<C> Cm, pi;
        FrOf<C> w = fe_zero<Fr>(), wp = w;
        if (entry_check<C>(com_xy + C::PW * (size_t)i, c_inf, proof_xy + C::PW * (size_t)i, pi_inf, yw, pt, Cm, pi)) {
            w = pow_index(rho, first + i);
            entry_scalars(w, omega, size, yw, pt, wp, wy);
        } else {
            *bad = 1u;
            Cm = G1POf<C>{fe_zero<typename C::Fq>(), fe_zero<typename C::Fq>()};
            pi = Cm;
            c_inf = pi_inf = true;
        }
        bases[i] = Cm;
        bases[(size_t)n + i] = pi;
        inf[i] = c_inf ? 1 : 0;
        inf[(size_t)n + i] = pi_inf ? 1 : 0;
        for (int k = 0; k < 8; k++) {
            rows[8 * (size_t)i + k] = w.v[k];
            rows[8 * ((size_t)n + i) + k] = wp.v[k];
        }
    }
    // sum rho^i y_i: over the wave by shuffles, over the block's waves through LDS
    for (uint32_t m = 1; m < 64; m <<= 1) wy = fe_add<Fr>(wy, shfl_xor_pod(wy, m));
    if ((threadIdx.x & 63u) == 0) wave_sum[threadIdx.x >> 6] = wy;
    __syncthreads();
    if (threadIdx.x == 0) {
        FrOf<C> s = wave_sum[0];
        for (uint32_t k = 1; k < KB_BLOCK / 64; k++) s = fe_add<Fr>(s, wave_sum[k]);
        for (int k = 0; k < 8; k++) part[8 * (size_t)blockIdx.x + k] = s.v[k];
    }
}

namespace {
const uint32_t* w32(const uint64_t* p) { return reinterpret_cast<const uint32_t*>(p); }

template <class C>
struct Batch {
    const KzgKey<C>* key;
    size_t n;
    const uint64_t *com_xy, *points, *proof_xy, *y;
    const uint8_t *com_inf, *proof_inf;
};
struct Laps {  // VKZG_HOST_TIMING: the device path's phases, us
    double upload = 0, prep = 0, msm = 0;
    size_t chunks = 0;
};

// the host pool, a contiguous slice per thread, the slices' sums added at the end
template <class C>
int fold_host(const Batch<C>& b, const FrOf<C>& rho, Sums<C>* total, bool* malformed) {
    HostPool& pool = host_pool();
    const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>(pool.size(), b.n));
    std::vector<Sums<C>> part(T, sums_zero<C>());
    std::vector<uint8_t> ok(T, 1);
    pool.run([&](unsigned k) {
        if (k >= T) return;
        ok[k] = fold_range<C>(b.n * k / T, b.n * (k + 1) / T, w32(b.com_xy), b.com_inf, w32(b.points), w32(b.proof_xy),
                              b.proof_inf, w32(b.y), rho, b.key->omega, b.key->size, part[k])
                    ? 1
                    : 0;
    });
    *total = sums_zero<C>();
    *malformed = false;
    for (unsigned k = 0; k < T; k++) {
        if (!ok[k]) *malformed = true;
        else *total = sums_add(*total, part[k]);
    }
    return VC_OK;
}

template <class C>
int fold_device(vc_ctx* ctx, const Batch<C>& b, const FrOf<C>& rho, Sums<C>* total, bool* malformed, Laps* laps) {
    using Fr = typename C::Fr;
    size_t chunk = KB_CHUNK_MAX;
    // VKZG_KZG_BATCH_CHUNK (read per call): a test forces small chunks
    if (const char* e = getenv("VKZG_KZG_BATCH_CHUNK"))
        if (atol(e) > 0) chunk = std::min<size_t>((size_t)atol(e), KB_CHUNK_MAX);
    chunk = std::min(chunk, b.n);
    const size_t max_blocks = (chunk + KB_BLOCK - 1) / KB_BLOCK;
    constexpr size_t PW = C::PW, PB = PW * 4;  // words and bytes of a G1 point
    const bool timing = host_timing();
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
    *total = sums_zero<C>();
    *malformed = false;
    for (size_t lo = 0; lo < b.n; lo += chunk) {
        const size_t cnt = std::min(chunk, b.n - lo), blocks = (cnt + KB_BLOCK - 1) / KB_BLOCK;
        const double c0 = timing ? clock_us() : 0.0;
        VK_CHECK_HIP(hipMemcpyAsync(d_com, w32(b.com_xy) + PW * lo, cnt * PB, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_proof, w32(b.proof_xy) + PW * lo, cnt * PB, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_y, b.y + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_point, b.points + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_cinf, b.com_inf + lo, cnt, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_pinf, b.proof_inf + lo, cnt, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemsetAsync(d_bad, 0, 4, st));
        // the refill: drops everything derived from the previous chunk's (or call's) bases
        VK_TRY(bases_reserve(ctx, t, 2 * cnt));
        double c1 = 0;
        if (timing) {
            VK_CHECK_HIP(hipStreamSynchronize(st));
            c1 = clock_us();
        }
        VK_LAUNCH(ctx, C::PREP_LAUNCH, k_kzg_batch_prep<C>, blocks, KB_BLOCK, 0, d_com, d_cinf, d_proof, d_pinf, d_y,
                  d_point, rho, b.key->omega, (uint64_t)b.key->size, (uint64_t)lo, (uint32_t)cnt,
                  t->bases.as<G1POf<C>>(), t->inf.as<uint8_t>(), d_rows.as<uint32_t>(), d_part.as<uint32_t>(), d_bad);
        // the partials and the flag: the blocks' words, then (not adjacent when blocks < max_blocks) the flag
        VK_CHECK_HIP(hipMemcpyAsync(part.data(), d_part.p, blocks * 32, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipMemcpyAsync(&part[max_blocks * 8], d_bad, 4, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipStreamSynchronize(st));
        const double c2 = timing ? clock_us() : 0.0;
        if (part[max_blocks * 8]) {
            *malformed = true;
            return VC_OK;
        }
        Sums<C> s = sums_zero<C>();
        for (size_t k = 0; k < blocks; k++) s.sy = fe_add<Fr>(s.sy, fr_words<Fr>(&part[8 * k]));
        VK_TRY(msm_run(ctx, t, cnt, d_rows.p, cnt, 1, reinterpret_cast<uint32_t*>(&s.p1)));
        VK_TRY(msm_run(ctx, t, 0, d_rows.p, 2 * cnt, 1, reinterpret_cast<uint32_t*>(&s.var)));
        *total = sums_add(*total, s);
        if (timing) {
            VK_CHECK_HIP(hipStreamSynchronize(st));
            laps->upload += c1 - c0, laps->prep += c2 - c1, laps->msm += clock_us() - c2;
        }
        laps->chunks++;
    }
    return VC_OK;
}

// rho Montgomery
template <class C>
int fold_impl(vc_ctx* ctx, const Batch<C>& b, const FrOf<C>& rho, G1AOf<C>* P1, G1AOf<C>* P2, bool* malformed,
              Laps* laps) {
    Sums<C> total;
    if (ctx) {
        Guard g(ctx);
        VK_TRY(fold_device(ctx, b, rho, &total, malformed, laps));
    } else {
        VK_TRY(fold_host(b, rho, &total, malformed));
    }
    if (!*malformed) fold_finish(total, *P1, *P2);
    return VC_OK;
}
// the argument checks shared by the fold and the verdict
template <class C>
bool args_ok(vc_ctx* ctx, const Batch<C>& b) {
    if (ctx && ctx->curve != C::CURVE) return false;
    return b.n == 0 || (b.com_xy && b.com_inf && b.points && b.proof_xy && b.proof_inf && b.y);
}

// hash_to_field(seed, dst = "vkzg-kzg-batch") in the curve's Fr, canonical words out
template <class C>
void batch_challenge(const uint8_t seed[32], uint64_t* rho_fr) {
    static const char dst[] = "vkzg-kzg-batch";
    mont_to_canon<typename C::Fr>(
        hash_to_fr<typename C::Fr>(seed, 32, reinterpret_cast<const uint8_t*>(dst), sizeof dst - 1), rho_fr);
}

template <class C>
int batch_fold(vc_ctx* ctx, const Batch<C>& b, const uint64_t* rho_fr, uint64_t* p1_xy, uint8_t* p1_inf,
               uint64_t* p2_xy, uint8_t* p2_inf, int* malformed) {
    using Fr = typename C::Fr;
    if (!args_ok(ctx, b) || !rho_fr || !p1_xy || !p1_inf || !p2_xy || !p2_inf || !malformed) return VC_E_INVALID;
    if (!ate::words_below_modulus<Fr>(w32(rho_fr))) return VC_E_INVALID;
    G1AOf<C> P[2] = {C::G1::zero(), C::G1::zero()};  // (n = 0: both sums are empty)
    bool bad = false;
    Laps laps;
    if (b.n) VK_TRY(fold_impl(ctx, b, canon_to_mont<Fr>(rho_fr), &P[0], &P[1], &bad, &laps));
    *malformed = bad ? 1 : 0;
    if (bad) return VC_OK;
    constexpr size_t NL = C::PW / 4;  // u64 words of a coordinate
    uint64_t xy[4 * NL];
    uint8_t inf[2];
    VK_TRY(acc_to_affine_batch(C::CURVE, reinterpret_cast<const uint32_t*>(P), 2, xy, inf));
    memcpy(p1_xy, xy, 2 * NL * 8);
    memcpy(p2_xy, xy + 2 * NL, 2 * NL * 8);
    *p1_inf = inf[0];
    *p2_inf = inf[1];
    return VC_OK;
}

template <class C>
int verify_batch(vc_ctx* ctx, const Batch<C>& b, const uint8_t* seed32, int* result, uint8_t* results) {
    if (!args_ok(ctx, b) || !result || (results && !ctx)) return VC_E_INVALID;
    *result = 1;
    if (b.n == 0) return VC_OK;
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
    batch_challenge<C>(seed, rho_c);
    const double c0 = host_timing() ? clock_us() : 0.0;
    G1AOf<C> P1, P2;
    bool bad = false;
    Laps laps;
    VK_TRY(fold_impl(ctx, b, canon_to_mont<typename C::Fr>(rho_c), &P1, &P2, &bad, &laps));
    const double c1 = host_timing() ? clock_us() : 0.0;
    const bool ok = !bad && pair_check(P1, P2, b.key->lines, b.key->lines + C::PC::ATE_LINES);
    if (host_timing())
        fprintf(stderr,
                "[kzg_verify_batch] n=%zu chunks=%zu: upload %.1f us, prep %.1f us, msm %.1f us, fold %.1f us, "
                "pairing %.1f us, call %.1f us\n",
                b.n, laps.chunks, laps.upload, laps.prep, laps.msm, c1 - c0, clock_us() - c1, clock_us() - c0);
    *result = ok ? 1 : 0;
    if (!results) return VC_OK;
    if (ok) {
        memset(results, 1, b.n);
        return VC_OK;
    }
    return vc_kzg_verify_many(ctx, b.key, b.n, b.com_xy, b.com_inf, b.points, b.proof_xy, b.proof_inf, b.y, results);
}

template <class C>
Batch<C> batch_of(const vc_kzg_vk* vk, size_t n, const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* points,
                  const uint64_t* proof_xy, const uint8_t* proof_inf, const uint64_t* y) {
    return Batch<C>{&kzg_key<C>(vk), n, com_xy, points, proof_xy, y, com_inf, proof_inf};
}
bool is_bls(const vc_kzg_vk* vk) { return vk->curve == VC_CURVE_BLS12_381; }  // the key's curve decides
}  // namespace

}  // namespace vk

using namespace vk;

extern "C" int vc_kzg_batch_challenge_curve(int curve, const uint8_t seed[32], uint64_t* rho_fr) {
    if (!seed || !rho_fr || (curve != VC_CURVE_BN254 && curve != VC_CURVE_BLS12_381)) return VC_E_INVALID;
    if (curve == VC_CURVE_BLS12_381) batch_challenge<BLS381Kzg>(seed, rho_fr);
    else batch_challenge<BN254Kzg>(seed, rho_fr);
    return VC_OK;
}

extern "C" int vc_kzg_batch_challenge(const uint8_t seed[32], uint64_t* rho_fr) {
    return vc_kzg_batch_challenge_curve(VC_CURVE_BN254, seed, rho_fr);
}

extern "C" int vc_kzg_batch_fold(vc_ctx* ctx, const vc_kzg_vk* vk, size_t n, const uint64_t* com_xy,
                                 const uint8_t* com_inf, const uint64_t* points, const uint64_t* proof_xy,
                                 const uint8_t* proof_inf, const uint64_t* y, const uint64_t* rho_fr, uint64_t* p1_xy,
                                 uint8_t* p1_inf, uint64_t* p2_xy, uint8_t* p2_inf, int* malformed) {
    if (!vk) return VC_E_INVALID;
    if (is_bls(vk))
        return batch_fold(ctx, batch_of<BLS381Kzg>(vk, n, com_xy, com_inf, points, proof_xy, proof_inf, y), rho_fr,
                          p1_xy, p1_inf, p2_xy, p2_inf, malformed);
    return batch_fold(ctx, batch_of<BN254Kzg>(vk, n, com_xy, com_inf, points, proof_xy, proof_inf, y), rho_fr, p1_xy,
                      p1_inf, p2_xy, p2_inf, malformed);
}

extern "C" int vc_kzg_verify_batch(vc_ctx* ctx, const vc_kzg_vk* vk, size_t n, const uint64_t* com_xy,
                                   const uint8_t* com_inf, const uint64_t* points, const uint64_t* proof_xy,
                                   const uint8_t* proof_inf, const uint64_t* y, const uint8_t* seed32, int* result,
                                   uint8_t* results) {
    if (!vk) return VC_E_INVALID;
    if (is_bls(vk))
        return verify_batch(ctx, batch_of<BLS381Kzg>(vk, n, com_xy, com_inf, points, proof_xy, proof_inf, y), seed32,
                            result, results);
    return verify_batch(ctx, batch_of<BN254Kzg>(vk, n, com_xy, com_inf, points, proof_xy, proof_inf, y), seed32,
                        result, results);
}

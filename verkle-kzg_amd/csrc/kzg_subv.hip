// KZG subvector batch verification (vc_kzg_verify_subvector_batch): n subvector proofs, one combined
// verdict, one text for both curves (C: a curve of kzg_curves.hpp; the key's curve selects the
// instantiation). The statement and the per-proof arithmetic are csrc/kzg_subv.hpp. The proofs fold
// with the weights rho^j into Kmax + 1 points of G1, and one multi-Miller loop over the key's own
// line tables with one final exponentiation follows on the host pool. Per chunk the device path is
//   upload  pi | C, the y, the index sets and the identity flags;
//   fold    k_kzg_subv_fold, a wave per run of 4 to 64 consecutive proofs: validates them (a
//           lane per proof; on BLS12-381 the subgroup test included) and writes their points into
//           the context's scratch table [pi_0 .. pi_{n-1} | C_0 .. C_{n-1}] (Montgomery affine: the
//           kernel is the table's fill, as k_kzg_batch_prep is), then proof by proof the
//           coefficients of Z_j in LDS, the scalar rows rho^j z_{j,t} and the wave's sums
//           a_t += rho^j a_{j,t}, which stay in LDS across the run; a partial vector per wave;
//   sum     k_kzg_subv_sum adds the waves' partials, a thread per t;
//   MSMs    msm_run over [pi | C] with row 0 = [rho^j z_{j,0} | -rho^j] and over the pi half with
//           row t for t = 1 .. Kmax of the chunk.
// The chunk. The rows are (Kmax + 2) cnt scalars; a chunk is sized so that they stay within
// SV_ROWS_MAX = 2^23 scalars (256 MiB), and never above 64 proofs for each of at most 2,048 waves
// (fewer waves where 2,048 partial vectors of Kmax values would pass 4 MiB). The
// refill rule is kzg_batch.hip's: every chunk goes through bases_reserve, which drops what an MSM
// derived from the previous bases. A malformed proof sets the call's bad flag and enters the table as the identity
// with zero rows; the flag is read before the MSMs, which a malformed batch skips. The chunks'
// accumulators and sums are added on the host, the weights continue across chunks (`first`).
// sum_t a_t [s^t]_1 is a joint double-and-add over the key's G1 powers on the host pool (at most K
// points: 0.4 ms at K = 64 against a table per (context, key) and one more launch chain).
// The host path (ctx == NULL) runs kzg_subv.hpp's coeffs_serial over the host pool, a slice of the
// proofs per thread: the oracle check of the fold on a machine without a GPU, not a product path.
#include <hip/hip_runtime.h>
#include <sys/random.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "ec29.hpp"
#include "host/pool.hpp"
#include "kzg_subv.hpp"
#include "pairing_internal.hpp"
#include "poly.hpp"
#include "scheme_internal.hpp"

namespace vk {

using namespace kzgv;

constexpr uint32_t SV_BLOCK = 64;  // one wave per block: its LDS rows are its own
constexpr size_t SV_ROWS_MAX = size_t(1) << 23;   // scalars of a chunk's rows
constexpr size_t SV_PART_MAX = size_t(1) << 17;   // values of a chunk's partials (4 MiB)
constexpr size_t SV_WAVES_MAX = 2048;
constexpr size_t SV_RUN_MIN = 4, SV_RUN_MAX = 64;  // proofs of a wave (a lane validates one: at most 64)

// The steps below read LDS rows that other lanes of this wave wrote. A wave's LDS operations
// complete in order; the release waits for them and the pair keeps the compiler from moving an access
// across: producers and consumers are lanes of one wave in one instruction stream.
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
template <class F>
__device__ __forceinline__ void store_fr(uint32_t* dst, const fe<F>& v) {
    for (int k = 0; k < 8; k++) dst[k] = v.v[k];
}

// Block b (one wave) takes proofs [b run, min(n, (b + 1) run)) of the chunk, run <= 64; proof j of
// the chunk is proof first + j of the call. off: n + 1 offsets into idx / y (8 words per y), every set of 1 ..
// kmax distinct indices below N (the host has checked). bases / inf: the scratch table, 2n entries.
// rows: row 0 is 2n Montgomery scalars at 0, row t >= 1 is n scalars at (t + 1) n. part: kmax values
// per block. bad: the call's flag (zeroed by the host; every malformed lane stores the same 1).
// LDS: z[kmax] | a[kmax], 64 kmax bytes.
template <class C>
__global__ __launch_bounds__(SV_BLOCK) void k_kzg_subv_fold(
    const uint32_t* __restrict__ com_xy, const uint8_t* __restrict__ com_inf, const uint32_t* __restrict__ proof_xy,
    const uint8_t* __restrict__ proof_inf, const uint32_t* __restrict__ y, const uint32_t* __restrict__ idx,
    const uint32_t* __restrict__ off, const FrOf<C>* __restrict__ pw, const FrOf<C>* __restrict__ inv1, uint32_t N,
    FrOf<C> rho, uint64_t first, uint32_t n, uint32_t run, uint32_t kmax, G1POf<C>* __restrict__ bases,
    uint8_t* __restrict__ inf, uint32_t* __restrict__ rows, uint32_t* __restrict__ part, uint32_t* __restrict__ bad) {
    using Fr = typename C::Fr;
    using FrE = FrOf<C>;
    extern __shared__ __attribute__((aligned(16))) unsigned char sv_smem[];
    FrE* z = reinterpret_cast<FrE*>(sv_smem);
    FrE* a = z + kmax;
    const uint32_t lane = threadIdx.x;
    const uint32_t lo = blockIdx.x * run, hi = min(n, lo + run);
    for (uint32_t t = lane; t < kmax; t += 64) a[t] = fe_zero<Fr>();
    wave_fence();
    FrE w = kzgb::pow_index(rho, first + lo);
    {
        // ---- the run's content, a lane per proof (run <= 64)
        const uint32_t g0 = lo, p = g0 + lane;
        bool ok = true;
        if (p < hi) {
            const uint32_t b0 = off[p], k = off[p + 1] - b0;
            bool c_inf = com_inf[p] != 0, pi_inf = proof_inf[p] != 0;
            G1POf<C> Cm, pi;
            ok = entry_check<C>(com_xy + C::PW * (size_t)p, c_inf, proof_xy + C::PW * (size_t)p, pi_inf,
                                y + 8 * (size_t)b0, k, Cm, pi);
            if (!ok) {
                *bad = 1u;
                Cm = G1POf<C>{fe_zero<typename C::Fq>(), fe_zero<typename C::Fq>()};
                pi = Cm;
                c_inf = pi_inf = true;
            }
            bases[p] = pi;
            bases[(size_t)n + p] = Cm;
            inf[p] = pi_inf ? 1 : 0;
            inf[(size_t)n + p] = c_inf ? 1 : 0;
        }
        const unsigned long long good = __ballot(ok);
        const uint32_t cntg = hi - g0;
        // ---- proof by proof, everything below uniform over the wave but the lane's t or i
#pragma unroll 1
        for (uint32_t q = 0; q < cntg; q++) {
            const uint32_t j = g0 + q;
            const uint32_t b0 = off[j], k = off[j + 1] - b0;
            const uint32_t* S = idx + b0;
            const bool live = (good >> q) & 1ull;
            if (live) {
#pragma unroll 1
                for (uint32_t i = 0; i < k; i++) {  // z <- z (X - w^S[i])
                    const FrE x = pw[S[i]];
#pragma unroll 1
                    for (uint32_t c = i >> 6;; c--) {
                        const uint32_t t = 64 * c + lane;
                        FrE v;
                        if (t <= i) v = z_step<Fr>(z, i, t, x);
                        wave_fence();  // every lane has read its neighbour's old z_{t-1}
                        if (t <= i) z[t] = v;
                        wave_fence();
                        if (!c) break;
                    }
                }
            }
            // ---- the rows' entries of this proof (a malformed one: zeros)
            for (uint32_t t = lane; t <= kmax; t += 64) {
                const FrE v = live ? row_scalar<Fr>(z, k, t, w) : fe_zero<Fr>();
                store_fr<Fr>(rows + 8 * ((t ? (size_t)(t + 1) * n : 0) + j), v);
            }
            if (lane == 0) store_fr<Fr>(rows + 8 * ((size_t)n + j), live ? fe_neg<Fr>(w) : fe_zero<Fr>());
            if (live) {
                uint32_t sum = 0;
                for (uint32_t t = lane; t < k; t += 64) sum += S[t];
                for (uint32_t s = 1; s < 64; s <<= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)s);
                const FrE wsum = kzgs::sub_wsum<Fr>(pw, N, sum);
#pragma unroll 1
                for (uint32_t ib = 0; ib < k; ib += 64) {  // 64 indices of the set, a lane each
                    const uint32_t i = ib + lane;
                    FrE x = fe_zero<Fr>(), u = x, b = x;
                    if (i < k) lane_weight<Fr>(S, k, pw, inv1, N, i, wsum, y + 8 * (size_t)(b0 + i), w, x, u);
#pragma unroll 1
                    for (uint32_t t = k; t-- > 0;) {
                        b = div_step<Fr>(z, k, t, x, b);
                        FrE s = fe_mul<Fr>(u, b);  // (u = 0 beyond the set)
                        for (uint32_t m = 1; m < 64; m <<= 1) s = fe_add<Fr>(s, shfl_xor_pod(s, m));
                        if (lane == 0) a[t] = fe_add<Fr>(a[t], s);
                    }
                }
                wave_fence();  // the next proof rewrites z
            }
            w = fe_mul<Fr>(w, rho);
        }
    }
    wave_fence();
    for (uint32_t t = lane; t < kmax; t += 64) store_fr<Fr>(part + 8 * ((size_t)blockIdx.x * kmax + t), a[t]);
}

// out[t] = sum over the waves of part[wave][t], a thread per t
template <class F>
__global__ __launch_bounds__(64) void k_kzg_subv_sum(const uint32_t* __restrict__ part, uint32_t waves, uint32_t kmax,
                                                    uint32_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= kmax) return;
    fe<F> s = fe_zero<F>();
    for (uint32_t wv = 0; wv < waves; wv++) s = fe_add<F>(s, kzgb::fr_words<F>(part + 8 * ((size_t)wv * kmax + t)));
    store_fr<F>(out + 8 * (size_t)t, s);
}

namespace {
const uint32_t* w32(const uint64_t* p) { return reinterpret_cast<const uint32_t*>(p); }

template <class C>
struct Batch {
    const SubKey<C>* key;
    size_t n;
    const uint64_t* com_xy;
    const uint8_t* com_inf;
    const uint32_t *idx_off, *idx;
    const uint64_t *y, *proof_xy;
    const uint8_t* proof_inf;
};
// what a fold makes: P[0] = P_0 - sum rho^j C_j, P[t] = P_t for t = 1 .. kmax; a[t], t < kmax
template <class C>
struct Fold {
    std::vector<G1AOf<C>> P;
    std::vector<FrOf<C>> a;
    explicit Fold(size_t kmax) : P(kmax + 1, C::G1::zero()), a(kmax, fe_zero<typename C::Fr>()) {}
    void add(const Fold& o) {
        for (size_t t = 0; t < P.size(); t++) P[t] = C::G1::add(P[t], o.P[t]);
        for (size_t t = 0; t < a.size(); t++) a[t] = fe_add<typename C::Fr>(a[t], o.a[t]);
    }
};
struct Laps {  // VKZG_HOST_TIMING: the device path's phases, us
    double upload = 0, fold = 0, msm = 0;
    size_t chunks = 0;
};

// Every status other than VC_OK, before any other work: VC_E_INVALID for the whole call first, then
// VC_E_RANGE. *kmax: the largest set.
template <class C>
int check_args(vc_ctx* ctx, const Batch<C>& b, size_t* kmax) {
    *kmax = 0;
    if (ctx && ctx->curve != C::CURVE) return VC_E_INVALID;
    if (b.n == 0) return VC_OK;
    if (!b.com_xy || !b.com_inf || !b.idx_off || !b.idx || !b.y || !b.proof_xy || !b.proof_inf) return VC_E_INVALID;
    if (b.n >= (size_t(1) << 32)) return VC_E_INVALID;
    const size_t N = b.key->size;
    for (size_t s = 0; s < b.n; s++)
        if (b.idx_off[s + 1] <= b.idx_off[s] || b.idx_off[s + 1] - b.idx_off[s] > N) return VC_E_INVALID;
    if (N <= (size_t(1) << 20)) {
        std::vector<uint32_t> seen(N, UINT32_MAX);  // the last set that held the index
        for (size_t s = 0; s < b.n; s++)
            for (uint32_t p = b.idx_off[s]; p < b.idx_off[s + 1]; p++) {
                const uint32_t i = b.idx[p];
                if (i >= N || seen[i] == (uint32_t)s) return VC_E_INVALID;
                seen[i] = (uint32_t)s;
            }
    } else {
        std::vector<uint32_t> srt;
        for (size_t s = 0; s < b.n; s++) {
            srt.assign(b.idx + b.idx_off[s], b.idx + b.idx_off[s + 1]);
            std::sort(srt.begin(), srt.end());
            if (srt.back() >= N || std::adjacent_find(srt.begin(), srt.end()) != srt.end()) return VC_E_INVALID;
        }
    }
    for (size_t s = 0; s < b.n; s++) *kmax = std::max<size_t>(*kmax, b.idx_off[s + 1] - b.idx_off[s]);
    if (*kmax > b.key->K) return VC_E_RANGE;
    if (ctx && N > kzgm::KM_MAX_N) return VC_E_RANGE;  // the device path: the prover's domains
    return VC_OK;
}

// proofs [lo, hi) on one thread; false when one of them is malformed
template <class C>
bool fold_range(const Batch<C>& b, size_t lo, size_t hi, size_t kmax, const FrOf<C>& rho, Fold<C>& out) {
    using Fr = typename C::Fr;
    using G1 = typename C::G1;
    std::vector<fe<Fr>> x, c, z(kmax), sc(kmax);
    FrOf<C> w = kzgb::pow_index(rho, lo);
    for (size_t j = lo; j < hi; j++) {
        const uint32_t b0 = b.idx_off[j], k = b.idx_off[j + 1] - b0;
        const bool c_inf = b.com_inf[j] != 0, pi_inf = b.proof_inf[j] != 0;
        G1POf<C> Cm, pi;
        if (!entry_check<C>(w32(b.com_xy) + C::PW * j, c_inf, w32(b.proof_xy) + C::PW * j, pi_inf,
                            w32(b.y) + 8 * (size_t)b0, k, Cm, pi))
            return false;
        sub_weights<Fr>(b.key->omega, b.idx + b0, k, x, c);  // (one inversion: the host has no tables)
        coeffs_serial<Fr>(x.data(), c.data(), w32(b.y) + 8 * (size_t)b0, k, w, z.data(), sc.data(), out.a.data());
        if (!pi_inf)
            for (uint32_t t = 0; t <= k; t++)
                out.P[t] = G1::add(out.P[t], kzgb::scalar_mul<C>(pi, row_scalar<Fr>(z.data(), k, t, w)));
        if (!c_inf) out.P[0] = G1::add(out.P[0], kzgb::scalar_mul<C>(Cm, fe_neg<Fr>(w)));
        w = fe_mul<Fr>(w, rho);
    }
    return true;
}

template <class C>
int fold_host(const Batch<C>& b, size_t kmax, const FrOf<C>& rho, Fold<C>* total, bool* malformed) {
    HostPool& pool = host_pool();
    const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>(pool.size(), b.n));
    std::vector<Fold<C>> part(T, Fold<C>(kmax));
    std::vector<uint8_t> ok(T, 1);
    pool.run([&](unsigned k) {
        if (k >= T) return;
        ok[k] = fold_range<C>(b, b.n * k / T, b.n * (k + 1) / T, kmax, rho, part[k]) ? 1 : 0;
    });
    *malformed = false;
    for (unsigned k = 0; k < T; k++) {
        if (!ok[k]) *malformed = true;
        else total->add(part[k]);
    }
    return VC_OK;
}

template <class C>
int fold_device(vc_ctx* ctx, const Batch<C>& b, size_t kmax, const FrOf<C>& rho, Fold<C>* total, bool* malformed,
                Laps* laps) {
    using Fr = typename C::Fr;
    const size_t n = b.n, N = b.key->size;
    const size_t waves_max = std::min(SV_WAVES_MAX, std::max<size_t>(64, SV_PART_MAX / kmax));
    size_t chunk = std::min(waves_max * SV_RUN_MAX, std::max<size_t>(1, SV_ROWS_MAX / (kmax + 2)));
    // VKZG_KZG_SUBV_CHUNK (read per call): a test forces small chunks
    if (const char* e = getenv("VKZG_KZG_SUBV_CHUNK"))
        if (atol(e) > 0) chunk = std::min<size_t>((size_t)atol(e), chunk);
    chunk = std::min(chunk, n);
    size_t max_idx = 0;  // the most indices a chunk holds
    for (size_t lo = 0; lo < n; lo += chunk)
        max_idx = std::max<size_t>(max_idx, b.idx_off[std::min(lo + chunk, n)] - b.idx_off[lo]);
    constexpr size_t PW = C::PW, PB = PW * 4;  // words and bytes of a G1 point
    const bool timing = host_timing();
    hipStream_t st = ctx->stream;
    const fe<Fr>*pw = nullptr, *inv1 = nullptr;
    VK_TRY(domain_tables<Fr>(ctx, b.key->omega, N, &pw, nullptr, &inv1));
    DevBuf d_pts(ctx), d_y(ctx), d_idx(ctx), d_off(ctx), d_flags(ctx), d_rows(ctx), d_part(ctx);
    VK_TRY(d_pts.ensure(chunk * 2 * PB));                     // C | pi
    VK_TRY(d_y.ensure(max_idx * 32));
    VK_TRY(d_idx.ensure(max_idx * 4));
    VK_TRY(d_off.ensure((chunk + 1) * 4));
    VK_TRY(d_flags.ensure(chunk * 2));                        // identity flags of C | pi
    VK_TRY(d_rows.ensure((kmax + 2) * chunk * 32));
    VK_TRY(d_part.ensure((waves_max + 1) * kmax * 32 + 4));   // the waves' partials, their sum, the bad flag
    uint32_t* d_com = d_pts.as<uint32_t>();
    uint32_t* d_proof = d_com + chunk * PW;
    uint8_t* d_cinf = d_flags.as<uint8_t>();
    uint8_t* d_pinf = d_cinf + chunk;
    uint32_t* d_sum = d_part.as<uint32_t>() + waves_max * kmax * 8;
    uint32_t* d_bad = d_sum + kmax * 8;
    std::vector<uint32_t> rel(chunk + 1), back(kmax * 8 + 1);
    Table* t = &ctx->scratch;
    *malformed = false;
    for (size_t lo = 0; lo < n; lo += chunk) {
        const size_t cnt = std::min(chunk, n - lo);
        const size_t base = b.idx_off[lo], nidx = b.idx_off[lo + cnt] - base;
        size_t kc = 0;  // the chunk's largest set: its rows and MSMs
        for (size_t i = 0; i <= cnt; i++) rel[i] = b.idx_off[lo + i] - (uint32_t)base;
        for (size_t i = 0; i < cnt; i++) kc = std::max<size_t>(kc, rel[i + 1] - rel[i]);
        // (cnt <= waves_max SV_RUN_MAX, so the run is at most SV_RUN_MAX)
        const size_t run = std::max(SV_RUN_MIN, (cnt + waves_max - 1) / waves_max), waves = (cnt + run - 1) / run;
        if (run > SV_RUN_MAX) return VC_E_INVALID;
        const double c0 = timing ? clock_us() : 0.0;
        VK_CHECK_HIP(hipMemcpyAsync(d_com, w32(b.com_xy) + PW * lo, cnt * PB, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_proof, w32(b.proof_xy) + PW * lo, cnt * PB, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_y.p, b.y + 4 * base, nidx * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_idx.p, b.idx + base, nidx * 4, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_off.p, rel.data(), (cnt + 1) * 4, hipMemcpyHostToDevice, st));
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
        VK_LAUNCH(ctx, C::CURVE == VC_CURVE_BN254 ? "kzg_subv_fold" : "kzg_bls_subv_fold", k_kzg_subv_fold<C>, waves,
                  SV_BLOCK, kc * 64, d_com, d_cinf, d_proof, d_pinf, d_y.as<uint32_t>(), d_idx.as<uint32_t>(),
                  d_off.as<uint32_t>(), pw, inv1, (uint32_t)N, rho, (uint64_t)lo, (uint32_t)cnt, (uint32_t)run,
                  (uint32_t)kc, t->bases.as<G1POf<C>>(), t->inf.as<uint8_t>(), d_rows.as<uint32_t>(),
                  d_part.as<uint32_t>(), d_bad);
        VK_LAUNCH(ctx, "kzg_subv_sum", k_kzg_subv_sum<Fr>, (kc + 63) / 64, 64, 0, d_part.as<uint32_t>(),
                  (uint32_t)waves, (uint32_t)kc, d_sum);
        VK_CHECK_HIP(hipMemcpyAsync(back.data(), d_sum, kc * 32, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipMemcpyAsync(&back[kmax * 8], d_bad, 4, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipStreamSynchronize(st));  // (rel is rewritten for the next chunk)
        const double c2 = timing ? clock_us() : 0.0;
        if (back[kmax * 8]) {
            *malformed = true;
            return VC_OK;
        }
        for (size_t k = 0; k < kc; k++) total->a[k] = fe_add<Fr>(total->a[k], kzgb::fr_words<Fr>(&back[8 * k]));
        G1AOf<C> acc;
        VK_TRY(msm_run(ctx, t, 0, d_rows.p, 2 * cnt, 1, reinterpret_cast<uint32_t*>(&acc)));
        total->P[0] = C::G1::add(total->P[0], acc);
        for (size_t k = 1; k <= kc; k++) {
            VK_TRY(msm_run(ctx, t, 0, d_rows.as<uint8_t>() + (k + 1) * cnt * 32, cnt, 1,
                           reinterpret_cast<uint32_t*>(&acc)));
            total->P[k] = C::G1::add(total->P[k], acc);
        }
        if (timing) {
            VK_CHECK_HIP(hipStreamSynchronize(st));
            laps->upload += c1 - c0, laps->fold += c2 - c1, laps->msm += clock_us() - c2;
        }
        laps->chunks++;
    }
    return VC_OK;
}

// sum_t a_t g1[t] by joint double-and-add, the t split over the host pool
template <class C>
G1AOf<C> powers_msm(const SubKey<C>& key, const std::vector<FrOf<C>>& a) {
    using Fr = typename C::Fr;
    using G1 = typename C::G1;
    const size_t m = a.size();
    if (!m) return G1::zero();
    std::vector<uint32_t> kw(8 * m);
    for (size_t t = 0; t < m; t++) {
        const fe<Fr> c = fe_from_mont<Fr>(a[t]);
        for (int i = 0; i < 8; i++) kw[8 * t + i] = c.v[i];
    }
    HostPool& pool = host_pool();
    const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>(pool.size(), (m + 3) / 4));
    std::vector<G1AOf<C>> part(T, G1::zero());
    pool.run([&](unsigned k) {
        if (k >= T) return;
        G1AOf<C> r = G1::zero();
        for (int i = 7; i >= 0; i--)
            for (int bit = 31; bit >= 0; bit--) {
                r = ate::g1_dbl(r);
                for (size_t t = m * k / T; t < m * (k + 1) / T; t++)
                    if ((kw[8 * t + i] >> bit) & 1) r = ate::g1_madd(r, key.g1[t], false);
            }
        part[k] = r;
    });
    G1AOf<C> r = part[0];
    for (unsigned k = 1; k < T; k++) r = G1::add(r, part[k]);
    return r;
}

// rho Montgomery; P: kmax + 1 accumulators, P[0] = P_H
template <class C>
int fold_impl(vc_ctx* ctx, const Batch<C>& b, size_t kmax, const FrOf<C>& rho, std::vector<G1AOf<C>>* P,
              bool* malformed, Laps* laps) {
    Fold<C> total(kmax);
    if (ctx) {
        Guard g(ctx);
        VK_TRY(fold_device(ctx, b, kmax, rho, &total, malformed, laps));
    } else {
        VK_TRY(fold_host(b, kmax, rho, &total, malformed));
    }
    if (*malformed) return VC_OK;
    total.P[0] = C::G1::add(total.P[0], powers_msm<C>(*b.key, total.a));
    *P = std::move(total.P);
    return VC_OK;
}

// the key's line tables 0 .. kmax: made on first use, once per key (pairing_internal.hpp)
template <class C>
void key_lines(const SubKey<C>& key, size_t kmax, std::vector<const ate::LineCoefT<typename C::Fq>*>* tabs) {
    using Line = ate::LineCoefT<typename C::Fq>;
    std::lock_guard<std::mutex> lk(key.lines_mu);
    const size_t have = key.lines.size();
    if (have < kmax + 1) {
        for (size_t t = have; t <= kmax; t++) key.lines.emplace_back(new Line[C::PC::ATE_LINES]);
        pool_for(have, kmax + 1, 2, [&](size_t t) { ate::ate_line_table(key.g2[t], key.lines[t].get()); });
    }
    tabs->resize(kmax + 1);
    for (size_t t = 0; t <= kmax; t++) (*tabs)[t] = key.lines[t].get();
}

// e(P[0], H) prod_{t >= 1} e(P[t], [s^t]_2) == 1: the tables split over the host pool, the partial
// products multiplied, one final exponentiation
template <class C>
bool pair_check(const SubKey<C>& key, const std::vector<G1AOf<C>>& P) {
    using Fq = typename C::Fq;
    const size_t m = P.size();
    std::vector<const ate::LineCoefT<Fq>*> tabs;
    key_lines<C>(key, m - 1, &tabs);
    std::vector<ate::G1EvalT<Fq>> ev(m);
    for (size_t t = 0; t < m; t++) ev[t] = ate::g1_eval_acc(P[t]);
    HostPool& pool = host_pool();
    const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>(pool.size(), (m + 3) / 4));
    std::vector<ate::Fq12T<Fq>> part(T);
    pool.run([&](unsigned k) {
        if (k >= T) return;
        const size_t lo = m * k / T, hi = m * (k + 1) / T;
        part[k] = ate::miller_loop_tabn<Fq>((int)(hi - lo), ev.data() + lo, tabs.data() + lo);
    });
    ate::Fq12T<Fq> f = part[0];
    for (unsigned k = 1; k < T; k++) f = ate::fq12_mul(f, part[k]);
    return ate::fq12_is_one(ate::final_exp(f));
}

// hash_to_field(seed, dst = "vkzg-kzg-subv-batch") in the curve's Fr, canonical words out
template <class C>
void subv_challenge(const uint8_t seed[32], uint64_t* rho_fr) {
    static const char dst[] = "vkzg-kzg-subv-batch";
    mont_to_canon<typename C::Fr>(
        hash_to_fr<typename C::Fr>(seed, 32, reinterpret_cast<const uint8_t*>(dst), sizeof dst - 1), rho_fr);
}

template <class C>
int batch_fold(vc_ctx* ctx, const Batch<C>& b, const uint64_t* rho_fr, size_t* kmax_out, uint64_t* p_xy,
               uint8_t* p_inf, int* malformed) {
    using Fr = typename C::Fr;
    if (!rho_fr || !kmax_out || !p_xy || !p_inf || !malformed) return VC_E_INVALID;
    if (!ate::words_below_modulus<Fr>(w32(rho_fr))) return VC_E_INVALID;
    size_t kmax = 0;
    VK_TRY(check_args(ctx, b, &kmax));
    std::vector<G1AOf<C>> P(1, C::G1::zero());  // (n = 0: the sums are empty)
    bool bad = false;
    Laps laps;
    if (b.n) VK_TRY(fold_impl(ctx, b, kmax, canon_to_mont<Fr>(rho_fr), &P, &bad, &laps));
    *malformed = bad ? 1 : 0;
    if (bad) return VC_OK;
    *kmax_out = kmax;
    return acc_to_affine_batch(C::CURVE, reinterpret_cast<const uint32_t*>(P.data()), kmax + 1, p_xy, p_inf);
}

template <class C>
int verify_batch(vc_ctx* ctx, const Batch<C>& b, const uint8_t* seed32, int* result, uint8_t* results) {
    if (!result) return VC_E_INVALID;
    size_t kmax = 0;
    VK_TRY(check_args(ctx, b, &kmax));
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
    subv_challenge<C>(seed, rho_c);
    const double c0 = host_timing() ? clock_us() : 0.0;
    std::vector<G1AOf<C>> P;
    bool bad = false;
    Laps laps;
    VK_TRY(fold_impl(ctx, b, kmax, canon_to_mont<typename C::Fr>(rho_c), &P, &bad, &laps));
    const double c1 = host_timing() ? clock_us() : 0.0;
    const bool ok = !bad && pair_check<C>(*b.key, P);
    if (host_timing())
        fprintf(stderr,
                "[kzg_verify_subvector_batch] n=%zu kmax=%zu chunks=%zu: upload %.1f us, fold %.1f us, msm %.1f us, "
                "whole fold %.1f us, pairing %.1f us, call %.1f us\n",
                b.n, kmax, laps.chunks, laps.upload, laps.fold, laps.msm, c1 - c0, clock_us() - c1, clock_us() - c0);
    *result = ok ? 1 : 0;
    if (!results) return VC_OK;
    if (ok) {
        memset(results, 1, b.n);
        return VC_OK;
    }
    // which ones: the single verifier over the host pool (its statuses were all decided above)
    constexpr size_t NL2 = C::PW / 2;  // u64 words of a point
    pool_for(0, b.n, 2, [&](size_t j) {
        int r = 0;
        const uint32_t b0 = b.idx_off[j];
        vc_kzg_verify_subvector(b.key, b.com_xy + NL2 * j, b.com_inf[j], b.idx + b0, b.idx_off[j + 1] - b0,
                                b.y + 4 * (size_t)b0, b.proof_xy + NL2 * j, b.proof_inf[j], &r);
        results[j] = r ? 1 : 0;
    });
    return VC_OK;
}

template <class C>
Batch<C> batch_of(const vc_kzg_svk* svk, size_t n, const uint64_t* com_xy, const uint8_t* com_inf,
                  const uint32_t* idx_off, const uint32_t* idx, const uint64_t* y, const uint64_t* proof_xy,
                  const uint8_t* proof_inf) {
    return Batch<C>{&sub_key<C>(svk), n, com_xy, com_inf, idx_off, idx, y, proof_xy, proof_inf};
}
bool is_bls(const vc_kzg_svk* svk) { return svk->curve == VC_CURVE_BLS12_381; }  // the key's curve decides
}  // namespace

}  // namespace vk

using namespace vk;

extern "C" int vc_kzg_subvector_batch_challenge(int curve, const uint8_t seed[32], uint64_t* rho_fr) {
    if (!seed || !rho_fr || (curve != VC_CURVE_BN254 && curve != VC_CURVE_BLS12_381)) return VC_E_INVALID;
    if (curve == VC_CURVE_BLS12_381) subv_challenge<BLS381Kzg>(seed, rho_fr);
    else subv_challenge<BN254Kzg>(seed, rho_fr);
    return VC_OK;
}

extern "C" int vc_kzg_subvector_batch_fold(vc_ctx* ctx, const vc_kzg_svk* svk, size_t n, const uint64_t* com_xy,
                                           const uint8_t* com_inf, const uint32_t* idx_off, const uint32_t* idx,
                                           const uint64_t* y, const uint64_t* proof_xy, const uint8_t* proof_inf,
                                           const uint64_t* rho_fr, size_t* kmax_out, uint64_t* p_xy, uint8_t* p_inf,
                                           int* malformed) {
    if (!svk) return VC_E_INVALID;
    if (is_bls(svk))
        return batch_fold(ctx, batch_of<BLS381Kzg>(svk, n, com_xy, com_inf, idx_off, idx, y, proof_xy, proof_inf),
                          rho_fr, kmax_out, p_xy, p_inf, malformed);
    return batch_fold(ctx, batch_of<BN254Kzg>(svk, n, com_xy, com_inf, idx_off, idx, y, proof_xy, proof_inf), rho_fr,
                      kmax_out, p_xy, p_inf, malformed);
}

extern "C" int vc_kzg_verify_subvector_batch(vc_ctx* ctx, const vc_kzg_svk* svk, size_t n, const uint64_t* com_xy,
                                             const uint8_t* com_inf, const uint32_t* idx_off, const uint32_t* idx,
                                             const uint64_t* y, const uint64_t* proof_xy, const uint8_t* proof_inf,
                                             const uint8_t* seed32, int* result, uint8_t* results) {
    if (!svk) return VC_E_INVALID;
    if (is_bls(svk))
        return verify_batch(ctx, batch_of<BLS381Kzg>(svk, n, com_xy, com_inf, idx_off, idx, y, proof_xy, proof_inf),
                            seed32, result, results);
    return verify_batch(ctx, batch_of<BN254Kzg>(svk, n, com_xy, com_inf, idx_off, idx, y, proof_xy, proof_inf), seed32,
                        result, results);
}

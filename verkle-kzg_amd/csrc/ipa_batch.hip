// IPA batch verification (vc_ipa_verify_batch): n openings over one CRS, one combined verdict. The
// entries fold with the weights rho^j sigma_j into one point S (csrc/ipa_batch.hpp), accepted when it
// is the identity. Per chunk of at most 65536 proofs the device path is
//   upload       the arrays, as vc_ipa_verify_many uploads them;
//   transcripts  k_ipa_batch_transcripts, a lane per proof: the fresh "ipa" transcript's [w, x_k]
//                hashed from register words (with prior transcripts: the host pool's, uploaded);
//   prep         k_ipa_batch_prep, a lane per point: validates C, L_k, R_k and writes them, Montgomery
//                affine, into the context's scratch table [C_j, L_j0, R_j0, ..] (the kernel is the
//                table's fill, so no entry ever reaches bases_fill's check);
//   field        k_ipa_batch_field, a wave walks several proofs: each lane keeps its N / 64 columns
//                of the summed fixed row in registers; per group of up to 64 proofs a lane per proof
//                then makes the q entry and the proof's 1 + 2K weighted scalars, which go beside
//                the table as msm_run's rows; one partial row per wave;
//   rowsum       k_ipa_batch_rowsum, a lane per column: the waves' partial rows added into the
//                call's row;
//   MSM          msm_run over the chunk's points; the accumulators are added on the host.
// After the last chunk msm_batch_run commits the one summed row, and the host adds the two points.
// A malformed entry sets the call's bad flag with a plain store; the flag is read before the MSMs,
// which a malformed batch skips. 65536 proofs of K = 8 are 1.1 M points: 71 MB of uploaded points
// and 71 MB of table, the largest pieces of a workspace sized by the chunk.
// The host paths (ctx == NULL) run ipa_batch.hpp over the host pool: the oracle check on a machine
// without a GPU, not a product path.
#include <hip/hip_runtime.h>
#include <sys/random.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "ec29.hpp"
#include "host/pool.hpp"
#include "ipa_batch.hpp"
#include "scheme_internal.hpp"

namespace vk {

using namespace ipab;

constexpr size_t IB_CHUNK_MAX = 65536;
constexpr int IB_CPL = 4;            // columns of the fixed row a lane keeps: N <= 64 IB_CPL
constexpr size_t IB_N_MAX = 64 * IB_CPL;
constexpr size_t IB_WAVES = 2048;    // waves of the field kernel at a full chunk: two per SIMD
constexpr uint32_t IB_PREP_BLOCK = 256;

// a lane per proof; chal: 1 + K challenges per proof, Montgomery (canon = 0) or canonical
__global__ __launch_bounds__(64) void k_ipa_batch_transcripts(
    const uint32_t* __restrict__ com_xy, const uint8_t* __restrict__ com_inf, const uint32_t* __restrict__ points,
    const uint32_t* __restrict__ y, const uint32_t* __restrict__ l_xy, const uint8_t* __restrict__ l_inf,
    const uint32_t* __restrict__ r_xy, const uint8_t* __restrict__ r_inf, int K, uint32_t n, int canon,
    uint32_t* __restrict__ chal) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    uint32_t* out = chal + (size_t)p * (size_t)(K + 1) * 8;
    entry_challenges(p, K, com_xy, com_inf, points, y, l_xy, l_inf, r_xy, r_inf, out);
    if (canon)
        for (int k = 0; k <= K; k++) fr_store(fe_from_mont<BN254Fr>(fr_load(out + 8 * k)), out + 8 * k);
}

// a lane per point: point g = T p + t of the chunk is term t of proof p (0: C, 1 + 2k: L_k, 2 + 2k:
// R_k). bases / inf: the scratch table; bad: the call's flag (every malformed lane stores the same 1)
__global__ __launch_bounds__(IB_PREP_BLOCK) void k_ipa_batch_prep(
    const uint32_t* __restrict__ com_xy, const uint8_t* __restrict__ com_inf, const uint32_t* __restrict__ l_xy,
    const uint8_t* __restrict__ l_inf, const uint32_t* __restrict__ r_xy, const uint8_t* __restrict__ r_inf, int K,
    uint32_t n, G1P* __restrict__ bases, uint8_t* __restrict__ inf, uint32_t* __restrict__ bad) {
    const uint32_t T = 1 + 2 * (uint32_t)K;
    const size_t g = (size_t)blockIdx.x * IB_PREP_BLOCK + threadIdx.x;
    if (g >= (size_t)n * T) return;
    const size_t p = g / T;
    const uint32_t t = (uint32_t)(g % T);
    const size_t at = p * (size_t)K + (size_t)((t - 1) >> 1);
    const uint32_t* xy = t == 0 ? com_xy + 16 * p : ((t - 1) & 1) ? r_xy + 16 * at : l_xy + 16 * at;
    bool is_inf = (t == 0 ? com_inf[p] : ((t - 1) & 1) ? r_inf[at] : l_inf[at]) != 0;
    uint32_t w[16];
    for (int k = 0; k < 16; k++) w[k] = xy[k];
    G1P P;
    if (!point_load(w, is_inf, P)) {
        *bad = 1u;
        P = G1P{fe_zero<BN254Fq>(), fe_zero<BN254Fq>()};
        is_inf = true;
    }
    bases[g] = P;
    inf[g] = is_inf ? 1 : 0;
}

// One wave per block; wave v takes proofs [v ppw, (v + 1) ppw) of the chunk, entry `first` + p of
// the call, in groups of up to 64: the wave walks a group's proofs one at a time for the columns of
// the fixed row, then a lane per proof makes the group's q entries and variable scalars (serial work
// per proof, which one lane per wave would otherwise do with 63 idle). chal: [w, x_0 .. x_{K-1}] Montgomery per proof; tip, y, point canonical; pw: the
// domain's w^i (Montgomery); part: N + 1 Montgomery scalars per wave; vs: 1 + 2K canonical scalars
// per proof (zero for an entry with tip, y or point >= r, which sets bad).
__global__ __launch_bounds__(64) void k_ipa_batch_field(
    const uint32_t* __restrict__ chal, const uint32_t* __restrict__ tip_w, const uint32_t* __restrict__ y_w,
    const uint32_t* __restrict__ point_w, const FrE* __restrict__ pw, FrE n_inv, FrE rho, uint64_t first, uint32_t N,
    int K, uint32_t n, uint32_t ppw, uint32_t* __restrict__ part, uint32_t* __restrict__ vs,
    uint32_t* __restrict__ bad) {
    __shared__ FrE xs[32];
    __shared__ FrE g_scale[64], g_num[64], g_wt[64];  // a group's proofs: sigma, the sum's numerator, rho^j
    __shared__ uint8_t g_ok[64];
    const uint32_t lane = threadIdx.x;
    const uint32_t lo = blockIdx.x * ppw, hi = min(n, lo + ppw);
    const uint32_t T = 1 + 2 * (uint32_t)K;
    FrE acc[IB_CPL], accq = fe_zero<BN254Fr>();
#pragma unroll
    for (int c = 0; c < IB_CPL; c++) acc[c] = fe_zero<BN254Fr>();
    FrE wt = pow_index(rho, first + lo);
    for (uint32_t g = lo; g < hi; g += 64) {
        const uint32_t gcnt = min(64u, hi - g);
        // the columns, the wave on one proof at a time
        for (uint32_t q = 0; q < gcnt; q++, wt = fr_mul(wt, rho)) {
            const uint32_t p = g + q;
            const uint32_t* ch = chal + (size_t)p * (size_t)(K + 1) * 8;
            __syncthreads();  // (the previous proof's reads of xs, the previous group's of g_*, are done)
            if ((int)lane < K) xs[lane] = fr_load(ch + 8 * (1 + lane));
            __syncthreads();
            uint32_t tw[8], yw[8], zw[8];
            for (int k = 0; k < 8; k++) {
                tw[k] = tip_w[8 * (size_t)p + k];
                yw[k] = y_w[8 * (size_t)p + k];
                zw[k] = point_w[8 * (size_t)p + k];
            }
            if (!entry_fr_ok(tw, yw, zw)) {  // (uniform over the wave)
                uint32_t* out = vs + (size_t)p * T * 8;
                for (uint32_t i = lane; i < T * 8; i += 64) out[i] = 0;
                if (lane == 0) *bad = 1u, g_ok[q] = 0;
                continue;
            }
            const FrE tip = fe_to_mont<BN254Fr>(fr_load(tw)), z = fe_to_mont<BN254Fr>(fr_load(zw));
            uint64_t idx = 0;
            const bool in_dom = point_in_domain(zw, N, &idx);
            FrE s[IB_CPL];
            Frac f = frac_zero();
#pragma unroll
            for (int c = 0; c < IB_CPL; c++) {
                const uint32_t i = lane + 64 * c;
                if (i < N) {
                    s[c] = s_coeff(xs, K, i);
                    if (!in_dom) f = frac_add_term(f, s[c], pw[i], z);
                }
            }
            // outside the domain every scalar of the proof is multiplied by the sum's denominator,
            // sigma = z^N - 1 (ipa_verify.hpp)
            FrE scale = fe_one<BN254Fr>();
            if (!in_dom) {
                for (uint32_t m = 1; m < 64; m <<= 1) f = frac_add(f, shfl_xor_pod(f, m));
                scale = f.den;
            }
            const FrE mt = fr_mul(tip, fr_mul(scale, wt));
#pragma unroll
            for (int c = 0; c < IB_CPL; c++)
                if (lane + 64 * c < N) acc[c] = fe_add<BN254Fr>(acc[c], row_entry(mt, s[c]));
            if (lane == 0) g_scale[q] = scale, g_num[q] = f.num, g_wt[q] = wt, g_ok[q] = 1;
        }
        __syncthreads();
        // the q entry and the variable scalars, a lane per proof of the group: the challenges are
        // read where they lie in device memory (an array of Montgomery elements)
        if (lane < gcnt && g_ok[lane]) {
            const uint32_t p = g + lane;
            const uint32_t* ch = chal + (size_t)p * (size_t)(K + 1) * 8;
            const FrE* xg = reinterpret_cast<const FrE*>(ch + 8);
            uint32_t tw[8], yw[8], zw[8];
            for (int k = 0; k < 8; k++) {
                tw[k] = tip_w[8 * (size_t)p + k];
                yw[k] = y_w[8 * (size_t)p + k];
                zw[k] = point_w[8 * (size_t)p + k];
            }
            const FrE tip = fe_to_mont<BN254Fr>(fr_load(tw)), z = fe_to_mont<BN254Fr>(fr_load(zw));
            const FrE scale = g_scale[lane], w_p = g_wt[lane];
            uint64_t idx = 0;
            const bool in_dom = point_in_domain(zw, N, &idx);
            const FrE cb = in_dom ? s_coeff(xg, K, (uint32_t)idx)
                                  : bary_dot_scaled(Frac{g_num[lane], scale}, z, K, n_inv);
            const FrE prodx = var_scalars(xg, K, fr_mul(scale, w_p), vs + (size_t)p * T * 8);
            accq = fe_add<BN254Fr>(
                accq, fr_mul(w_p, row_tail(prodx, fr_load(ch), fe_to_mont<BN254Fr>(fr_load(yw)), tip, cb, scale)));
            // (a zero scale: the host has rejected the domain elements that give one)
            if (fe_is_zero<BN254Fr>(scale)) *bad = 1u;
        }
    }
    for (uint32_t m = 1; m < 64; m <<= 1) accq = fe_add<BN254Fr>(accq, shfl_xor_pod(accq, m));
    uint32_t* row = part + (size_t)blockIdx.x * ((size_t)N + 1) * 8;
#pragma unroll
    for (int c = 0; c < IB_CPL; c++)
        if (lane + 64 * c < N) fr_store(acc[c], row + 8 * (size_t)(lane + 64 * c));
    if (lane == 0) fr_store(accq, row + 8 * (size_t)N);
}

// a lane per column of the N + 1: total[i] += sum over the waves' partial rows
__global__ __launch_bounds__(64) void k_ipa_batch_rowsum(const uint32_t* __restrict__ part, uint32_t waves,
                                                         uint32_t width, uint32_t* __restrict__ total) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= width) return;
    FrE s = fr_load(total + 8 * (size_t)i);
    for (uint32_t v = 0; v < waves; v++) s = fe_add<BN254Fr>(s, fr_load(part + ((size_t)v * width + i) * 8));
    fr_store(s, total + 8 * (size_t)i);
}

namespace {
const uint32_t* w32(const uint64_t* p) { return reinterpret_cast<const uint32_t*>(p); }

struct Batch {
    size_t N, n;
    int K;
    const uint64_t *com_xy, *points, *l_xy, *r_xy, *tip, *y;
    const uint8_t *com_inf, *l_inf, *r_inf;
    vc_transcript** transcripts;
    bool prior() const {  // any prior transcript: then every transcript runs on the host pool
        if (transcripts)
            for (size_t p = 0; p < n; p++)
                if (transcripts[p]) return true;
        return false;
    }
};
struct Laps {  // VKZG_HOST_TIMING: the device path's phases, us
    double host_tr = 0, upload = 0, transcripts = 0, prep = 0, field = 0, msm = 0, fixed = 0;
    size_t chunks = 0;
};

int log2_of(size_t N) {
    int K = 0;
    while ((size_t(1) << K) < N) K++;
    return K;
}
bool n_ok(size_t N, size_t max) { return N >= 2 && !(N & (N - 1)) && N <= max; }
bool arrays_ok(const Batch& b, bool with_tip) {
    return b.n == 0 || (b.com_xy && b.com_inf && b.points && b.l_xy && b.l_inf && b.r_xy && b.r_inf && b.y &&
                        (!with_tip || b.tip));
}
// vc_ipa_verify_many's rule: a point that is a domain element w^i but not below N
bool domain_error(const Batch& b) {
    using F = BN254Fr;
    std::atomic<bool> err{false};
    pool_for(0, b.n, 256, [&](size_t p) {
        uint64_t idx;
        if (!ate::words_below_modulus<F>(w32(b.points + 4 * p))) return;
        if (point_in_domain(w32(b.points + 4 * p), b.N, &idx)) return;
        if (fe_eq<F>(fe_pow_u64<F>(canon_to_mont<F>(b.points + 4 * p), b.N), fe_one<F>())) err = true;
    });
    return err;
}
std::vector<Fr> domain_powers(size_t N) {
    std::vector<Fr> pw(N);
    const Fr omega = bn254_group_gen(N);
    Fr w = fe_one<BN254Fr>();
    for (size_t i = 0; i < N; i++) {
        pw[i] = w;
        w = fe_mul<BN254Fr>(w, omega);
    }
    return pw;
}
G1A scalar_mul(const G1P& P, const FrE& k_mont) {
    const FrE k = fe_from_mont<BN254Fr>(k_mont);
    G1A r = BN254G1::zero();
    for (int b = BN254Fr::BITS - 1; b >= 0; b--) {
        r = BN254G1::dbl(r);
        if ((k.v[b >> 5] >> (b & 31)) & 1u) r = BN254G1::madd(r, P, false);
    }
    return r;
}

// the chunk's arrays in device memory
struct DevArrays {
    DevBuf fr, pts, flags;
    uint32_t *tip, *y, *point, *com, *l, *r;
    uint8_t *cinf, *linf, *rinf;
    explicit DevArrays(vc_ctx* ctx) : fr(ctx), pts(ctx), flags(ctx) {}
    int ensure(size_t chunk, int K) {
        const size_t T = 1 + 2 * (size_t)K;
        VK_TRY(fr.ensure(chunk * 3 * 32));   // tip | y | point
        VK_TRY(pts.ensure(chunk * T * 64));  // C | L | R
        VK_TRY(flags.ensure(chunk * T));     // identity flags of C | L | R
        tip = fr.as<uint32_t>(), y = tip + chunk * 8, point = y + chunk * 8;
        com = pts.as<uint32_t>(), l = com + chunk * 16, r = l + chunk * (size_t)K * 16;
        cinf = flags.as<uint8_t>(), linf = cinf + chunk, rinf = linf + chunk * (size_t)K;
        return VC_OK;
    }
    int upload(const Batch& b, size_t lo, size_t cnt, hipStream_t st) {
        const size_t K = (size_t)b.K;
        if (b.tip) VK_CHECK_HIP(hipMemcpyAsync(tip, b.tip + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(y, b.y + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(point, b.points + 4 * lo, cnt * 32, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(com, b.com_xy + 8 * lo, cnt * 64, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(l, b.l_xy + 8 * lo * K, cnt * K * 64, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(r, b.r_xy + 8 * lo * K, cnt * K * 64, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(cinf, b.com_inf + lo, cnt, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(linf, b.l_inf + lo * K, cnt * K, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(rinf, b.r_inf + lo * K, cnt * K, hipMemcpyHostToDevice, st));
        return VC_OK;
    }
};

size_t chunk_size(size_t n) {
    size_t chunk = IB_CHUNK_MAX;
    // VKZG_IPA_BATCH_CHUNK (read per call): a test forces small chunks
    if (const char* e = getenv("VKZG_IPA_BATCH_CHUNK"))
        if (atol(e) > 0) chunk = std::min<size_t>((size_t)atol(e), IB_CHUNK_MAX);
    return std::min(chunk, n);
}

int launch_transcripts(vc_ctx* ctx, const DevArrays& d, int K, size_t cnt, int canon, uint32_t* d_chal) {
    VK_LAUNCH(ctx, "ipa_batch_transcripts", k_ipa_batch_transcripts, (cnt + 63) / 64, 64, 0, d.com, d.cinf, d.point, d.y,
              d.l, d.linf, d.r, d.rinf, K, (uint32_t)cnt, canon, d_chal);
    return VC_OK;
}

int challenges_device(vc_ctx* ctx, const Batch& b, uint64_t* out) {
    const size_t chunk = chunk_size(b.n), C = (size_t)b.K + 1;
    DevArrays d(ctx);
    DevBuf d_chal(ctx);
    VK_TRY(d.ensure(chunk, b.K));
    VK_TRY(d_chal.ensure(chunk * C * 32));
    hipStream_t st = ctx->stream;
    for (size_t lo = 0; lo < b.n; lo += chunk) {
        const size_t cnt = std::min(chunk, b.n - lo);
        VK_TRY(d.upload(b, lo, cnt, st));
        VK_TRY(launch_transcripts(ctx, d, b.K, cnt, 1, d_chal.as<uint32_t>()));
        VK_CHECK_HIP(hipMemcpyAsync(out + 4 * lo * C, d_chal.p, cnt * C * 32, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipStreamSynchronize(st));
    }
    return VC_OK;
}

// S = var + commit(row); chal (prior transcripts only): every entry's host challenges, Montgomery
int fold_device(vc_ctx* ctx, Table* t, const Batch& b, const Fr& rho, const std::vector<Fr>& chal, G1A* S,
                bool* malformed, Laps* laps) {
    const size_t N = b.N, n = b.n, C = (size_t)b.K + 1, T = 1 + 2 * (size_t)b.K;
    const size_t chunk = chunk_size(n), max_waves = std::min(chunk, IB_WAVES);
    const bool timing = host_timing();
    DevArrays d(ctx);
    DevBuf d_chal(ctx), d_vs(ctx), d_part(ctx), d_row(ctx), d_pw(ctx), d_fixed(ctx);
    VK_TRY(d.ensure(chunk, b.K));
    VK_TRY(d_chal.ensure(chunk * C * 32));
    VK_TRY(d_vs.ensure(chunk * T * 32));
    VK_TRY(d_part.ensure(max_waves * (N + 1) * 32));
    VK_TRY(d_row.ensure((N + 1) * 32 + 4));  // the call's summed row, then the bad flag
    VK_TRY(d_pw.ensure(N * 32));
    VK_TRY(d_fixed.ensure(65));
    hipStream_t st = ctx->stream;
    uint32_t* d_bad = d_row.as<uint32_t>() + (N + 1) * 8;
    const std::vector<Fr> pw = domain_powers(N);
    VK_CHECK_HIP(hipMemcpyAsync(d_pw.p, pw.data(), N * 32, hipMemcpyHostToDevice, st));
    VK_CHECK_HIP(hipMemsetAsync(d_row.p, 0, (N + 1) * 32 + 4, st));
    const Fr n_inv = fe_inv_bin<BN254Fr>(mont_from_u64<BN254Fr>(N));
    Table* sc = &ctx->scratch;
    G1A var = BN254G1::zero();
    *malformed = false;
    for (size_t lo = 0; lo < n; lo += chunk) {
        const size_t cnt = std::min(chunk, n - lo);
        const uint32_t ppw = (uint32_t)((cnt + max_waves - 1) / max_waves), waves = (uint32_t)((cnt + ppw - 1) / ppw);
        const double c0 = timing ? clock_us() : 0.0;
        VK_TRY(d.upload(b, lo, cnt, st));
        if (!chal.empty())
            VK_CHECK_HIP(hipMemcpyAsync(d_chal.p, &chal[lo * C], cnt * C * 32, hipMemcpyHostToDevice, st));
        VK_TRY(bases_reserve(ctx, sc, cnt * T));
        double c1 = 0, c2 = 0, c3 = 0;
        if (timing) {
            VK_CHECK_HIP(hipStreamSynchronize(st));
            c1 = clock_us();
        }
        if (chal.empty()) VK_TRY(launch_transcripts(ctx, d, b.K, cnt, 0, d_chal.as<uint32_t>()));
        if (timing) {
            VK_CHECK_HIP(hipStreamSynchronize(st));
            c2 = clock_us();
        }
        VK_LAUNCH(ctx, "ipa_batch_prep", k_ipa_batch_prep, (cnt * T + IB_PREP_BLOCK - 1) / IB_PREP_BLOCK, IB_PREP_BLOCK, 0,
                  d.com, d.cinf, d.l, d.linf, d.r, d.rinf, b.K, (uint32_t)cnt, sc->bases.as<G1P>(), sc->inf.as<uint8_t>(),
                  d_bad);
        if (timing) {
            VK_CHECK_HIP(hipStreamSynchronize(st));
            c3 = clock_us();
        }
        VK_LAUNCH(ctx, "ipa_batch_field", k_ipa_batch_field, waves, 64, 0, d_chal.as<uint32_t>(), d.tip, d.y, d.point,
                  d_pw.as<FrE>(), n_inv, rho, (uint64_t)lo, (uint32_t)N, b.K, (uint32_t)cnt, ppw, d_part.as<uint32_t>(),
                  d_vs.as<uint32_t>(), d_bad);
        VK_LAUNCH(ctx, "ipa_batch_rowsum", k_ipa_batch_rowsum, (N + 1 + 63) / 64, 64, 0, d_part.as<uint32_t>(), waves,
                  (uint32_t)(N + 1), d_row.as<uint32_t>());
        uint32_t bad = 0;
        VK_CHECK_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipStreamSynchronize(st));
        const double c4 = timing ? clock_us() : 0.0;
        if (bad) {
            *malformed = true;
            return VC_OK;
        }
        G1A acc;
        VK_TRY(msm_run(ctx, sc, 0, d_vs.p, cnt * T, /*mont=*/0, reinterpret_cast<uint32_t*>(&acc)));
        var = BN254G1::add(var, acc);
        if (timing) {
            VK_CHECK_HIP(hipStreamSynchronize(st));
            laps->upload += c1 - c0, laps->transcripts += c2 - c1, laps->prep += c3 - c2, laps->field += c4 - c3;
            laps->msm += clock_us() - c4;
        }
        laps->chunks++;
    }
    const double c5 = timing ? clock_us() : 0.0;
    uint8_t* d_fxy = d_fixed.as<uint8_t>();
    VK_TRY(msm_batch_run(ctx, t, N + 1, d_row.p, 1, /*mont=*/1, d_fxy, d_fxy + 64));
    uint32_t fixed[17] = {0};
    VK_CHECK_HIP(hipMemcpyAsync(fixed, d_fxy, 65, hipMemcpyDeviceToHost, st));
    VK_CHECK_HIP(hipStreamSynchronize(st));
    *S = var;
    if (!(reinterpret_cast<const uint8_t*>(fixed)[64])) {
        G1P F;
        F.x = fe_to_mont<BN254Fq>(words_load<BN254Fq>(fixed));
        F.y = fe_to_mont<BN254Fq>(words_load<BN254Fq>(fixed + 8));
        *S = BN254G1::madd(var, F, false);
    }
    if (timing) laps->fixed += clock_us() - c5;
    return VC_OK;
}

// the host pool, a contiguous slice of entries per thread; chal: every entry's challenges
int fold_host(const uint64_t* crs_xy, const Batch& b, const Fr& rho, const std::vector<Fr>& chal, G1A* S,
              bool* malformed) {
    const size_t N = b.N, C = (size_t)b.K + 1;
    std::vector<G1P> crs(N + 1);
    for (size_t i = 0; i <= N; i++)
        if (!ate::g1_load(w32(crs_xy + 8 * i), crs[i])) return VC_E_INVALID;
    const std::vector<Fr> pw = domain_powers(N);
    const Fr n_inv = fe_inv_bin<BN254Fr>(mont_from_u64<BN254Fr>(N));
    HostPool& pool = host_pool();
    const unsigned W = (unsigned)std::max<size_t>(1, std::min<size_t>(pool.size(), b.n));
    std::vector<std::vector<Fr>> rows(W, std::vector<Fr>(N + 1, fe_zero<BN254Fr>()));
    std::vector<G1A> vars(W, BN254G1::zero());
    std::vector<uint8_t> ok(W, 1);
    pool.run([&](unsigned k) {
        if (k >= W) return;
        const size_t lo = b.n * k / W, hi = b.n * (k + 1) / W;
        Fr wt = pow_index(rho, lo);
        for (size_t p = lo; p < hi && ok[k]; p++, wt = fe_mul<BN254Fr>(wt, rho))
            if (!fold_entry(p, (uint32_t)N, b.K, w32(b.com_xy), b.com_inf, w32(b.points), w32(b.l_xy), b.l_inf,
                            w32(b.r_xy), b.r_inf, w32(b.tip), w32(b.y), reinterpret_cast<const uint32_t*>(&chal[p * C]),
                            pw.data(), n_inv, wt, rows[k].data(), vars[k], scalar_mul))
                ok[k] = 0;
    });
    *malformed = false;
    for (unsigned k = 0; k < W; k++)
        if (!ok[k]) *malformed = true;
    if (*malformed) return VC_OK;
    // the summed row's commitment, a column slice per thread
    for (unsigned k = 1; k < W; k++) {
        for (size_t i = 0; i <= N; i++) rows[0][i] = fe_add<BN254Fr>(rows[0][i], rows[k][i]);
        vars[0] = BN254G1::add(vars[0], vars[k]);
    }
    const unsigned V = (unsigned)std::min<size_t>(pool.size(), N + 1);
    std::vector<G1A> fx(V, BN254G1::zero());
    pool.run([&](unsigned k) {
        if (k >= V) return;
        for (size_t i = (N + 1) * k / V; i < (N + 1) * (k + 1) / V; i++)
            fx[k] = BN254G1::add(fx[k], scalar_mul(crs[i], rows[0][i]));
    });
    *S = vars[0];
    for (unsigned k = 0; k < V; k++) *S = BN254G1::add(*S, fx[k]);
    return VC_OK;
}

// every entry's challenges on the host: the shared text for fresh transcripts, the transcript
// objects (advanced) when any prior one is given; Montgomery
void challenges_host(const Batch& b, std::vector<Fr>& chal) {
    const size_t C = (size_t)b.K + 1;
    chal.resize(b.n * C);
    if (b.prior()) {
        ipa_host_challenges(0, b.n, b.K, b.com_xy, b.com_inf, b.points, b.y, b.l_xy, b.l_inf, b.r_xy, b.r_inf,
                            b.transcripts, chal.data());
        return;
    }
    pool_for(0, b.n, 16, [&](size_t p) {
        entry_challenges(p, b.K, w32(b.com_xy), b.com_inf, w32(b.points), w32(b.y), w32(b.l_xy), b.l_inf, w32(b.r_xy),
                         b.r_inf, reinterpret_cast<uint32_t*>(&chal[p * C]));
    });
}

// the checks and the fold shared by vc_ipa_batch_fold and vc_ipa_verify_batch (n > 0); rho Montgomery
int fold_impl(vc_ctx* ctx, int table, const uint64_t* crs_xy, const Batch& b, const Fr& rho, G1A* S, bool* malformed,
              Laps* laps) {
    if (ctx ? ctx->curve != VC_CURVE_BN254 : !crs_xy) return VC_E_INVALID;
    if (!n_ok(b.N, IB_N_MAX) || !arrays_ok(b, true)) return VC_E_INVALID;
    std::vector<Fr> chal;
    if (!ctx) {
        if (domain_error(b)) return VC_E_DOMAIN;
        challenges_host(b, chal);
        return fold_host(crs_xy, b, rho, chal, S, malformed);
    }
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    if (t->n < b.N + 1) return VC_E_INVALID;
    if (domain_error(b)) return VC_E_DOMAIN;
    if (b.prior()) {
        const double c0 = host_timing() ? clock_us() : 0.0;
        challenges_host(b, chal);
        if (host_timing()) laps->host_tr = clock_us() - c0;
    }
    return fold_device(ctx, t, b, rho, chal, S, malformed, laps);
}
}  // namespace

}  // namespace vk

using namespace vk;

extern "C" int vc_ipa_batch_challenge(const uint8_t seed[32], uint64_t* rho_fr) {
    if (!seed || !rho_fr) return VC_E_INVALID;
    static const char dst[] = "vkzg-ipa-batch";
    mont_to_canon<BN254Fr>(hash_to_fr(seed, 32, reinterpret_cast<const uint8_t*>(dst), sizeof dst - 1), rho_fr);
    return VC_OK;
}

extern "C" int vc_ipa_challenges_many(vc_ctx* ctx, size_t N, size_t n, const uint64_t* com_xy, const uint8_t* com_inf,
                                      const uint64_t* points, const uint64_t* y, const uint64_t* l_xy,
                                      const uint8_t* l_inf, const uint64_t* r_xy, const uint8_t* r_inf, uint64_t* out) {
    const Batch b{N, n, log2_of(N), com_xy, points, l_xy, r_xy, nullptr, y, com_inf, l_inf, r_inf, nullptr};
    if ((ctx && ctx->curve != VC_CURVE_BN254) || !n_ok(N, size_t(1) << 28) || !arrays_ok(b, false) || (n && !out))
        return VC_E_INVALID;
    if (n == 0) return VC_OK;
    if (ctx) {
        Guard g(ctx);
        return challenges_device(ctx, b, out);
    }
    std::vector<Fr> chal;
    challenges_host(b, chal);
    pool_for(0, chal.size(), 1024, [&](size_t i) { mont_to_canon<BN254Fr>(chal[i], out + 4 * i); });
    return VC_OK;
}

extern "C" int vc_ipa_batch_fold(vc_ctx* ctx, int table, const uint64_t* crs_xy, size_t N, size_t n,
                                 const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* points,
                                 const uint64_t* l_xy, const uint8_t* l_inf, const uint64_t* r_xy, const uint8_t* r_inf,
                                 const uint64_t* tip, const uint64_t* y, vc_transcript** transcripts,
                                 const uint64_t* rho_fr, uint64_t* s_xy, uint8_t* s_inf, int* malformed) {
    const Batch b{N, n, log2_of(N), com_xy, points, l_xy, r_xy, tip, y, com_inf, l_inf, r_inf, transcripts};
    if (!rho_fr || !s_xy || !s_inf || !malformed) return VC_E_INVALID;
    if (!ate::words_below_modulus<BN254Fr>(w32(rho_fr))) return VC_E_INVALID;
    G1A S = BN254G1::zero();  // (n = 0: the sum is empty)
    bool bad = false;
    Laps laps;
    if (n) {
        VK_TRY(fold_impl(ctx, table, crs_xy, b, canon_to_mont<BN254Fr>(rho_fr), &S, &bad, &laps));
    } else if ((ctx ? ctx->curve != VC_CURVE_BN254 : !crs_xy) || !n_ok(N, IB_N_MAX)) {
        return VC_E_INVALID;
    }
    *malformed = bad ? 1 : 0;
    if (bad) return VC_OK;
    return acc_to_affine_batch(VC_CURVE_BN254, reinterpret_cast<const uint32_t*>(&S), 1, s_xy, s_inf);
}

extern "C" int vc_ipa_verify_batch(vc_ctx* ctx, int table, size_t N, size_t n, const uint64_t* com_xy,
                                   const uint8_t* com_inf, const uint64_t* points, const uint64_t* l_xy,
                                   const uint8_t* l_inf, const uint64_t* r_xy, const uint8_t* r_inf, const uint64_t* tip,
                                   const uint64_t* y, vc_transcript** transcripts, const uint8_t* seed32, int* result,
                                   uint8_t* results) {
    const Batch b{N, n, log2_of(N), com_xy, points, l_xy, r_xy, tip, y, com_inf, l_inf, r_inf, transcripts};
    if (!ctx || ctx->curve != VC_CURVE_BN254 || !result || !n_ok(N, IB_N_MAX) || !arrays_ok(b, true)) return VC_E_INVALID;
    {
        Guard g(ctx);
        Table* t = ctx->table(table);
        if (!t) return VC_E_TABLE;
        if (t->n < N + 1) return VC_E_INVALID;
    }
    if (n == 0) {
        *result = 1;
        return VC_OK;
    }
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
    VK_TRY(vc_ipa_batch_challenge(seed, rho_c));
    // prior transcripts advance once, in the fold; a rejecting call's per-opening pass runs on copies
    // of their states before it
    struct Copies {
        std::vector<vc_transcript*> v;
        ~Copies() {
            for (vc_transcript* t : v) vc_transcript_free(t);
        }
    } copies;
    if (results && b.prior()) {
        copies.v.resize(n, nullptr);
        for (size_t p = 0; p < n; p++)
            if (transcripts[p]) copies.v[p] = vc_transcript_clone(transcripts[p]);
    }
    const double c0 = host_timing() ? clock_us() : 0.0;
    G1A S;
    bool bad = false;
    Laps laps;
    VK_TRY(fold_impl(ctx, table, nullptr, b, canon_to_mont<BN254Fr>(rho_c), &S, &bad, &laps));
    const bool ok = !bad && BN254G1::is_zero(S);
    if (host_timing())
        fprintf(stderr,
                "[ipa_verify_batch] n=%zu N=%zu chunks=%zu: host transcripts %.1f us, upload %.1f us, transcripts %.1f us, "
                "prep %.1f us, field %.1f us, msm %.1f us, fixed commit %.1f us, call %.1f us\n",
                n, N, laps.chunks, laps.host_tr, laps.upload, laps.transcripts, laps.prep, laps.field, laps.msm,
                laps.fixed, clock_us() - c0);
    *result = ok ? 1 : 0;
    if (!results) return VC_OK;
    if (ok) {
        memset(results, 1, n);
        return VC_OK;
    }
    return vc_ipa_verify_many(ctx, table, N, n, com_xy, com_inf, points, l_xy, l_inf, r_xy, r_inf, tip, y,
                              copies.v.empty() ? nullptr : copies.v.data(), results);
}

// Multiproof prover and verifier (reference: vector-commit/src/multiproof.rs).
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <system_error>
#include <thread>

#include "ff29.hpp"
#include "poly.hpp"
#include "protocol.hpp"

namespace vk {

// ---------------------------------------------------------------- multiproof kernels
// one block per z group: q_z[k] = (S_z[k] - S_z[z]) * inv[k] (k != z),
// q_z[z] = -w^-z sum_{k != z} q_z[k] w^k   (divide_by_vanishing, lagrange_basis.rs:91-119)
// 1/(w^k - w^z) = w^-z / (w^(k-z) - 1) = pw_inv[z] inv1[(k - z) mod N]: the per-domain cached
// inv1 table replaces a Z x N denominator pass and its batch inversion (and host round trip)
__global__ void __launch_bounds__(256) k_mp_quot(const fe<F>* __restrict__ S, const fe<F>* __restrict__ inv1,
                                                const fe<F>* __restrict__ pw, const fe<F>* __restrict__ pw_inv,
                                                const uint32_t* __restrict__ zval, size_t N, fe<F>* __restrict__ Q) {
    __shared__ fe<F> sh[256];
    uint32_t zi = blockIdx.x;
    uint32_t z = zval[zi];
    const fe<F>* Sz = S + (size_t)zi * N;
    fe<F> fz = Sz[z];
    const fe<F> wmz = pw_inv[z];
    fe<F> acc = fe_zero<F>();
    for (size_t k = threadIdx.x; k < N; k += 256) {
        fe<F> q = fe_zero<F>();
        if (k != z) {
            q = fe_mul<F>(fe_mul<F>(fe_sub<F>(Sz[k], fz), wmz), inv1[(k + N - z) & (N - 1)]);
            acc = fe_add<F>(acc, fe_mul<F>(q, pw[k]));
        }
        Q[(size_t)zi * N + k] = q;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] = fe_add<F>(sh[threadIdx.x], sh[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) Q[(size_t)zi * N + z] = fe_neg<F>(fe_mul<F>(sh[0], pw_inv[z]));
}

// g[k] = sum_z Q[z][k], h[k] = sum_z invt_z[z] S[z][k], hmg = h - g (with invt_z and hmg): a block per MP_CB_K columns, its 256
// threads split the Z rows MP_CB_R ways (row-groups strided by MP_CB_R), partials added in LDS --
// the one-thread-per-column form ran 256 dependent multiplies per thread on 4 waves (~0.15 ms of
// the multiproof finish at N = 256)
constexpr uint32_t MP_CB_K = 16, MP_CB_R = 16;
__global__ void __launch_bounds__(256) k_mp_combine(const fe<F>* __restrict__ S, const fe<F>* __restrict__ Q,
                                                    const fe<F>* __restrict__ invt_z, size_t N, uint32_t Z,
                                                    fe<F>* __restrict__ g, fe<F>* __restrict__ h,
                                                    fe<F>* __restrict__ hmg) {
    __shared__ fe<F> pg[MP_CB_R][MP_CB_K], ph[MP_CB_R][MP_CB_K];
    const uint32_t kc = threadIdx.x % MP_CB_K, rg = threadIdx.x / MP_CB_K;
    const size_t k = (size_t)blockIdx.x * MP_CB_K + kc;
    fe<F> gg = fe_zero<F>(), hh = fe_zero<F>();
    if (k < N)
        for (uint32_t zi = rg; zi < Z; zi += MP_CB_R) {
            gg = fe_add<F>(gg, Q[(size_t)zi * N + k]);
            if (invt_z) hh = fe_add<F>(hh, fe_mul<F>(invt_z[zi], S[(size_t)zi * N + k]));
        }
    pg[rg][kc] = gg;
    ph[rg][kc] = hh;
    __syncthreads();
    if (rg == 0 && k < N) {
        for (uint32_t j = 1; j < MP_CB_R; j++) {
            gg = fe_add<F>(gg, pg[j][kc]);
            if (invt_z) hh = fe_add<F>(hh, ph[j][kc]);
        }
        g[k] = gg;
        if (invt_z) h[k] = hh;
        if (invt_z && hmg) hmg[k] = fe_sub<F>(hh, gg);
    }
}

// the multiproof transcript's records "C" ++ compressed(C_i) ++ "z" ++ le64(z_i) ++ "y" ++ le(y_i)
// (multiproof.rs:106-113) for queries [lo, hi) into out: 75 bytes at offset 75 i, so the records
// are written straight into the transcript on up to 16 host threads (the point compression is the
// costly part); the SHA-256 over them stays serial
static void mp_records(const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z, const uint64_t* y,
                       size_t lo, size_t hi, uint8_t* out) {
    constexpr size_t REC = 75;
    static const uint64_t zero[8] = {0};
    for (size_t i = lo; i < hi; i++) {
        uint8_t* o = out + REC * (i - lo);
        o[0] = 'C';
        compress_g1(com_inf[i] ? zero : com_xy + 8 * i, com_inf[i] != 0, o + 1);
        o[33] = 'z';
        for (int k = 0; k < 8; k++) o[34 + k] = (uint8_t)(z[i] >> (8 * k));
        o[42] = 'y';
        memcpy(o + 43, y + 4 * i, 32);
    }
}

static std::vector<Fr> invert_domain_at(const Fr& t, size_t N) {  // utils.rs:57-62 (integer i)
    std::vector<Fr> d(N);
    for (size_t i = 0; i < N; i++) d[i] = fe_sub<F>(t, fr_u64(i));
    return host_batch_inv(d);
}

// ---- multiproof prover in three phases (multiproof.rs:99-176), so the Q x N field phase can
// be sharded over GPUs with one exchange:
//   mp_begin       host: transcript over all (C, z, y) and the challenge r        (:106-114)
//   mp_accumulate  device, per query shard [first, first + Qs): dense per-z sums
//                  S[z][k] = sum_{i: z_i = z} r^i f_i[k]  (canonical, N x N)      (:116-127)
//   mp_finish      device + host: sum of the shards' S, quotients, g, D, t, h, E and the
//                  inner proof                                                     (:129-175)
// Grouping queries by z and summing per group first is the same field arithmetic as the
// reference's per-group LagrangeBasis sums; rows of z with no query are zero and add nothing.
// pool_ok = false: the call's own filler thread feeds the hash (scheme_host.cpp
// transcript_digest_records) -- mp_prove_many's transcript workers and vc_multiproof_begin, whose
// callers run several transcripts at once: on the shared host pool their record filling queued
// on the pool's one-loop lock. No transcript is returned on error (VC_E_OOM if the hashing threw).
static int mp_begin(size_t N, size_t Q, const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z,
                    const uint64_t* y, vc_transcript** tr_out, Fr* r_out, bool pool_ok = true) {
    *tr_out = nullptr;
    if (!is_pow2(N) || Q == 0) return VC_E_INVALID;
    for (size_t i = 0; i < Q; i++)
        if (z[i] >= N) return VC_E_DOMAIN;
    // the records stream into the hash (never stored whole: transcript_digest_records)
    vc_transcript* tr = vc_transcript_new("multiproof");
    try {
        *r_out = transcript_digest_records(
            tr, Q, 75, [&](size_t lo, size_t hi, uint8_t* out) { mp_records(com_xy, com_inf, z, y, lo, hi, out); },
            "r", pool_ok && Q >= 8192);
    } catch (...) {  // the filler thread's failure, rethrown by the digest
        vc_transcript_free(tr);
        return VC_E_OOM;
    }
    *tr_out = tr;
    return VC_OK;
}

// distinct query points, sorted; VC_E_DOMAIN for a z outside the domain (the reference indexes
// the Lagrange evaluations with it and panics). The accumulate / finish entry points take z
// from the caller again, so every path validates here (a bitmap of N, not of max z).
static int mp_points(size_t N, size_t Q, const uint64_t* z, std::vector<uint32_t>* out) {
    if (N == 0 || N > (size_t(1) << 28)) return VC_E_INVALID;  // BN254 Fr has 2-adicity 28
    std::vector<uint8_t> seen(N, 0);
    for (size_t i = 0; i < Q; i++) {
        if (z[i] >= N) return VC_E_DOMAIN;
        seen[z[i]] = 1;
    }
    out->clear();
    for (size_t k = 0; k < N; k++)
        if (seen[k]) out->push_back((uint32_t)k);
    return VC_OK;
}

// rp[i] = r^(first + i) as radix-2^29 Montgomery limbs (x R', R' = 2^261, ff29.hpp), canonical, at
// a stride of MP_RP_WORDS words (the chunk kernel reads them as uniform scalar loads)
using P29 = F29BN254Fr;
constexpr uint32_t MP_RP_WORDS = 16;
__global__ void k_mp_rpow(Fr r, size_t first, size_t n, uint32_t* __restrict__ rp) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr acc = fe_one<F>(), b = r;
    size_t e = first + i;
    while (e) {
        if (e & 1) acc = fe_mul<F>(acc, b);
        e >>= 1;
        if (e) b = fe_sqr<F>(b);
    }
    const f29<P29> v = canon29<P29>(from_mont32<P29, F>(acc));
#pragma unroll
    for (int j = 0; j < P29::L; j++) rp[i * MP_RP_WORDS + j] = v.v[j];
}

// one block per (k block, chunk c of <= CH queries of one z): partial[c][k] =
// sum over sorted positions [be[2c], be[2c+1]) of r^i f_i[k] (f canonical; partial canonical).
// HBM-bound stream of the Q x N evaluations (the r^i are uniform over a block). Radix-2^29 with
// lazy reduction: the products f_i[k] (r^i R') of LZ queries add into 17 unsigned 64-bit columns
// (<= 9 products of < 2^58 per query and column) and ONE Montgomery reduction (9 rows, <= 9 more
// products per column) serves them: (9 LZ + 9) 2^58 + 2^35 < 2^64 for LZ <= 6 -- ~100-120
// instructions per element instead of a full 32-bit-limb multiply (~270) and an add. A block
// result is below (LZ p^2 / R' + p) = (1 + LZ 2^-7) p; the block results are added with one
// conditional subtraction each, so the running total stays below 2 p over a chunk of CH / LZ
// blocks, and a last one makes it canonical.
// Shapes (LZ x CH) measured: 3 x 16 (round 4's first), 4 x 16, 4 x 32, 6 x 24; 4 x 16 is built.
constexpr uint32_t MP_LZ_MAX = 6;
// one block of <= LZ queries: products into the columns, one Montgomery reduction
template <uint32_t LZ>
__device__ __forceinline__ f29<P29> mp_block(const uint4 (&v)[LZ][2], const uint32_t (&qi)[LZ], uint32_t nq,
                                             const uint32_t* __restrict__ rp) {
    static_assert(LZ <= MP_LZ_MAX, "column bound");
    constexpr int L = P29::L;
    uint64_t t[2 * L];  // 2L - 1 product columns and the reduction's top carry
#pragma unroll
    for (int x = 0; x < 2 * L; x++) t[x] = 0;
#pragma unroll
    for (uint32_t j = 0; j < LZ; j++) {
        if (j >= nq) break;
        const uint32_t w[8] = {v[j][0].x, v[j][0].y, v[j][0].z, v[j][0].w, v[j][1].x, v[j][1].y, v[j][1].z, v[j][1].w};
        const f29<P29> a = unpack29<P29>(w);
        const uint32_t* b = rp + (size_t)qi[j] * MP_RP_WORDS;
#pragma unroll
        for (int y = 0; y < L; y++) {
            const uint32_t by = b[y];
#pragma unroll
            for (int x = 0; x < L; x++) t[x + y] += (uint64_t)a.v[x] * by;
        }
    }
    // Montgomery reduction of the columns (separated operand scanning): t / R' mod p
#pragma unroll
    for (int i = 0; i < L; i++) {
        const uint32_t m = ((uint32_t)t[i] * P29::inv) & M29;
#pragma unroll
        for (int j = 0; j < L; j++) t[i + j] += (uint64_t)m * P29::p(j);
        t[i + 1] += t[i] >> 29;
    }
    f29<P29> r;  // columns L .. 2L - 1 are the reduced value (as sqr29)
#pragma unroll
    for (int j = L; j < 2 * L - 1; j++) {
        t[j + 1] += t[j] >> 29;
        r.v[j - L] = (uint32_t)t[j] & M29;
    }
    r.v[L - 1] = (uint32_t)t[2 * L - 1];
    return r;
}

// NT = 1: non-temporal loads (the evaluations are read once per proof)
template <int NT, uint32_t LZ>
__device__ __forceinline__ void mp_load(const uint32_t* __restrict__ f, const uint32_t* __restrict__ order, uint32_t u,
                                        uint32_t nq, size_t N, size_t k, uint4 (&v)[LZ][2], uint32_t (&qi)[LZ]) {
#pragma unroll
    for (uint32_t j = 0; j < LZ; j++) {
        qi[j] = j < nq ? order[u + j] : 0u;
        if (j < nq) {
            const uint4* src = reinterpret_cast<const uint4*>(f + ((size_t)qi[j] * N + k) * 8);
            if constexpr (NT) {
                typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                const u32x4* s4 = reinterpret_cast<const u32x4*>(src);
                const u32x4 a = __builtin_nontemporal_load(s4), b = __builtin_nontemporal_load(s4 + 1);
                v[j][0] = make_uint4(a.x, a.y, a.z, a.w);
                v[j][1] = make_uint4(b.x, b.y, b.z, b.w);
            } else {
                v[j][0] = src[0];
                v[j][1] = src[1];
            }
        }
    }
}

// PF = 1: the next block's loads are issued before the current block's arithmetic, so every lane
// keeps LZ x 32 B in flight while it multiplies (measured slower; not instantiated)
template <int NT, uint32_t LZ, uint32_t CH, int PF = 0>
__global__ void __launch_bounds__(256) k_mp_chunk(const uint32_t* __restrict__ f, const uint32_t* __restrict__ rp,
                                                 const uint32_t* __restrict__ order, const uint32_t* __restrict__ be,
                                                 size_t N, uint32_t kblk, Fr* __restrict__ partial) {
    const uint32_t c = blockIdx.x / kblk;  // 1-D grid: chunks can outnumber gridDim.y's 65535
    const size_t k = (size_t)(blockIdx.x % kblk) * blockDim.x + threadIdx.x;
    if (k >= N) return;
    const uint32_t u0 = be[2 * c], cnt = be[2 * c + 1] - u0;
    f29<P29> total = zero29<P29>();
    uint4 v[LZ][2];
    uint32_t qi[LZ];
    if constexpr (PF) {
        if (cnt > 0) mp_load<NT, LZ>(f, order, u0, min(cnt, LZ), N, k, v, qi);
    }
#pragma unroll
    for (uint32_t h = 0; h < CH; h += LZ) {
        if (h >= cnt) break;
        const uint32_t nq = min(cnt - h, LZ);
        if constexpr (PF) {
            uint4 w[LZ][2];
            uint32_t qw[LZ];
            if (h + LZ < cnt) mp_load<NT, LZ>(f, order, u0 + h + LZ, min(cnt - h - LZ, LZ), N, k, w, qw);
            const f29<P29> r = mp_block<LZ>(v, qi, nq, rp);
            total = csub29<P29>(carry29<P29>(add29_raw<P29>(total, r)));
#pragma unroll
            for (uint32_t j = 0; j < LZ; j++) {
                v[j][0] = w[j][0];
                v[j][1] = w[j][1];
                qi[j] = qw[j];
            }
        } else {
            mp_load<NT, LZ>(f, order, u0 + h, nq, N, k, v, qi);
            const f29<P29> r = mp_block<LZ>(v, qi, nq, rp);
            total = csub29<P29>(carry29<P29>(add29_raw<P29>(total, r)));
        }
    }
    total = csub29<P29>(carry29<P29>(total));
    pack29<P29>(total, partial[(size_t)c * N + k].v);
}

// S[row][k] = sum of the partials of the row's chunks [zc[row], zc[row+1])
__global__ void k_mp_chunk_reduce(const Fr* __restrict__ partial, const uint32_t* __restrict__ zc, size_t N,
                                  uint32_t kblk, Fr* __restrict__ S) {
    const uint32_t zz = blockIdx.x / kblk;
    const size_t k = (size_t)(blockIdx.x % kblk) * blockDim.x + threadIdx.x;
    if (k >= N) return;
    Fr acc = fe_zero<F>();
    for (uint32_t c = zc[zz]; c < zc[zz + 1]; c++) acc = fe_add<F>(acc, partial[(size_t)c * N + k]);
    S[(size_t)zz * N + k] = acc;
}

// rows of S are the distinct query points zval (sorted, over ALL queries -- every shard
// uses the same rows so the shards' S add up); Z = zval.size().
// The shard's plan depends on z alone (not on the challenge r): rows, the counting sort of the
// queries by row, chunks of <= CH queries inside a row, and their uploads -- so vc_multiproof_begin_accumulate
// builds it while the host transcript that yields r runs on another thread.
struct MpPlan {
    size_t Qs = 0, first = 0, Z = 0;
    uint32_t nch = 0;
    std::vector<uint32_t> order, be, zc;  // alive until mp_run's sync (async uploads)
    DevBuf d_rp, d_order, d_be, d_zc, d_part;
    explicit MpPlan(vc_ctx* ctx) : d_rp(ctx), d_order(ctx), d_be(ctx), d_zc(ctx), d_part(ctx) {}
};
// block / chunk shape of k_mp_chunk, LZ x CH = 4 x 16: 0.125-0.129 ms against 0.128-0.131 for 3 x 16
// (profiles/r04/mp_shape_ab.txt)
constexpr uint32_t MP_LZ = 4, MP_CHUNK = 16;
static int mp_plan(vc_ctx* ctx, size_t N, size_t Qs, const uint64_t* z, size_t first, const std::vector<uint32_t>& zval,
                   MpPlan* pl) {
    hipStream_t st = ctx->stream;
    const size_t Z = zval.size();
    pl->Qs = Qs;
    pl->first = first;
    pl->Z = Z;
    if (Qs == 0) return VC_OK;
    // row of each query: a table over the domain (z < N, checked by mp_points over all queries)
    std::vector<uint32_t> row_of(N, 0xffffffffu), row(Qs);
    for (size_t k = 0; k < Z; k++) row_of[zval[k]] = (uint32_t)k;
    for (size_t i = 0; i < Qs; i++) {
        if (z[i] >= N || row_of[z[i]] == 0xffffffffu) return VC_E_DOMAIN;
        row[i] = row_of[z[i]];
    }
    // counting sort of the shard's queries by row, then chunks of <= MP_CHUNK queries
    std::vector<uint32_t> cnt(Z + 1, 0);
    pl->order.resize(Qs);
    for (size_t i = 0; i < Qs; i++) cnt[row[i] + 1]++;
    for (size_t k = 0; k < Z; k++) cnt[k + 1] += cnt[k];
    {
        std::vector<uint32_t> pos(cnt.begin(), cnt.end() - 1);
        for (size_t i = 0; i < Qs; i++) pl->order[pos[row[i]]++] = (uint32_t)i;
    }
    // chunks of <= MP_CHUNK queries inside one row; zc[row] = first chunk of the row
    pl->be.clear();
    pl->zc.assign(Z + 1, 0);
    for (size_t k = 0; k < Z; k++) {
        pl->zc[k] = (uint32_t)(pl->be.size() / 2);
        for (uint32_t u = cnt[k]; u < cnt[k + 1]; u += MP_CHUNK) {
            pl->be.push_back(u);
            pl->be.push_back(std::min<uint32_t>(u + MP_CHUNK, cnt[k + 1]));
        }
    }
    pl->nch = (uint32_t)(pl->be.size() / 2);
    pl->zc[Z] = pl->nch;
    VK_TRY(pl->d_rp.ensure(Qs * MP_RP_WORDS * 4));
    VK_TRY(pl->d_order.ensure(Qs * 4));
    VK_TRY(pl->d_be.ensure(pl->be.size() * 4));
    VK_TRY(pl->d_zc.ensure((Z + 1) * 4));
    VK_TRY(pl->d_part.ensure(std::max<size_t>(pl->nch, 1) * N * 32));
    VK_CHECK_HIP(hipMemcpyAsync(pl->d_order.p, pl->order.data(), Qs * 4, hipMemcpyHostToDevice, st));
    VK_CHECK_HIP(hipMemcpyAsync(pl->d_be.p, pl->be.data(), pl->be.size() * 4, hipMemcpyHostToDevice, st));
    VK_CHECK_HIP(hipMemcpyAsync(pl->d_zc.p, pl->zc.data(), (Z + 1) * 4, hipMemcpyHostToDevice, st));
    return VC_OK;
}
static int mp_run(vc_ctx* ctx, size_t N, const void* d_data, const Fr& r, MpPlan& pl, void* d_S) {
    hipStream_t st = ctx->stream;
    const size_t Qs = pl.Qs, Z = pl.Z;
    if (Qs == 0) {  // an empty shard contributes zero sums (synchronous like every ABI call)
        VK_CHECK_HIP(hipMemsetAsync(d_S, 0, Z * N * 32, st));
        VK_CHECK_HIP(hipStreamSynchronize(st));
        return VC_OK;
    }
    VK_LAUNCH(ctx, "mp_rpow", k_mp_rpow, (Qs + 255) / 256, 256, 0, r, pl.first, Qs, pl.d_rp.as<uint32_t>());
    const uint32_t kblk = (uint32_t)((N + 255) / 256);
    // non-temporal loads: 0.119-0.121 ms (4.43-4.51 TB/s) against 0.125-0.127 at 2^16 x 256
    // (profiles/r04/mp_nt_ab.txt)
    VK_LAUNCH(ctx, "mp_chunk", (k_mp_chunk<1, MP_LZ, MP_CHUNK>), (size_t)pl.nch * kblk, 256, 0, reinterpret_cast<const uint32_t*>(d_data),
              pl.d_rp.as<uint32_t>(), pl.d_order.as<uint32_t>(), pl.d_be.as<uint32_t>(), N, kblk, pl.d_part.as<Fr>());
    VK_LAUNCH(ctx, "mp_chunk_reduce", k_mp_chunk_reduce, Z * kblk, 256, 0, pl.d_part.as<Fr>(), pl.d_zc.as<uint32_t>(),
              N, kblk, reinterpret_cast<Fr*>(d_S));
    VK_CHECK_HIP(hipStreamSynchronize(st));  // the plan's host vectors may die after this
    return VC_OK;
}
static int mp_accumulate(vc_ctx* ctx, size_t N, size_t Qs, const void* d_data, const uint64_t* z, const Fr& r,
                         size_t first, const std::vector<uint32_t>& zval, void* d_S) {
    MpPlan pl(ctx);
    const int st = mp_plan(ctx, N, Qs, z, first, zval, &pl);
    if (st != VC_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // uploads from the plan's vectors may be queued
        return st;
    }
    return mp_run(ctx, N, d_data, r, pl, d_S);
}

// mp_begin on a helper thread while this thread runs `overlap` (the shard's plan; mp_prove also
// the evaluations' upload): the serial SHA-256 transcript is the longest host step of a multiproof
// (2.6 ms at Q = 2^16), and neither the plan nor the upload needs its challenge. Falls back to
// running both in turn if no thread can be started. On failure no transcript is returned and the
// stream is synchronised (uploads that the overlap queued may read the caller's vectors).
template <class Fn>
static int mp_begin_overlapped(vc_ctx* ctx, size_t N, size_t Q, const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z,
                               const uint64_t* y, vc_transcript** tr_out, Fr* r_out, Fn overlap) {
    int st_b = VC_E_INVALID, st_o = VC_OK;
    *tr_out = nullptr;
    auto guarded = [&]() -> int {  // the helper must be joined whatever the overlap does
        try {
            return overlap();
        } catch (...) {
            return VC_E_OOM;
        }
    };
    // the overlapped transcript fills its records on its own filler thread, not the host pool the
    // overlapped planning uses: single proof 3.99-4.15 -> 3.84-3.89 ms (`profiles/r04/mp_begin_pool/`)
    std::thread th;
    try {
        th = std::thread([&] {
            try {
                st_b = mp_begin(N, Q, com_xy, com_inf, z, y, tr_out, r_out, /*pool_ok=*/false);
            } catch (...) {  // nothing may leave a thread function
                st_b = VC_E_OOM;
            }
        });
    } catch (const std::system_error&) {  // no thread: one after the other
        st_b = mp_begin(N, Q, com_xy, com_inf, z, y, tr_out, r_out);
        if (st_b == VC_OK) st_o = guarded();
    }
    if (th.joinable()) {
        st_o = guarded();
        th.join();
    }
    if (st_b != VC_OK || st_o != VC_OK) {
        if (*tr_out) vc_transcript_free(*tr_out);
        *tr_out = nullptr;
        (void)hipStreamSynchronize(ctx->stream);
        return st_b != VC_OK ? st_b : st_o;
    }
    return VC_OK;
}

// S = sum over G shards (canonical) -> Montgomery
__global__ void k_mp_sum_parts(const Fr* __restrict__ parts, int G, size_t NN, Fr* __restrict__ S) {
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= NN) return;
    Fr acc = parts[g];
    for (int k = 1; k < G; k++) acc = fe_add<F>(acc, parts[(size_t)k * NN + g]);
    S[g] = fe_to_mont<F>(acc);
}

// ---- the middle of a multiproof (multiproof.rs:129-160) in two stages over one proof's buffers:
// mp_finish runs each once, mp_prove_many once per proof around its batched D and E commits.
struct MpMid {  // the rows' points, their summed S (Montgomery), the quotients, 1 / (t - z)
    DevBuf zv, S, Q, it;
    explicit MpMid(vc_ctx* ctx) : zv(ctx), S(ctx), Q(ctx), it(ctx) {}
    int ensure(size_t Z, size_t N) {
        VK_TRY(zv.ensure(Z * 4));
        VK_TRY(S.ensure(Z * N * 32));
        VK_TRY(Q.ensure(Z * N * 32));
        return it.ensure(Z * 32);
    }
};
struct MpDomain {  // domain_tables of the proofs' N; where null, mp_stage_g fetches them
    const fe<F>*pw = nullptr, *pwi = nullptr, *inv1 = nullptr;
};
static int mp_combine(vc_ctx* ctx, size_t N, uint32_t Z, MpMid& m, const fe<F>* invt, fe<F>* d_g, fe<F>* d_h,
                      fe<F>* d_hmg) {
    VK_LAUNCH(ctx, "mp_combine", k_mp_combine, (N + MP_CB_K - 1) / MP_CB_K, 256, 0, m.S.as<fe<F>>(), m.Q.as<fe<F>>(), invt,
              N, Z, d_g, d_h, d_hmg);
    return VC_OK;
}
// stage 1, sums -> quotients -> g: S = the sum of the G shards' parts, the rows' quotients, g
static int mp_stage_g(vc_ctx* ctx, size_t N, const std::vector<uint32_t>& zval, const void* d_S_parts, int G,
                      MpDomain& dom, MpMid& m, fe<F>* d_g, fe<F>* d_h) {
    const uint32_t Z = (uint32_t)zval.size();
    VK_CHECK_HIP(hipMemcpyAsync(m.zv.p, zval.data(), Z * 4, hipMemcpyHostToDevice, ctx->stream));
    VK_LAUNCH(ctx, "mp_sum_parts", k_mp_sum_parts, ((size_t)Z * N + 255) / 256, 256, 0,
              reinterpret_cast<const Fr*>(d_S_parts), G, (size_t)Z * N, m.S.as<Fr>());
    if (!dom.pw) VK_TRY(domain_tables<F>(ctx, bn254_group_gen(N), N, &dom.pw, &dom.pwi, &dom.inv1));
    VK_LAUNCH(ctx, "mp_quot", k_mp_quot, Z, 256, 0, m.S.as<fe<F>>(), dom.inv1, dom.pw, dom.pwi, m.zv.as<uint32_t>(), N,
              m.Q.as<fe<F>>());
    return mp_combine(ctx, N, Z, m, nullptr, d_g, d_h, nullptr);
}
// stage 2, t -> h: the rows' 1 / (t - z), z an integer (utils.rs:57-62), gathered into invz -- Z
// host values the caller keeps alive until the stream has passed their upload -- then h (d_hmg:
// null, or where h - g goes)
static int mp_stage_h(vc_ctx* ctx, size_t N, const std::vector<uint32_t>& zval, const Fr& tt, Fr* invz, MpMid& m,
                      fe<F>* d_g, fe<F>* d_h, fe<F>* d_hmg) {
    const uint32_t Z = (uint32_t)zval.size();
    const std::vector<Fr> invs = invert_domain_at(tt, N);
    for (uint32_t k = 0; k < Z; k++) invz[k] = invs[zval[k]];
    VK_CHECK_HIP(hipMemcpyAsync(m.it.p, invz, Z * 32, hipMemcpyHostToDevice, ctx->stream));
    return mp_combine(ctx, N, Z, m, m.it.as<fe<F>>(), d_g, d_h, d_hmg);
}
// the inner proofs of P prepared multiproofs (h - g, E - D, t, the transcript after "E"): one
// batched IPA, or P KZG openings through canonical words
static int mp_inner_proofs(vc_ctx* ctx, int scheme, Table* t, size_t N, const std::vector<std::vector<Fr>>& hmg,
                           const std::vector<Acc>& mc, const std::vector<Fr>& tt, vc_transcript** trs,
                           vc_ipa_proof* ipa_proofs, uint64_t* kzg_xy, uint8_t* kzg_inf, uint64_t* kzg_y) {
    if (scheme == 0) return ipa_prove_impl(ctx, t, N, hmg, mc, tt, trs, ipa_proofs);
    std::vector<uint64_t> ev(N * 4);
    for (size_t p = 0; p < hmg.size(); p++) {
        for (size_t k = 0; k < N; k++) canon_of(hmg[p][k], &ev[4 * k]);
        uint64_t tc[4];
        canon_of(tt[p], tc);
        VK_TRY(kzg_open_bn254(ctx, t, N, ev.data(), tc, kzg_xy + p * 8, kzg_inf + p, kzg_y + p * 4));
    }
    return VC_OK;
}
// the multiproof ABI's scheme and the output pointers of its P proofs
static bool mp_outputs_ok(int scheme, size_t P, const vc_ipa_proof* ipa_proofs, const uint64_t* kzg_xy,
                          const uint8_t* kzg_inf, const uint64_t* kzg_y) {
    if (scheme == 1) return P == 0 || (kzg_xy && kzg_inf && kzg_y);
    if (scheme != 0) return false;
    for (size_t p = 0; p < P; p++)
        if (!ipa_proofs || !proof_ok(&ipa_proofs[p])) return false;
    return true;
}

static int mp_finish(vc_ctx* ctx, int scheme, Table* t, size_t N, const std::vector<uint32_t>& zval,
                     const void* d_S_parts, int G, vc_transcript* tr, uint64_t* d_xy, uint8_t* d_inf,
                     vc_ipa_proof* ipa_proof, uint64_t* kzg_xy, uint8_t* kzg_inf, uint64_t* kzg_y) {
    if (!is_pow2(N) || G < 1 || zval.empty()) return VC_E_INVALID;
    hipStream_t st = ctx->stream;
    // verbose(): phase laps on stderr (with a stream sync at each: diagnostics only)
    auto tic = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!verbose()) return;
        (void)hipStreamSynchronize(st);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[mp_finish] %s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - tic).count());
        tic = now;
    };
    const uint32_t Z = (uint32_t)zval.size();
    MpMid mid(ctx);
    DevBuf d_g(ctx), d_h(ctx);
    VK_TRY(mid.ensure(Z, N));
    VK_TRY(d_g.ensure(N * 32));
    VK_TRY(d_h.ensure(N * 32));
    MpDomain dom;
    VK_TRY(mp_stage_g(ctx, N, zval, d_S_parts, G, dom, mid, d_g.as<fe<F>>(), d_h.as<fe<F>>()));
    // D = commit(g) and E = commit(h) read g / h in device memory (Montgomery scalars) on the latency
    // path, which completes by polled flags: no read-back of g or h and no stream wait; h - g (the
    // inner proof's data) is made on the device and copied into page-locked memory ahead of the E
    // commit, so it is on the host when E's flags are
    auto commit_dev = [&](const void* d_sc, uint64_t* xy, uint8_t* inf) -> int {
        VK_TRY(ctx->ws[WS_MISC].ensure(65));
        uint8_t* dxy_ = ctx->ws[WS_MISC].as<uint8_t>();
        bool on_host = false;
        VK_TRY(msm_batch_run(ctx, t, N, d_sc, 1, 1, dxy_, dxy_ + 64, xy, inf, &on_host, nullptr, nullptr));
        if (on_host) return VC_OK;
        uint8_t tmp[65];
        VK_CHECK_HIP(hipMemcpyAsync(tmp, dxy_, 65, hipMemcpyDeviceToHost, st));
        VK_CHECK_HIP(hipStreamSynchronize(st));
        memcpy(xy, tmp, 64);
        *inf = tmp[64];
        return VC_OK;
    };
    lap("sums, quotients, g");
    uint64_t dxy[8];
    uint8_t dinf;
    VK_TRY(commit_dev(d_g.p, dxy, &dinf));
    lap("D");
    transcript_append_point(tr, dxy, dinf, "D");
    std::vector<Fr> tt(1, transcript_digest(tr, "t"));
    // 1 / (t - z) staged in page-locked memory, behind the N words h - g comes back into
    VK_TRY(ctx->pin_mp.ensure(N * 32 + (size_t)Z * 32));
    uint8_t* pin_hmg = static_cast<uint8_t*>(ctx->pin_mp.p);
    DevBuf d_hmg(ctx);
    VK_TRY(d_hmg.ensure(N * 32));
    VK_TRY(mp_stage_h(ctx, N, zval, tt[0], reinterpret_cast<Fr*>(pin_hmg + N * 32), mid, d_g.as<fe<F>>(), d_h.as<fe<F>>(),
                      d_hmg.as<fe<F>>()));
    VK_CHECK_HIP(hipMemcpyAsync(pin_hmg, d_hmg.p, N * 32, hipMemcpyDeviceToHost, st));
    lap("t, h");
    uint64_t exy[8];
    uint8_t einf;
    VK_TRY(commit_dev(d_h.p, exy, &einf));  // (its completion follows the copy above in the stream)
    lap("E");
    transcript_append_point(tr, exy, einf, "E");
    std::vector<std::vector<Fr>> hmg(1, std::vector<Fr>(N));
    memcpy(hmg[0].data(), pin_hmg, N * 32);
    const std::vector<Acc> mc(1, C::add(acc_of(exy, einf), C::neg(acc_of(dxy, dinf))));
    memcpy(d_xy, dxy, 64);
    *d_inf = dinf;
    const int s = mp_inner_proofs(ctx, scheme, t, N, hmg, mc, tt, &tr, ipa_proof, kzg_xy, kzg_inf, kzg_y);
    if (scheme == 0) lap("inner IPA proof");
    return s;
}

// ---- the sparse field phase (scheme_internal.hpp MpSparse; the verkle tree proofs): the same sums
// S[row][k] = sum r^i f_i[k] as k_mp_chunk's, with f_i[k] looked up instead of streamed -- a verkle
// opening's row has a handful of non-zeros of 256, most of them items already in the tree's device
// mirror, and many queries open the same row at different points; so no Q x N matrix is built,
// uploaded or read. Each distinct row has a descriptor of 2 N / 32 words: its non-zero columns as a
// bitmap, and per bitmap word the index of that word's first non-zero in the source list. A query
// names its row; lane k of a block tests bit k, ranks it with a popcount and loads the value from
// the mirror's items or the literals. The plan (queries sorted by point, chunks of one point's
// queries, the reduce pass over a point's chunks) is k_mp_chunk's own MpPlan, and so is the
// arithmetic: mp_block over blocks of MP_SP_LZ queries, an absent element entering as zero. A block
// in which no lane of the wave has an element is skipped (extension rows live in columns 0..3: three
// of the four waves of a 256-column block).
constexpr uint32_t MP_SP_LZ = 4;
__global__ void __launch_bounds__(256) k_mp_sparse_chunk(const uint32_t* __restrict__ desc, const uint32_t* __restrict__ q_row,
                                                        const uint32_t* __restrict__ srcs,
                                                        const uint64_t* __restrict__ item,
                                                        const uint64_t* __restrict__ aux,
                                                        const uint32_t* __restrict__ rp, const uint32_t* __restrict__ order,
                                                        const uint32_t* __restrict__ be, uint32_t N, uint32_t kblk,
                                                        Fr* __restrict__ partial) {
    const uint32_t c = blockIdx.x / kblk;
    const uint32_t k = (blockIdx.x % kblk) * blockDim.x + threadIdx.x;
    if (k >= N) return;
    const uint32_t W = N >> 5, kw = k >> 5, below = (1u << (k & 31)) - 1u;
    const uint32_t u0 = be[2 * c], cnt = be[2 * c + 1] - u0;
    f29<P29> total = zero29<P29>();
    for (uint32_t h = 0; h < cnt; h += MP_SP_LZ) {
        const uint32_t nq = min(cnt - h, MP_SP_LZ);
        uint4 v[MP_SP_LZ][2];
        uint32_t qi[MP_SP_LZ];
        int have = 0;
#pragma unroll
        for (uint32_t j = 0; j < MP_SP_LZ; j++) {
            qi[j] = j < nq ? order[u0 + h + j] : 0u;
            v[j][0] = v[j][1] = make_uint4(0, 0, 0, 0);
            if (j < nq) {
                const uint32_t* d = desc + (size_t)q_row[qi[j]] * (2 * W);
                const uint32_t word = d[kw];
                if ((word >> (k & 31)) & 1u) {
                    const uint32_t s = srcs[d[W + kw] + __popc(word & below)];
                    const uint4* src = reinterpret_cast<const uint4*>(
                        (s & MP_SRC_AUX) ? aux + 4 * (size_t)(s & ~MP_SRC_AUX) : item + 4 * (size_t)s);
                    v[j][0] = src[0];
                    v[j][1] = src[1];
                    have = 1;
                }
            }
        }
        if (!__any(have)) continue;  // (the same for every lane of the wave)
        const f29<P29> r = mp_block<MP_SP_LZ>(v, qi, nq, rp);
        total = csub29<P29>(carry29<P29>(add29_raw<P29>(total, r)));
    }
    total = csub29<P29>(carry29<P29>(total));
    pack29<P29>(total, partial[(size_t)c * N + k].v);
}

// the rows' descriptors, checked (every index a kernel will follow is validated here) and uploaded
// with the source list, the queries' rows and the literal values
struct MpSparseUp {
    uvec<uint32_t> desc;
    DevBuf d_desc, d_qrow, d_srcs, d_aux;
    explicit MpSparseUp(vc_ctx* ctx) : d_desc(ctx), d_qrow(ctx), d_srcs(ctx), d_aux(ctx) {}
};
static int mp_sparse_upload(vc_ctx* ctx, size_t N, size_t Q, const MpSparse& sp, MpSparseUp* up) {
    const size_t W = N / 32, R = sp.n_rows;
    if (N % 32 || R >= MP_SRC_AUX || Q >= MP_SRC_AUX) return VC_E_RANGE;
    const size_t nnz = R ? sp.row_ptr[R] : 0;
    up->desc.assign(R * 2 * W, 0);
    for (size_t d = 0; d < R; d++) {
        uint32_t* bm = &up->desc[d * 2 * W];
        const uint32_t a = sp.row_ptr[d], b = sp.row_ptr[d + 1];
        if (a > b || b > nnz) return VC_E_INVALID;
        for (uint32_t e = a; e < b; e++) {
            const uint32_t col = sp.col[e], s = sp.src[e];
            if (col >= N || (e > a && col <= sp.col[e - 1])) return VC_E_INVALID;  // ascending: the rank is the index
            if ((s & MP_SRC_AUX) ? (s & ~MP_SRC_AUX) >= sp.n_aux : s >= sp.n_item) return VC_E_INVALID;
            bm[col >> 5] |= 1u << (col & 31);
        }
        uint32_t run = a;
        for (size_t w = 0; w < W; w++) {
            bm[W + w] = run;
            run += (uint32_t)__builtin_popcount(bm[w]);
        }
    }
    for (size_t q = 0; q < Q; q++)
        if (sp.q_row[q] >= R) return VC_E_INVALID;
    hipStream_t st = ctx->stream;
    VK_TRY(up->d_desc.ensure(std::max<size_t>(up->desc.size(), 1) * 4));
    VK_TRY(up->d_qrow.ensure(Q * 4));
    VK_TRY(up->d_srcs.ensure(std::max<size_t>(nnz, 1) * 4));
    VK_TRY(up->d_aux.ensure(std::max<size_t>(sp.n_aux, 1) * 32));
    if (!up->desc.empty())
        VK_CHECK_HIP(hipMemcpyAsync(up->d_desc.p, up->desc.data(), up->desc.size() * 4, hipMemcpyHostToDevice, st));
    VK_CHECK_HIP(hipMemcpyAsync(up->d_qrow.p, sp.q_row, Q * 4, hipMemcpyHostToDevice, st));
    if (nnz) VK_CHECK_HIP(hipMemcpyAsync(up->d_srcs.p, sp.src, nnz * 4, hipMemcpyHostToDevice, st));
    if (sp.n_aux) VK_CHECK_HIP(hipMemcpyAsync(up->d_aux.p, sp.aux, sp.n_aux * 32, hipMemcpyHostToDevice, st));
    return VC_OK;
}

int mp_prove_sparse(vc_ctx* ctx, int scheme, int table, size_t N, size_t Q, const uint64_t* com_xy,
                    const uint8_t* com_inf, const uint64_t* z, const uint64_t* y, const MpSparse& sp, uint64_t* d_xy,
                    uint8_t* d_inf, vc_ipa_proof* ipa_proof, uint64_t* kzg_xy, uint8_t* kzg_inf, uint64_t* kzg_y) {
    if (!ctx || !com_xy || !com_inf || !z || !y || !d_xy || !d_inf || ctx->curve != VC_CURVE_BN254 || !is_pow2(N) ||
        Q == 0 || !sp.q_row || (sp.n_rows && (!sp.row_ptr || !sp.col || !sp.src)) || (sp.n_aux && !sp.aux) ||
        (sp.n_item && !sp.d_item))
        return VC_E_INVALID;
    if (!mp_outputs_ok(scheme, 1, ipa_proof, kzg_xy, kzg_inf, kzg_y)) return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    std::vector<uint32_t> zval;
    VK_TRY(mp_points(N, Q, z, &zval));
    const size_t Z = zval.size();
    hipStream_t st = ctx->stream;
    MpPlan pl(ctx);
    MpSparseUp up(ctx);
    DevBuf d_S(ctx);
    vc_transcript* tr = nullptr;
    Fr r;
    VK_TRY(mp_begin_overlapped(ctx, N, Q, com_xy, com_inf, z, y, &tr, &r, [&]() -> int {
        VK_TRY(d_S.ensure(Z * N * 32));
        VK_TRY(mp_sparse_upload(ctx, N, Q, sp, &up));
        return mp_plan(ctx, N, Q, z, 0, zval, &pl);
    }));
    auto run = [&]() -> int {
        const uint32_t kblk = (uint32_t)((N + 255) / 256);
        VK_LAUNCH(ctx, "mp_rpow", k_mp_rpow, (Q + 255) / 256, 256, 0, r, (size_t)0, Q, pl.d_rp.as<uint32_t>());
        VK_LAUNCH(ctx, "mp_sparse_chunk", k_mp_sparse_chunk, (size_t)pl.nch * kblk, 256, 0, up.d_desc.as<uint32_t>(),
                  up.d_qrow.as<uint32_t>(), up.d_srcs.as<uint32_t>(), sp.d_item, up.d_aux.as<uint64_t>(),
                  pl.d_rp.as<uint32_t>(), pl.d_order.as<uint32_t>(), pl.d_be.as<uint32_t>(), (uint32_t)N, kblk,
                  pl.d_part.as<Fr>());
        VK_LAUNCH(ctx, "mp_chunk_reduce", k_mp_chunk_reduce, Z * kblk, 256, 0, pl.d_part.as<Fr>(), pl.d_zc.as<uint32_t>(),
                  N, kblk, d_S.as<Fr>());
        return mp_finish(ctx, scheme, t, N, zval, d_S.p, 1, tr, d_xy, d_inf, ipa_proof, kzg_xy, kzg_inf, kzg_y);
    };
    const int s = run();
    if (s != VC_OK) (void)hipStreamSynchronize(st);
    vc_transcript_free(tr);
    return s;
}

// E - D and t of verify_multiproof (:178-215); tr returned positioned after "E"
static int mp_claim(vc_ctx* ctx, size_t N, size_t Q, const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z,
                    const uint64_t* y, const uint64_t* d_xy, uint8_t d_inf, Acc* claim, Fr* t_out,
                    vc_transcript** tr_out) {
    if (!is_pow2(N) || N > (size_t(1) << 28)) return VC_E_INVALID;  // tables below are sized by N
    for (size_t i = 0; i < Q; i++)
        if (z[i] >= N) return VC_E_DOMAIN;
    const double c0 = host_timing() ? clock_us() : 0.0;
    vc_transcript* tr = nullptr;
    Fr r;
    // the e-coefficient MSM's points (the Q commitments) are uploaded and checked on the GPU while
    // the host transcript runs (mp_begin_overlapped) once the transcript is long enough to pay for
    // the helper thread (Q = 32768: verify 2.37-2.52 -> 2.28 ms; neutral at 4096)
    const bool filled = Q >= 8192;
    if (Q == 0) {  // no queries: the transcript of the labels alone (mp_begin wants Q > 0)
        tr = vc_transcript_new("multiproof");
        r = transcript_digest(tr, "r");
    } else if (filled) {
        VK_TRY(mp_begin_overlapped(ctx, N, Q, com_xy, com_inf, z, y, &tr, &r,
                                   [&] { return bases_fill(ctx, &ctx->scratch, com_xy, com_inf, Q); }));
    } else {
        VK_TRY(mp_begin(N, Q, com_xy, com_inf, z, y, &tr, &r));
    }
    vc_transcript_append_point(tr, d_xy, d_inf, "D");
    Fr tt = transcript_digest(tr, "t");
    std::vector<Fr> invs = invert_domain_at(tt, N);
    std::vector<Fr> coef(Q);
    // coef_i = r^i / (t - z_i): contiguous slices on the host pool, each starting from r^lo
    // (2 Q multiplies: ~2.5 ms serial at Q = 2^15)
    auto fill = [&](size_t lo, size_t hi) {
        Fr rp = fe_pow_u64<F>(r, lo);
        for (size_t i = lo; i < hi; i++) {
            coef[i] = fe_mul<F>(rp, invs[z[i]]);
            rp = fe_mul<F>(rp, r);
        }
    };
    if (Q < 4096 || host_pool().size() == 1) {
        fill(0, Q);
    } else {
        const unsigned T = host_pool().size();
        host_pool().run([&](unsigned k) { fill(Q * k / T, Q * (k + 1) / T); });
    }
    const double c1 = host_timing() ? clock_us() : 0.0;
    Acc e;
    int st = msm_points(ctx, com_xy, com_inf, coef, &e, filled);
    if (st != VC_OK) {
        vc_transcript_free(tr);
        return st;
    }
    if (host_timing())
        fprintf(stderr, "mp_claim Q=%zu transcript+coef_us=%.1f e_msm_us=%.1f\n", Q, c1 - c0, clock_us() - c1);
    uint64_t exy[8];
    uint8_t einf;
    aff_of(e, exy, &einf);
    vc_transcript_append_point(tr, exy, einf, "E");
    *claim = C::add(e, C::neg(acc_of(d_xy, d_inf)));
    *t_out = tt;
    *tr_out = tr;
    return VC_OK;
}

}  // namespace vk

using namespace vk;

extern "C" {

int vc_multiproof_prove(vc_ctx* ctx, int scheme, int table, size_t N, size_t Q, const uint64_t* data,
                        const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z, const uint64_t* y,
                        uint64_t* d_xy, uint8_t* d_inf, vc_ipa_proof* ipa_proof, uint64_t* kzg_xy, uint8_t* kzg_inf,
                        uint64_t* kzg_y) {
    if (!ctx || !data || !com_xy || !com_inf || !z || !y || !d_xy || !d_inf || ctx->curve != VC_CURVE_BN254)
        return VC_E_INVALID;
    if (!mp_outputs_ok(scheme, 1, ipa_proof, kzg_xy, kzg_inf, kzg_y)) return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    vc_transcript* tr = nullptr;
    Fr r;
    std::vector<uint32_t> zval;
    if (!is_pow2(N) || Q == 0) return VC_E_INVALID;
    VK_TRY(mp_points(N, Q, z, &zval));
    DevBuf d_data(ctx), d_S(ctx);
    MpPlan pl(ctx);
    // the 32 Q N bytes of evaluations cross PCIe and the shard is planned under the transcript
    VK_TRY(mp_begin_overlapped(ctx, N, Q, com_xy, com_inf, z, y, &tr, &r, [&]() -> int {
        VK_TRY(d_data.ensure(Q * N * 32));
        VK_TRY(d_S.ensure(zval.size() * N * 32));
        VK_CHECK_HIP(hipMemcpyAsync(d_data.p, data, Q * N * 32, hipMemcpyHostToDevice, ctx->stream));
        return mp_plan(ctx, N, Q, z, 0, zval, &pl);
    }));
    int st = mp_run(ctx, N, d_data.p, r, pl, d_S.p);
    if (st == VC_OK)
        st = mp_finish(ctx, scheme, t, N, zval, d_S.p, 1, tr, d_xy, d_inf, ipa_proof, kzg_xy, kzg_inf, kzg_y);
    vc_transcript_free(tr);
    return st;
}

// P independent multiproofs of Q queries each (same N, one CRS / SRS) on one GPU, proof-parallel:
// the host transcripts (records + serial SHA-256, the part that bounds one proof) run on worker
// threads while the GPU accumulates every proof whose challenge r is ready; each later stage then
// runs ONCE for all P proofs -- one batched D commit, one batched E commit and, for IPA, one
// batched inner proof (its 8 latency-bound rounds shared by the P proofs) -- instead of P times.
// Each proof is the one vc_multiproof_prove gives for its queries. Arrays are [P][Q] (com_xy [P][Q][8],
// y [P][Q][4]); d_data [P][Q][N] canonical on the device; outputs [P].
int vc_multiproof_prove_many(vc_ctx* ctx, int scheme, int table, size_t N, size_t Q, size_t P, const void* d_data,
                             const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z, const uint64_t* y,
                             uint64_t* d_xy, uint8_t* d_inf, vc_ipa_proof* ipa_proofs, uint64_t* kzg_xy,
                             uint8_t* kzg_inf, uint64_t* kzg_y) {
    if (!ctx || (P && (!d_data || !com_xy || !com_inf || !z || !y || !d_xy || !d_inf)) ||
        ctx->curve != VC_CURVE_BN254 || !mp_outputs_ok(scheme, P, ipa_proofs, kzg_xy, kzg_inf, kzg_y))
        return VC_E_INVALID;
    Guard guard(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    if (!is_pow2(N) || Q == 0) return VC_E_INVALID;
    if (P == 0) return VC_OK;
    struct Begun {
        vc_transcript* tr = nullptr;
        Fr r;
        std::vector<uint32_t> zval;
        int st = VC_E_INVALID;
        bool done = false;
    };
    std::vector<Begun> B(P);
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<size_t> next{0};
    std::atomic<bool> cancel{false};  // set once phase 2 fails: the workers start no further transcript
    // one proof per worker at a time, each filled serially (no nested host pool): T workers share
    // the host's CPUs instead of queueing on the pool's one-loop lock
    const unsigned T = (unsigned)std::min<size_t>(P, std::max(1u, std::min(8u, std::thread::hardware_concurrency() / 2)));
    std::vector<std::thread> workers;
    for (unsigned k = 0; k < T; k++)
        workers.emplace_back([&] {
            for (size_t p; !cancel.load(std::memory_order_relaxed) && (p = next.fetch_add(1)) < P;) {
                Begun b;
                try {  // nothing may leave a thread function
                    b.st = mp_begin(N, Q, com_xy + p * Q * 8, com_inf + p * Q, z + p * Q, y + p * Q * 4, &b.tr,
                                    &b.r, false);
                    if (b.st == VC_OK) b.st = mp_points(N, Q, z + p * Q, &b.zval);
                } catch (...) {
                    b.st = VC_E_OOM;
                }
                std::lock_guard<std::mutex> lk(mu);
                B[p] = std::move(b);
                B[p].done = true;
                cv.notify_all();
            }
        });
    auto free_all = [&] {  // (after the workers have been joined)
        for (auto& b : B)
            if (b.tr) vc_transcript_free(b.tr);
    };
    // phase 2: per-point sums of each proof as soon as its transcript is done (GPU, in order)
    std::vector<std::unique_ptr<DevBuf>> S(P);
    int st = VC_OK;
    for (size_t p = 0; p < P && st == VC_OK; p++) {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return B[p].done; });
        }
        if ((st = B[p].st) != VC_OK) break;
        S[p] = std::make_unique<DevBuf>(ctx);
        st = S[p]->ensure(B[p].zval.size() * N * 32);
        if (st == VC_OK)
            st = mp_accumulate(ctx, N, Q, static_cast<const uint8_t*>(d_data) + p * Q * N * 32, z + p * Q, B[p].r, 0, B[p].zval, S[p]->p);
    }
    if (st != VC_OK) cancel.store(true);
    for (auto& w : workers) w.join();
    workers.clear();
    if (st != VC_OK) {
        free_all();
        return st;
    }
    // phase 3: quotients and g of every proof, then D for all P in one batched commit
    hipStream_t hs = ctx->stream;
    MpDomain dom;
    st = domain_tables<F>(ctx, bn254_group_gen(N), N, &dom.pw, &dom.pwi, &dom.inv1);
    std::vector<std::unique_ptr<MpMid>> mid(P);
    DevBuf d_g(ctx), d_h(ctx);
    if (st == VC_OK) st = d_g.ensure(P * N * 32);
    if (st == VC_OK) st = d_h.ensure(P * N * 32);
    for (size_t p = 0; p < P && st == VC_OK; p++) {
        mid[p] = std::make_unique<MpMid>(ctx);
        if ((st = mid[p]->ensure(B[p].zval.size(), N)) != VC_OK) break;
        st = mp_stage_g(ctx, N, B[p].zval, S[p]->p, 1, dom, *mid[p], d_g.as<fe<F>>() + p * N, d_h.as<fe<F>>() + p * N);
    }
    std::vector<Fr> g(P * N), h(P * N);
    std::vector<uint64_t> dxy(P * 8), exy(P * 8);
    std::vector<uint8_t> dinf(P), einf(P);
    std::vector<Fr> tt(P);
    if (st == VC_OK && hipMemcpyAsync(g.data(), d_g.p, P * N * 32, hipMemcpyDeviceToHost, hs) != hipSuccess) st = VC_E_HIP;
    if (st == VC_OK && hipStreamSynchronize(hs) != hipSuccess) st = VC_E_HIP;
    if (st == VC_OK) st = commit_batch(ctx, t, N, g.data(), P, dxy.data(), dinf.data());
    // t of every proof, then h and E for all P
    for (size_t p = 0; p < P && st == VC_OK; p++) {
        transcript_append_point(B[p].tr, &dxy[p * 8], dinf[p], "D");
        tt[p] = transcript_digest(B[p].tr, "t");
        std::vector<Fr> invz(B[p].zval.size());
        st = mp_stage_h(ctx, N, B[p].zval, tt[p], invz.data(), *mid[p], d_g.as<fe<F>>() + p * N, d_h.as<fe<F>>() + p * N,
                        nullptr);
        if (hipStreamSynchronize(hs) != hipSuccess && st == VC_OK) st = VC_E_HIP;  // invz dies here
    }
    if (st == VC_OK && hipMemcpyAsync(h.data(), d_h.p, P * N * 32, hipMemcpyDeviceToHost, hs) != hipSuccess) st = VC_E_HIP;
    if (st == VC_OK && hipStreamSynchronize(hs) != hipSuccess) st = VC_E_HIP;
    if (st == VC_OK) st = commit_batch(ctx, t, N, h.data(), P, exy.data(), einf.data());
    std::vector<std::vector<Fr>> hmg(P, std::vector<Fr>(N));
    std::vector<Acc> mc(P);
    std::vector<vc_transcript*> trs(P);
    for (size_t p = 0; p < P && st == VC_OK; p++) {
        transcript_append_point(B[p].tr, &exy[p * 8], einf[p], "E");
        for (size_t k = 0; k < N; k++) hmg[p][k] = fe_sub<F>(h[p * N + k], g[p * N + k]);
        mc[p] = C::add(acc_of(&exy[p * 8], einf[p]), C::neg(acc_of(&dxy[p * 8], dinf[p])));
        memcpy(d_xy + p * 8, &dxy[p * 8], 64);
        d_inf[p] = dinf[p];
        trs[p] = B[p].tr;
    }
    // the inner proofs: one batched IPA (each proof with its own transcript), or P KZG openings
    if (st == VC_OK)
        st = mp_inner_proofs(ctx, scheme, t, N, hmg, mc, tt, trs.data(), ipa_proofs, kzg_xy, kzg_inf, kzg_y);
    free_all();
    return st;
}

int vc_multiproof_begin(size_t N, size_t Q, const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z,
                        const uint64_t* y, vc_transcript** tr_out, uint64_t* r_out, size_t* rows) {
    if (!com_xy || !com_inf || !z || !y || !tr_out || !r_out || !rows) return VC_E_INVALID;
    vc_transcript* tr = nullptr;
    Fr r;
    VK_TRY(mp_begin(N, Q, com_xy, com_inf, z, y, &tr, &r, false));  // (callers overlap several)
    canon_of(r, r_out);
    std::vector<uint32_t> zval;
    const int zst = mp_points(N, Q, z, &zval);  // z itself was validated by mp_begin
    if (zst != VC_OK) {
        vc_transcript_free(tr);
        return zst;
    }
    *rows = zval.size();
    *tr_out = tr;
    return VC_OK;
}

int vc_multiproof_rows(size_t N, size_t Q, const uint64_t* z, size_t* rows) {
    if (!z || !rows || !is_pow2(N) || Q == 0) return VC_E_INVALID;
    std::vector<uint32_t> zval;
    VK_TRY(mp_points(N, Q, z, &zval));
    *rows = zval.size();
    return VC_OK;
}

// begin + accumulate of one query shard [first, first + Qs) with the transcript overlapped (the
// single-proof paths: mp_prove, vc_multiproof_prove_sharded)
int vc_multiproof_begin_accumulate(vc_ctx* ctx, size_t N, size_t Q, const uint64_t* com_xy, const uint8_t* com_inf,
                                   const uint64_t* z, const uint64_t* y, size_t first, size_t Qs, const void* d_data,
                                   void* d_S, vc_transcript** tr_out, uint64_t* r_out) {
    if (tr_out) *tr_out = nullptr;  // no transcript on any error return (vc_scheme.h)
    if (!ctx || !com_xy || !com_inf || !z || !y || !d_S || !tr_out || !r_out || (Qs && !d_data) || first > Q ||
        Qs > Q - first || ctx->curve != VC_CURVE_BN254 || !is_pow2(N) || Q == 0)
        return VC_E_INVALID;
    std::vector<uint32_t> zval;
    VK_TRY(mp_points(N, Q, z, &zval));
    Guard g(ctx);
    MpPlan pl(ctx);
    Fr r;
    VK_TRY(mp_begin_overlapped(ctx, N, Q, com_xy, com_inf, z, y, tr_out, &r,
                               [&] { return mp_plan(ctx, N, Qs, z + first, first, zval, &pl); }));
    canon_of(r, r_out);
    const int st2 = mp_run(ctx, N, d_data, r, pl, d_S);
    if (st2 != VC_OK) {
        vc_transcript_free(*tr_out);
        *tr_out = nullptr;
    }
    return st2;
}

int vc_multiproof_accumulate(vc_ctx* ctx, size_t N, size_t Q, const uint64_t* z, size_t first, size_t Qs,
                             const void* d_data, const uint64_t* r, void* d_S) {
    if (!ctx || !z || !r || !d_S || (Qs && !d_data) || first > Q || Qs > Q - first || ctx->curve != VC_CURVE_BN254)
        return VC_E_INVALID;
    if (!is_pow2(N) || Q == 0) return VC_E_INVALID;
    Guard g(ctx);
    std::vector<uint32_t> zval;
    VK_TRY(mp_points(N, Q, z, &zval));
    return mp_accumulate(ctx, N, Qs, d_data, z + first, fr_of(r), first, zval, d_S);
}

int vc_multiproof_finish(vc_ctx* ctx, int scheme, int table, size_t N, size_t Q, const uint64_t* z,
                         const void* d_S_parts, int G, vc_transcript* tr, uint64_t* d_xy, uint8_t* d_inf,
                         vc_ipa_proof* ipa_proof, uint64_t* kzg_xy, uint8_t* kzg_inf, uint64_t* kzg_y) {
    if (!ctx || !z || !d_S_parts || G < 1 || !tr || !d_xy || !d_inf || ctx->curve != VC_CURVE_BN254)
        return VC_E_INVALID;
    if (!mp_outputs_ok(scheme, 1, ipa_proof, kzg_xy, kzg_inf, kzg_y)) return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    std::vector<uint32_t> zval;
    VK_TRY(mp_points(N, Q, z, &zval));
    return mp_finish(ctx, scheme, t, N, zval, d_S_parts, G, tr, d_xy, d_inf, ipa_proof, kzg_xy, kzg_inf,
                     kzg_y);
}

int vc_multiproof_verify_ipa(vc_ctx* ctx, int table, size_t N, size_t Q, const uint64_t* com_xy, const uint8_t* com_inf,
                             const uint64_t* z, const uint64_t* y, const uint64_t* d_xy, uint8_t d_inf,
                             const vc_ipa_proof* proof, int* result) {
    if (!ctx || !com_xy || !com_inf || !z || !y || !d_xy || !proof_ok(proof) || !result || ctx->curve != VC_CURVE_BN254)
        return VC_E_INVALID;
    Guard g(ctx);
    Table* t = ctx->table(table);
    if (!t) return VC_E_TABLE;
    Acc claim;
    Fr tt;
    vc_transcript* tr = nullptr;
    VK_TRY(mp_claim(ctx, N, Q, com_xy, com_inf, z, y, d_xy, d_inf, &claim, &tt, &tr));
    int st = ipa_verify_impl(ctx, t, N, claim, tt, proof, tr, result);
    vc_transcript_free(tr);
    return st;
}

int vc_multiproof_kzg_claim(vc_ctx* ctx, size_t N, size_t Q, const uint64_t* com_xy, const uint8_t* com_inf,
                            const uint64_t* z, const uint64_t* y, const uint64_t* d_xy, uint8_t d_inf, uint64_t* c_xy,
                            uint8_t* c_inf, uint64_t* t_out) {
    if (!ctx || !com_xy || !com_inf || !z || !y || !d_xy || !c_xy || !c_inf || !t_out || ctx->curve != VC_CURVE_BN254)
        return VC_E_INVALID;
    Guard g(ctx);
    Acc claim;
    Fr tt;
    vc_transcript* tr = nullptr;
    VK_TRY(mp_claim(ctx, N, Q, com_xy, com_inf, z, y, d_xy, d_inf, &claim, &tt, &tr));
    vc_transcript_free(tr);
    aff_of(claim, c_xy, c_inf);
    canon_of(tt, t_out);
    return VC_OK;
}

int vc_multiproof_verify_kzg(vc_ctx* ctx, const vc_kzg_vk* vk, size_t N, size_t Q, const uint64_t* com_xy,
                             const uint8_t* com_inf, const uint64_t* z, const uint64_t* y, const uint64_t* d_xy,
                             uint8_t d_inf, const uint64_t* kzg_proof_xy, uint8_t kzg_proof_inf,
                             const uint64_t* kzg_y, int* result) {
    if (!vk || !result || !kzg_y || (!kzg_proof_xy && !kzg_proof_inf)) return VC_E_INVALID;
    if (kzg_vk_curve(vk) != VC_CURVE_BN254) return VC_E_INVALID;  // the protocol layer is BN254
    uint64_t c_xy[8], t[4];
    uint8_t c_inf = 0;
    VK_TRY(vc_multiproof_kzg_claim(ctx, N, Q, com_xy, com_inf, z, y, d_xy, d_inf, c_xy, &c_inf, t));
    // KZG::verify_point takes no transcript (kzg/mod.rs:165-189): the claim and the proof decide
    return vc_kzg_verify(vk, c_xy, c_inf, t, kzg_proof_xy, kzg_proof_inf, kzg_y, result);
}

}  // extern "C"

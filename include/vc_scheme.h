/* vc_scheme.h -- scheme-level C ABI of libvkzg.so: the reference's VectorCommitment
 * operations (/root/reference/vector-commit/src/lib.rs:70-174) for BN254 G1, with every
 * MSM / quotient / fold on the GPU and the serial Fiat-Shamir work on the host.  KZG openings
 * are verified with the BN254 pairing: one at a time on the host (vc_kzg_verify), or a batch on
 * the GPU with one verdict per proof (vc_kzg_verify_many); IPA openings likewise, one at a time
 * (vc_ipa_verify) or a batch with one verdict each (vc_ipa_verify_many).
 *
 * Field elements (Fr) are 4 canonical little-endian u64 limbs; points are canonical affine
 * x[4], y[4] + a u8 identity flag (as in vc_msm.h).  All calls are synchronous and return
 * VC_OK or a VC_E_* status (vc_msm.h).  The reference leaves its batch methods `todo!()`
 * (prove_batch / verify_batch, ipa/mod.rs:156-189, kzg/mod.rs:156-197); here vc_ipa_prove takes a
 * batch, and vc_ipa_verify_many / vc_kzg_verify_many verify n independent openings with one verdict
 * each (what verify_batch would return per entry); vc_kzg_verify_batch and vc_ipa_verify_batch are
 * the aggregated single-verdict checks.
 *
 * Scope: the protocol layer is instantiated for BN254 (the only curve the reference runs,
 * vector-commit/Cargo.toml:15).  The MSM / commit engines (vc_msm.h) also serve BLS12-381 G1
 * and Bandersnatch, and the KZG verifiers also take a BLS12-381 key (the section "KZG
 * verification on BLS12-381" at the end states its layouts and rules).
 */
#ifndef VC_SCHEME_H
#define VC_SCHEME_H

#include <stddef.h>
#include <stdint.h>

#include "vc_msm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- Fiat-Shamir (a12)
 * TranscriptHasher (transcript.rs:28-62): append(label || compressed(value)); digest(label) =
 * hash_to_field(state || label) with DefaultFieldHasher<Sha256> and DST = the label given at
 * creation; then state = ser(out) || label. */
typedef struct vc_transcript vc_transcript;
vc_transcript* vc_transcript_new(const char* label);
/* which SHA-256 rounds the host transcript runs on this machine: 1 = x86 SHA extensions (SHA-NI),
 * 0 = the portable rounds (same digests; a machine-dependent speed, reported by bench.py) */
int vc_host_sha256_path(void);
vc_transcript* vc_transcript_clone(const vc_transcript* t);
void vc_transcript_free(vc_transcript* t);
void vc_transcript_reserve(vc_transcript* t, size_t bytes); /* capacity hint for long transcripts */
int vc_transcript_append_bytes(vc_transcript* t, const uint8_t* bytes, size_t n, const char* label);
int vc_transcript_append_point(vc_transcript* t, const uint64_t* xy, uint8_t inf, const char* label);
int vc_transcript_append_fr(vc_transcript* t, const uint64_t* fr, const char* label);
int vc_transcript_append_u64(vc_transcript* t, uint64_t v, const char* label);
int vc_transcript_digest(vc_transcript* t, const char* label, uint64_t* out_fr);
/* raw hash_to_field(msg) mod r with the given DST */
int vc_hash_to_field(const uint8_t* msg, size_t n, const uint8_t* dst, size_t dst_len, uint64_t* out_fr);

/* ---------------------------------------------------------------- serialisation (a13)
 * arkworks 0.4 compressed SW encoding (32 B) and VCCommitment::to_data_item (lib.rs:56-67). */
int vc_point_compress(const uint64_t* xy, uint8_t inf, uint8_t* out32);
/* batched on the device: n points -> n Fr (canonical) */
int vc_to_data_item_batch(vc_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t n, uint64_t* out_fr);

/* ---------------------------------------------------------------- CRS (a15)
 * IPAPointGenerator::gen (ipa_point_generator.rs:51-67): first `num` accepted points of
 * sha256(seed || le64(i)) -> Affine::from_random_bytes.  VC_E_RANGE if num > max
 * (PointGeneratorError::OutOfBounds, Appendix B.1). */
int vc_ipa_crs(const uint8_t* seed, size_t seed_len, size_t max, size_t num, uint64_t* out_xy);
/* KZG::setup (kzg/mod.rs:115-124): Lagrange SRS L_j = l_j(s) * G over the domain of size
 * n = next_pow2(max_items), computed on the device; out n points (table uploaded into ctx). */
int vc_kzg_setup(vc_ctx* ctx, size_t max_items, const uint64_t* secret_fr, int* table_id, size_t* size);

/* ---------------------------------------------------------------- IPA (ipa/mod.rs)
 * `table` holds the N + 1 CRS points g[0..N], q (IPAUniversalParams::new_from_vec).
 * Proof layout: L[k], R[k] points (k = log2 N rounds), tip, y. */
typedef struct {
    size_t rounds;
    uint64_t* l_xy; uint8_t* l_inf;   /* rounds x 8 u64, rounds */
    uint64_t* r_xy; uint8_t* r_inf;
    uint64_t tip[4];
    uint64_t y[4];
} vc_ipa_proof;

int vc_ipa_commit(vc_ctx* ctx, int table, size_t N, const uint64_t* data, size_t batch,
                  uint64_t* out_xy, uint8_t* out_inf);
/* prove_point (:137-154 -> low_level_ipa :268-319). transcript may be NULL (fresh "ipa").
 * Proves `batch` independent openings at once (same N, one CRS): data batch x N, points batch,
 * commitments batch; transcripts NULL or an array of batch handles (consumed state). */
int vc_ipa_prove(vc_ctx* ctx, int table, size_t N, const uint64_t* data, const uint64_t* com_xy,
                 const uint8_t* com_inf, const uint64_t* points, size_t batch,
                 vc_transcript** transcripts, vc_ipa_proof* proofs);
/* n openings in one call, the whole proof made on the device (the reference's prove_batch,
 * ipa/mod.rs:156-163, is todo!(); its BatchProof is Vec<Proof>). Opening i is prove_point of row
 * row[i] of `data` (rows x N canonical values; row == NULL: row i, and then rows == n) at
 * points[i] (n x 4) over a fresh "ipa" transcript; callers with prior transcript state keep using
 * vc_ipa_prove. The row's commitment is com_xy + 8 row[i], com_inf[row[i]] (per row, as
 * vc_ipa_commit gives them; not checked against the data, as in vc_ipa_prove). Outputs are the flat
 * layouts vc_ipa_verify_many / vc_ipa_verify_batch read, K = log2 N: l_xy / r_xy n x K x 8,
 * l_inf / r_inf n x K, tip and y n x 4 -- a batch goes from prover to verifier without repacking.
 * Opening i equals, bit for bit, what vc_ipa_prove(ctx, table, N, data + row[i] N 4, .., points +
 * 4 i, 1, NULL, ..) writes.
 * Every status other than VC_OK is decided on the host before any GPU work, the outputs untouched.
 * VC_E_INVALID: N not a power of two or outside [2, 256] (vc_ipa_verify_batch's bound: a wave's
 * share of a row is four entries per lane), a context that is not BN254, a null array with n > 0,
 * row == NULL with rows != n, a row[i] >= rows, a point >= r, a table of fewer than N + 1 points.
 * VC_E_TABLE: an unknown table. VC_E_DOMAIN for the whole call when a point is a domain element
 * w^i that is not below N as an integer (as vc_ipa_prove treats a batch). n = 0 is VC_OK.
 * The rows are uploaded once; per chunk of at most 8192 openings the weights, the transcripts, the
 * folds and the rounds' scalar rows are made by kernels and committed by the fixed-base engine
 * with nothing of the proof crossing to the host between the rounds (the commit's own
 * normalisation aside): the device workspace does not grow with n. Throughput-
 * shaped: a batch of one pays the whole pipeline's launches and is slower than vc_ipa_prove. */
int vc_ipa_prove_many(vc_ctx* ctx, int table, size_t N, size_t rows, const uint64_t* data,
                      const uint32_t* row, const uint64_t* com_xy, const uint8_t* com_inf,
                      const uint64_t* points, size_t n,
                      uint64_t* l_xy, uint8_t* l_inf, uint64_t* r_xy, uint8_t* r_inf,
                      uint64_t* tip, uint64_t* y);
/* the same with the rows already in device memory (rows x N x 4 u64, canonical; not written) */
int vc_ipa_prove_many_device(vc_ctx* ctx, int table, size_t N, size_t rows, const void* d_data,
                             const uint32_t* row, const uint64_t* com_xy, const uint8_t* com_inf,
                             const uint64_t* points, size_t n,
                             uint64_t* l_xy, uint8_t* l_inf, uint64_t* r_xy, uint8_t* r_inf,
                             uint64_t* tip, uint64_t* y);
/* verify_point (:165-181 -> low_level_verify_ipa :321-360); result 1 = valid, 0 = invalid */
int vc_ipa_verify(vc_ctx* ctx, int table, size_t N, const uint64_t* com_xy, uint8_t com_inf,
                  const uint64_t* point, const vc_ipa_proof* proof, vc_transcript* transcript,
                  int* result);
/* n independent openings (same N, one CRS), one verdict each: results[i] = 1 / 0 as
 * low_level_verify_ipa (ipa/mod.rs:321-360) of entry i. Flat layouts, K = log2 N rounds:
 * com_xy n x 8, com_inf n, points n x 4, l_xy / r_xy n x K x 8, l_inf / r_inf n x K,
 * tip n x 4, y n x 4 (u64, canonical). transcripts: NULL, or n handles, each NULL (fresh
 * "ipa") or a prior state, advanced as vc_ipa_verify advances it.
 * For every entry vc_ipa_verify answers with VC_OK, results[i] is its result. Malformed proof
 * contents give the verdict 0 and VC_OK, as in vc_kzg_verify_many and unlike vc_ipa_verify (which
 * returns VC_E_NOT_ON_CURVE for an off-curve L_k): a coordinate of C, L_k or R_k >= p, such a point
 * off the curve, tip, y or point >= r; no entry changes another's verdict, and the identity flag
 * is a valid input for C, L_k and R_k. A point that is a domain element w^i not below N as an
 * integer is the verifier's own input, not proof content: VC_E_DOMAIN for the whole call before
 * any GPU work, nothing written to results (as vc_ipa_prove treats a batch). VC_E_INVALID: N not a
 * power of two or < 2, a table of fewer than N + 1 points, a context that is not BN254, null
 * arrays with n > 0. n = 0 is VC_OK.
 * The transcripts run on the host pool, everything else on the device (scalar rows, the fixed-base
 * commit of the rows, the per-proof sum over C, L_k, R_k and the verdict), in chunks of at most
 * 16384 proofs: the device workspace does not grow with n. Throughput-shaped: a batch of one pays
 * the whole pipeline's launches and is slower than vc_ipa_verify. */
int vc_ipa_verify_many(vc_ctx* ctx, int table, size_t N, size_t n,
                       const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* points,
                       const uint64_t* l_xy, const uint8_t* l_inf, const uint64_t* r_xy, const uint8_t* r_inf,
                       const uint64_t* tip, const uint64_t* y, vc_transcript** transcripts, uint8_t* results);
/* One combined check for n openings ("are all of these valid?"; the reference names it
 * verify_batch, ipa/mod.rs:183-189, and leaves it todo!()). Let E_j be the left side of the identity
 * low_level_verify_ipa checks for entry j (the identity exactly when the entry is valid), sigma_j = 1
 * for a point below N and z_j^N - 1 otherwise (non-zero: domain elements not below N are refused).
 * With one challenge rho:
 *   S = sum_j rho^j sigma_j E_j,   accept  <=>  S is the identity.
 * A batch of valid entries is accepted for every rho; a batch with an invalid entry is accepted for
 * at most n - 1 of the r values of rho. rho = vc_hash_to_field(seed, 32, dst = "vkzg-ipa-batch"): the
 * verifier draws the seed itself once it holds the inputs; a given seed makes the call
 * deterministic. Layouts and status rules are vc_ipa_verify_many's, with one more bound: N <= 256
 * (the fold keeps a lane's columns of the fixed row in registers), VC_E_INVALID above it. */
/* rho for a seed (host, no context) */
int vc_ipa_batch_challenge(const uint8_t seed[32], uint64_t* rho_fr);
/* [w, x_0 .. x_{K-1}] of every entry's fresh "ipa" transcript, canonical: out n x (1 + K) x 4.
 * ctx == NULL: host pool; ctx != NULL: the device kernel (a lane per entry). No N <= 256 bound. */
int vc_ipa_challenges_many(vc_ctx* ctx, size_t N, size_t n, const uint64_t* com_xy, const uint8_t* com_inf,
                           const uint64_t* points, const uint64_t* y, const uint64_t* l_xy, const uint8_t* l_inf,
                           const uint64_t* r_xy, const uint8_t* r_inf, uint64_t* out);
/* the fold alone: S as a canonical affine point. *malformed = 1 (S unspecified) when any entry is
 * malformed in vc_ipa_verify_many's sense. ctx != NULL: device path over the table's CRS (crs_xy
 * ignored). ctx == NULL: host path (host pool) over crs_xy, the N + 1 points g_0 .. g_{N-1}, q as
 * canonical affine x[4] y[4] -- the check of the fold against the oracle on a machine without a
 * GPU, not a product path. VC_E_INVALID also for rho_fr >= r. */
int vc_ipa_batch_fold(vc_ctx* ctx, int table, const uint64_t* crs_xy, size_t N, size_t n, const uint64_t* com_xy,
                      const uint8_t* com_inf, const uint64_t* points, const uint64_t* l_xy, const uint8_t* l_inf,
                      const uint64_t* r_xy, const uint8_t* r_inf, const uint64_t* tip, const uint64_t* y,
                      vc_transcript** transcripts, const uint64_t* rho_fr, uint64_t* s_xy, uint8_t* s_inf,
                      int* malformed);
/* *result = 1 when the combined check accepts, else 0. seed32 == NULL: 32 bytes of OS entropy
 * (getrandom). results: NULL, or n bytes: all 1 when the check accepts; when it rejects (a malformed
 * entry included) vc_ipa_verify_many's verdicts, so a rejecting call costs the fold plus that call.
 * transcripts: NULL (every transcript a fresh "ipa" one, hashed on the device), or n handles as
 * vc_ipa_verify_many takes them (then all transcripts run on the host pool and the handles advance as
 * there, once). VC_E_DOMAIN before any GPU work with nothing written; a malformed proof entry gives
 * *result = 0 with VC_OK; n = 0: VC_OK, *result = 1. Chunks of at most 65536 proofs: the device
 * workspace does not grow with n. */
int vc_ipa_verify_batch(vc_ctx* ctx, int table, size_t N, size_t n, const uint64_t* com_xy, const uint8_t* com_inf,
                        const uint64_t* points, const uint64_t* l_xy, const uint8_t* l_inf, const uint64_t* r_xy,
                        const uint8_t* r_inf, const uint64_t* tip, const uint64_t* y, vc_transcript** transcripts,
                        const uint8_t* seed32, int* result, uint8_t* results);
/* prove_commitment (:199-234): proof of knowledge of the first n = data.max() + 1 values
 * behind a commitment (L, R per round, tip; y is set to 0). n must be a power of two: the
 * reference's assert in vec_add_and_distribute (utils.rs:37) panics on any odd split above 1
 * -> VC_E_INVALID here. Fresh "ipa" transcript, `batch` proofs of the same n at once. */
int vc_ipa_prove_commitment(vc_ctx* ctx, int table, size_t n, const uint64_t* data, const uint64_t* com_xy,
                            const uint8_t* com_inf, size_t batch, vc_ipa_proof* proofs);
/* verify_commitment_proof (:237-265) over g[0..2^rounds]; result 1 = valid, 0 = invalid */
int vc_ipa_verify_commitment_proof(vc_ctx* ctx, int table, const uint64_t* com_xy, uint8_t com_inf,
                                   const vc_ipa_proof* proof, int* result);

/* ---------------------------------------------------------------- KZG (kzg/mod.rs)
 * prove_point (:136-154): y = evaluate(point), q = divide_by_vanishing(index) when
 * point <= size, else divide_by_vanishing_outside_domain(point); proof = MSM(L, q).
 * evals may be shorter than the domain (`max`). The point's status is decided on the host
 * before any GPU work and a failing call leaves the outputs untouched: VC_E_INVALID for a
 * point >= r, VC_E_DOMAIN for point == size (the reference panics there, Appendix B.4) and
 * for a domain element that is not below size (z^size == 1, r - 1 = w^(size / 2) among them:
 * the reference divides by zero, precompute.rs:86), VC_OK otherwise. The same holds for
 * the device, part and commit+prove forms below, for vc_kzg_quotient and for
 * vc_group_kzg_prove (every member fails alike: no partial result). */
int vc_kzg_prove(vc_ctx* ctx, int table, size_t size, const uint64_t* evals, size_t max,
                 const uint64_t* point, uint64_t* proof_xy, uint8_t* proof_inf, uint64_t* y);
/* same with the evaluations already in device memory (canonical, 4 u64 each) */
int vc_kzg_prove_device(vc_ctx* ctx, int table, size_t size, const void* d_evals, size_t max,
                        const uint64_t* point, uint64_t* proof_xy, uint8_t* proof_inf, uint64_t* y);
/* n openings in one call: opening i is prove_point of row `row[i]` (row == NULL: row i, and then
 * rows == n) of `data` (rows x width canonical values, width <= N is the single call's `max`) at
 * points[i], and gives exactly what vc_kzg_prove(ctx, table, N, data + row[i] * width * 4, width,
 * points + 4 i, ..) gives. The rows are uploaded and converted once, the openings run in chunks of
 * at most 16,384: two field launches and one batched fixed-base commit per chunk. BN254 and
 * BLS12-381, 2 <= N <= 1024.
 * A status other than VC_OK is decided on the host before any GPU work and leaves the outputs
 * untouched: VC_E_INVALID (N not a power of two or outside [2, 1024], width > N, a null array with
 * n > 0, row == NULL with rows != n, a row[i] >= rows, a point >= r), VC_E_RANGE (the table has
 * fewer than N points), VC_E_DOMAIN for the whole call when a point equals N (Appendix B.4, as the
 * single call) or is a domain element (z^N == 1) that is not below N (the reference divides by
 * zero, precompute.rs:86). n == 0 is VC_OK.
 * proof_xy: n x 2 NL u64; proof_inf: n; y: n x 4 u64. */
int vc_kzg_prove_many(vc_ctx* ctx, int table, size_t N, size_t rows, size_t width, const uint64_t* data,
                      const uint32_t* row, const uint64_t* points, size_t n, uint64_t* proof_xy, uint8_t* proof_inf,
                      uint64_t* y);
/* same with the rows already in device memory (rows x width canonical values, 4 u64 each) */
int vc_kzg_prove_many_device(vc_ctx* ctx, int table, size_t N, size_t rows, size_t width, const void* d_data,
                             const uint32_t* row, const uint64_t* points, size_t n, uint64_t* proof_xy,
                             uint8_t* proof_inf, uint64_t* y);
/* Subvector proofs: one constant-size proof that k positions of one committed row hold k values --
 * what the reference's prove_batch / verify_batch name (kzg/mod.rs:156-163, 191-197) and leave
 * todo!(). Domain of size N with generator w, row f (zero beyond `width`), S a set of k distinct
 * indices below N, Z_S(X) = prod_{i in S} (X - w^i), I the polynomial of degree < k with
 * I(w^i) = f_i on S. The proof is pi_S = [q(s)]_1 with q = (f - I) / Z_S, the values are y_i = f_i
 * in the caller's index order, and the verifier accepts when
 *   e(pi_S, [Z_S(s)]_2) == e(C - [I(s)]_1, H).
 * With c_i = 1 / Z_S'(w^i) = prod_{l in S, l != i} 1 / (w^i - w^l): q = sum_{i in S} c_i q^(i), q^(i)
 * the single-point quotient of index i, hence pi_S = sum_i c_i pi_i over vc_kzg_prove's proofs.
 * k = 1 is vc_kzg_prove at that index; k = N gives the identity.
 *
 * n subsets in one call: subset s is idx[idx_off[s] .. idx_off[s + 1]) (1 <= k_s <= N) and proves
 * row row[s] (row == NULL: row s, and then rows == n) of `data`, as vc_kzg_prove_many's rows. The
 * proof does not depend on the order of a subset's indices; y[p] is the value at idx[p]. Per chunk
 * of at most 16,384 subsets: one field launch, a wave per subset, and one batched fixed-base commit.
 * BN254 and BLS12-381, 2 <= N <= 1024.
 * A status other than VC_OK is decided on the host before any GPU work and leaves the outputs
 * untouched: VC_E_INVALID (an index >= N, a repeated index inside one subset, an empty subset, a
 * non-monotone idx_off, or any of vc_kzg_prove_many's argument rules), VC_E_RANGE, VC_E_TABLE as
 * there. n == 0 is VC_OK.
 * idx_off: n + 1 u32; idx: idx_off[n] u32; proof_xy: n x 2 NL u64; proof_inf: n; y: idx_off[n] x 4 u64. */
int vc_kzg_prove_subvector_many(vc_ctx* ctx, int table, size_t N, size_t rows, size_t width, const uint64_t* data,
                                const uint32_t* row, const uint32_t* idx_off, const uint32_t* idx, size_t n,
                                uint64_t* proof_xy, uint8_t* proof_inf, uint64_t* y);
/* same with the rows already in device memory (rows x width canonical values, 4 u64 each) */
int vc_kzg_prove_subvector_many_device(vc_ctx* ctx, int table, size_t N, size_t rows, size_t width,
                                       const void* d_data, const uint32_t* row, const uint32_t* idx_off,
                                       const uint32_t* idx, size_t n, uint64_t* proof_xy, uint8_t* proof_inf,
                                       uint64_t* y);
/* the k canonical weights c_i of the set idx[0 .. k) in the domain of size N (host, no context;
 * curve: VC_CURVE_BN254 or VC_CURVE_BLS12_381), for an aggregator that holds single proofs already
 * (vc_kzg_prove_all_points mode 1, vc_kzg_prove_many) and forms sum c_i pi_i with the MSM calls.
 * VC_E_INVALID: N not a power of two in [2, 2^28], k == 0, an index >= N, a repeated index. */
int vc_kzg_subvector_weights(int curve, size_t N, const uint32_t* idx, size_t k, uint64_t* c_out);
/* [s^t]_1 for t < K from the Lagrange SRS alone (no secret): K batched commits of the rows
 * (w^(j t))_j. out: K x 2 NL u64. 2 <= N <= 1024; VC_E_RANGE for K > N or a table with fewer than
 * N points; VC_E_INVALID for K == 0 or when a power is the identity (s = 0 is no setup). */
int vc_kzg_g1_powers(vc_ctx* ctx, int table, size_t N, size_t K, uint64_t* out);
/* commit + prove_point in one call (configs[3]'s unit): C = commit(evals) (kzg/mod.rs:126-134) and
 * the proof at `point` as vc_kzg_prove_device; both MSMs over the SRS run as one batched
 * pipeline (vc_msm_device_many). */
int vc_kzg_commit_prove_device(vc_ctx* ctx, int table, size_t size, const void* d_evals, size_t max,
                               const uint64_t* point, uint64_t* com_xy, uint8_t* com_inf, uint64_t* proof_xy,
                               uint8_t* proof_inf, uint64_t* y);
/* multi-GPU open: the quotient (every part computes it; it is elementwise and ~10 % of the
 * MSM) and window slice `part` of `parts` of the proof MSM as an un-normalised accumulator;
 * the parts' accumulators sum (vc_partials_sum) to the proof */
int vc_kzg_prove_device_part(vc_ctx* ctx, int table, size_t size, const void* d_evals, size_t max,
                             const uint64_t* point, int part, int parts, uint32_t* out_acc, uint64_t* y);
/* KZG::prove_all_points (kzg/mod.rs:200-235), the FK amortised opening -- private and never
 * called in the reference (its test at :299 has no #[test]). table = the Lagrange SRS of domain
 * `size`; evals = n_evals values (the data's own domain is next_pow2(n_evals), as
 * LagrangeBasis::from_vec). Outputs *count points (out_xy, out_inf) and values (out_y = data[i]).
 *   mode 0: the reference's computation exactly -- coefficients c of the data's interpolant of
 *     degree d, c_hat = [c_d, 0^(d+1), c_0 .. c_{d-1}] cut to the domain D::new(2 d), g1 =
 *     ifft(lagrange SRS) over the key domain, s_hat = reverse(g1[0..d]) || 0, h_hat =
 *     ifft(fft(s_hat) .* fft(c_hat)); returns (h_hat[i], data[i]) for i < that domain.
 *     VC_E_DOMAIN where the reference panics: all-zero data (coeffs[degree] of an empty
 *     polynomial), a domain larger than the data (data[i] out of bounds), d > size.
 *   mode 1: the opening proofs FK computes (what the reference's test expects): for every i <
 *     size, pi_i = [q_i(s)]_1 with q_i = (f - f(w^i)) / (X - w^i) -- the Toeplitz product of the
 *     coefficients with the monomial SRS fft(lagrange SRS) by a 2 size circulant, then an FFT.
 *     Equal to vc_kzg_prove at index i; n_evals <= size (VC_E_RANGE otherwise).
 * out_xy: count x 2 NL u64 (count <= size, or the mode-0 domain); out_y: count x 4 u64. */
int vc_kzg_prove_all_points(vc_ctx* ctx, int table, size_t size, const uint64_t* evals, size_t n_evals, int mode,
                            uint64_t* out_xy, uint8_t* out_inf, uint64_t* out_y, size_t* count);
/* the quotient alone (a5/a6), for parity tests: q (size x 4 u64) and y */
int vc_kzg_quotient(vc_ctx* ctx, size_t size, const uint64_t* evals, size_t max, const uint64_t* point,
                    uint64_t* q_out, uint64_t* y);

/* ---------------------------------------------------------------- multiproof (multiproof.rs)
 * scheme: 0 = IPA (table = N + 1 CRS points), 1 = KZG (table = Lagrange SRS of size N).
 * queries: data Q x N (Fr), commitments Q, z Q (u64, < N), y Q (Fr).
 * Output: proof D and the inner proof (IPA proof or KZG (proof point, y)). */
int vc_multiproof_prove(vc_ctx* ctx, int scheme, int table, size_t N, size_t Q, const uint64_t* data,
                        const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z,
                        const uint64_t* y, uint64_t* d_xy, uint8_t* d_inf, vc_ipa_proof* ipa_proof,
                        uint64_t* kzg_proof_xy, uint8_t* kzg_proof_inf, uint64_t* kzg_y);
/* The same prover in three phases, so the Q x N field phase shards over GPUs with one
 * exchange. vc_multiproof_prove == begin + accumulate(all Q) + finish(G=1).
 * phase 1 (host, every rank): transcript over all (C, z, y) (:106-114), challenge r
 *   (canonical), and the number of distinct query points `rows` (the rows of S). Pure host code,
 *   safe to call from several threads at once: above 4096 queries each call runs one filler
 *   thread of its own beside its SHA-256 (not the shared host pool), so concurrent transcripts
 *   proceed side by side. */
int vc_multiproof_begin(size_t N, size_t Q, const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z,
                        const uint64_t* y, vc_transcript** transcript, uint64_t* r, size_t* rows);
/* phase 2 (device, per shard): S[row][k] = sum r^i f_i[k] over queries i in [first, first + Qs)
 *   grouped by point; d_data = that slice's Qs x N evaluations (canonical, device); d_S =
 *   rows x N x 4 u64 (canonical, device). z = ALL Q points (it fixes the rows). */
int vc_multiproof_accumulate(vc_ctx* ctx, size_t N, size_t Q, const uint64_t* z, size_t first, size_t Qs,
                             const void* d_data, const uint64_t* r, void* d_S);
/* phases 1 + 2 in one call, the host transcript on a helper thread while the calling thread sorts
 *   this shard's queries by point and uploads the plan (only the per-point sums wait for r): the
 *   same transcript, r and S as vc_multiproof_begin + vc_multiproof_accumulate. rows (the size of
 *   d_S) from vc_multiproof_rows. On error no transcript is returned. */
int vc_multiproof_rows(size_t N, size_t Q, const uint64_t* z, size_t* rows);
int vc_multiproof_begin_accumulate(vc_ctx* ctx, size_t N, size_t Q, const uint64_t* com_xy, const uint8_t* com_inf,
                                   const uint64_t* z, const uint64_t* y, size_t first, size_t Qs, const void* d_data,
                                   void* d_S, vc_transcript** transcript, uint64_t* r);
/* phase 3: G shards' S matrices (device, contiguous, e.g. an all-gather) are summed; then
 *   quotients, g, D, t, h, E and the inner proof (:129-175). Advances `transcript`. */
int vc_multiproof_finish(vc_ctx* ctx, int scheme, int table, size_t N, size_t Q, const uint64_t* z,
                         const void* d_S_parts, int G, vc_transcript* transcript, uint64_t* d_xy, uint8_t* d_inf,
                         vc_ipa_proof* ipa_proof, uint64_t* kzg_proof_xy, uint8_t* kzg_proof_inf, uint64_t* kzg_y);
/* Proof-parallel: P independent multiproofs of Q queries each on one GPU (a caller proving
 * several blocks). Per proof the result is vc_multiproof_prove's; the host transcripts run on
 * worker threads beside the GPU's per-point sums, and the D / E commits and (IPA) the inner
 * proofs run once for all P proofs (batched). Layouts: com_xy [P][Q][8], com_inf [P][Q],
 * z [P][Q], y [P][Q][4] (host); d_data [P][Q][N] x 4 u64 canonical (device); outputs d_xy [P][8],
 * d_inf [P], and ipa_proofs[P] (scheme 0, each with caller-owned round arrays) or
 * kzg_xy [P][8], kzg_inf [P], kzg_y [P][4] (scheme 1). */
int vc_multiproof_prove_many(vc_ctx* ctx, int scheme, int table, size_t N, size_t Q, size_t P, const void* d_data,
                             const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z, const uint64_t* y,
                             uint64_t* d_xy, uint8_t* d_inf, vc_ipa_proof* ipa_proofs, uint64_t* kzg_xy,
                             uint8_t* kzg_inf, uint64_t* kzg_y);
/* IPA-scheme verification (verify_multiproof :178-215 + low_level_verify_ipa) */
int vc_multiproof_verify_ipa(vc_ctx* ctx, int table, size_t N, size_t Q, const uint64_t* com_xy,
                             const uint8_t* com_inf, const uint64_t* z, const uint64_t* y,
                             const uint64_t* d_xy, uint8_t d_inf, const vc_ipa_proof* proof, int* result);
/* KZG-scheme: the (commitment E - D, t) pair verify_point checks with pairings, for a caller
 * that runs its own pairing check (vc_multiproof_verify_kzg below runs this library's). */
int vc_multiproof_kzg_claim(vc_ctx* ctx, size_t N, size_t Q, const uint64_t* com_xy, const uint8_t* com_inf,
                            const uint64_t* z, const uint64_t* y, const uint64_t* d_xy, uint8_t d_inf,
                            uint64_t* c_xy, uint8_t* c_inf, uint64_t* t);

/* ---------------------------------------------------------------- KZG verification (pairings)
 * KZG::verify_point (kzg/mod.rs:165-189) with the BN254 optimal-ate pairing (csrc/pairing.hpp).
 * G2 points: 16 canonical little-endian u64, x.c0[4] x.c1[4] y.c0[4] y.c1[4] (an Fq2 element is
 * c0 + c1 u, u^2 = -1), on the twist y^2 = x^3 + 3 / (9 + u), plus a u8 identity flag.
 * The check is e(proof, [s]_2) e(y G - C - p proof, H) == 1 with p = omega^point for
 * point < size and the point itself otherwise (the reference's `<` at :172).
 * A malformed key is VC_E_INVALID. A malformed proof entry -- a G1 point off the curve, a
 * coordinate >= p, an Fr value >= r -- gives the verdict 0 and VC_OK. The identity is a valid G1
 * input. Every call except vc_kzg_verify_many, vc_multiproof_verify_kzg and the device path
 * of vc_kzg_batch_fold / vc_kzg_verify_batch (ctx != NULL) is host code that needs no context and
 * no GPU. */
typedef struct vc_kzg_vk vc_kzg_vk;
/* [secret]_2 = secret * H, what KZG::setup computes at kzg/mod.rs:122 (H: the G2 generator) */
int vc_kzg_g2_from_secret(const uint64_t* secret_fr, uint64_t* out_g2_xy, uint8_t* out_g2_inf);
/* the verifying key of a domain of `size` (a power of two): checks [s]_2 (on the twist, of order
 * r, not the identity), tabulates the Miller-loop lines of [s]_2 and H */
int vc_kzg_vk_new(const uint64_t* g2_xy, uint8_t g2_inf, size_t size, vc_kzg_vk** vk);
void vc_kzg_vk_free(vc_kzg_vk* vk);
/* one opening on the host; result 1 = valid, 0 = invalid */
int vc_kzg_verify(const vc_kzg_vk* vk, const uint64_t* com_xy, uint8_t com_inf, const uint64_t* point_fr,
                  const uint64_t* proof_xy, uint8_t proof_inf, const uint64_t* y_fr, int* result);
/* result 1 when prod e(P_i, Q_i) == 1 (lines computed on the fly). Q_i arbitrary points of G2:
 * VC_E_INVALID for a G1 / G2 input off its curve or a G2 input outside the subgroup; identities
 * on either side pair to one. */
int vc_bn254_pairing_check(size_t n, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                           const uint8_t* g2_inf, int* result);
/* n independent openings on the device, one lane each: results[i] = 1 / 0 as vc_kzg_verify of
 * entry i (com_xy n x 8, points n x 4, proof_xy n x 8, y n x 4 u64; flags n). The key's line
 * tables are uploaded into ctx on first use. */
int vc_kzg_verify_many(vc_ctx* ctx, const vc_kzg_vk* vk, size_t n, const uint64_t* com_xy, const uint8_t* com_inf,
                       const uint64_t* points, const uint64_t* proof_xy, const uint8_t* proof_inf,
                       const uint64_t* y, uint8_t* results);
/* One combined check for n openings ("are all of these valid?"; the reference names it
 * verify_batch, kzg/mod.rs:190-196, and leaves it todo!()). With one challenge rho and the
 * weights rho^i (i = 0 .. n-1), p_i as in the check above:
 *   P1 = sum rho^i pi_i,  P2 = (sum rho^i y_i) G - sum rho^i C_i - sum (rho^i p_i) pi_i,
 *   accept  <=>  e(P1, [s]_2) e(P2, H) == 1.
 * A batch of valid entries is accepted for every rho; a batch with an invalid entry is accepted
 * for at most n - 1 of the r values of rho. rho = vc_hash_to_field(seed, 32, dst =
 * "vkzg-kzg-batch"): the verifier draws the seed itself once it holds the inputs (no hash over the
 * inputs); a given seed makes the call deterministic. Layouts are vc_kzg_verify_many's. */
/* rho for a seed (host, no context) */
int vc_kzg_batch_challenge(const uint8_t seed[32], uint64_t* rho_fr);
/* the fold alone: P1, P2 as canonical affine points. *malformed = 1 (points unspecified) when any entry
 * is malformed in vc_kzg_verify_many's sense: a coordinate >= p, a point off the curve, y or point >= r.
 * ctx == NULL: host path (host pool), any n.  ctx != NULL: device path, BN254 context.
 * VC_E_INVALID: a null key, a context that is not BN254, null arrays with n > 0, rho_fr >= r. */
int vc_kzg_batch_fold(vc_ctx* ctx, const vc_kzg_vk* vk, size_t n, const uint64_t* com_xy, const uint8_t* com_inf,
                      const uint64_t* points, const uint64_t* proof_xy, const uint8_t* proof_inf, const uint64_t* y,
                      const uint64_t* rho_fr, uint64_t* p1_xy, uint8_t* p1_inf, uint64_t* p2_xy, uint8_t* p2_inf,
                      int* malformed);
/* *result = 1 when the combined check accepts, else 0. seed == NULL: 32 bytes of OS entropy (getrandom).
 * results: NULL, or n bytes. When the combined check accepts they are all 1 and no per-opening pairing
 * runs. When it rejects (a malformed entry included) they are vc_kzg_verify_many's verdicts, so ctx is
 * required (VC_E_INVALID with ctx == NULL and results != NULL). n = 0: VC_OK, *result = 1.
 * A malformed proof entry gives *result = 0 with VC_OK; the identity flag is a valid input for C_i
 * and pi_i. The device path works in chunks of at most 2^20 entries: its workspace does not grow
 * with n. */
int vc_kzg_verify_batch(vc_ctx* ctx, const vc_kzg_vk* vk, size_t n, const uint64_t* com_xy, const uint8_t* com_inf,
                        const uint64_t* points, const uint64_t* proof_xy, const uint8_t* proof_inf, const uint64_t* y,
                        const uint8_t* seed32, int* result, uint8_t* results);
/* verify_multiproof for KZG (multiproof.rs:178-215): vc_multiproof_kzg_claim's computation,
 * then vc_kzg_verify of (E - D, t, inner proof) */
int vc_multiproof_verify_kzg(vc_ctx* ctx, const vc_kzg_vk* vk, size_t N, size_t Q, const uint64_t* com_xy,
                             const uint8_t* com_inf, const uint64_t* z, const uint64_t* y, const uint64_t* d_xy,
                             uint8_t d_inf, const uint64_t* kzg_proof_xy, uint8_t kzg_proof_inf,
                             const uint64_t* kzg_y, int* result);

/* ---- P multiproofs in one call, one verdict each (csrc/mp_verify.hip): the transcripts, the
 * coefficients r^i / (t - z_i), the sums E_p, the claims E_p - D_p and the inner verification all
 * run on the device, per chunk of at most 8,192 proofs and 2^18 queries (the workspace does not
 * grow with P); nothing of a proof crosses to the host before the verdicts (or claims) come back.
 * Layout: proof p owns queries [q_ptr[p], q_ptr[p + 1]) of the flat query arrays (q_ptr: P + 1
 * ascending offsets; com_xy total x 8, com_inf total, z total, y total x 4 u64); q_ptr == NULL: every
 * proof has Q queries, vc_multiproof_prove_many's [P][Q] layout (Q is not read otherwise). d_xy
 * P x 8, d_inf P. The inner IPA proofs in vc_ipa_verify_many's flat layout (l_xy / r_xy P x K x 8,
 * l_inf / r_inf P x K, tip and ipa_y P x 4, K = log2 N), the inner KZG proofs in
 * vc_kzg_verify_many's (kzg_xy P x 8, kzg_inf P, kzg_y P x 4). All values canonical.
 * results[p] is what vc_multiproof_verify_ipa / _kzg gives for proof p wherever that call returns
 * VC_OK. Malformed proof content gives the verdict 0 with VC_OK, as in the other _many verifiers:
 * a coordinate of a C_i, of D or of an inner point >= p, such a point off the curve, a y_i, tip or
 * inner y >= r. No entry changes another's verdict; the identity flag is a valid point.
 * vc_multiproof_claims_many reports such an entry in malformed[p] (its outputs unspecified) and
 * otherwise gives vc_multiproof_kzg_claim's (E - D, t) bit for bit (c_xy P x 8, zero for the
 * identity, c_inf P, t P x 4). The coefficients are mp_claim's: the denominator is t - z_i with z_i
 * the integer. A t that is itself an integer below N (no test can produce one: it is a hash) gives
 * the entry the verdict 0 / malformed 1.
 * Statuses, decided on the host before any GPU work with nothing written: VC_E_INVALID for N not a
 * power of two in [2, 2^28] (the inner many-verifiers' bound), a context or key that is not BN254,
 * a null array with P > 0, a q_ptr that is not ascending, a proof with 0 or more than VC_MPV_Q_MAX
 * queries (long proofs stay with the single call, where the host's SHA-256 beats one lane's), for
 * IPA a table with fewer than N + 1 points; VC_E_TABLE for an unknown table; then VC_E_DOMAIN for
 * the whole call when any z_i >= N (the verifier's own input, as in the single call). P = 0 is
 * VC_OK. */
#define VC_MPV_Q_MAX 4096
int vc_multiproof_claims_many(vc_ctx* ctx, size_t N, size_t P, const uint64_t* q_ptr, size_t Q,
                              const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z, const uint64_t* y,
                              const uint64_t* d_xy, const uint8_t* d_inf, uint64_t* c_xy, uint8_t* c_inf, uint64_t* t,
                              uint8_t* malformed);
int vc_multiproof_verify_many_ipa(vc_ctx* ctx, int table, size_t N, size_t P, const uint64_t* q_ptr, size_t Q,
                                  const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z,
                                  const uint64_t* y, const uint64_t* d_xy, const uint8_t* d_inf, const uint64_t* l_xy,
                                  const uint8_t* l_inf, const uint64_t* r_xy, const uint8_t* r_inf, const uint64_t* tip,
                                  const uint64_t* ipa_y, uint8_t* results);
int vc_multiproof_verify_many_kzg(vc_ctx* ctx, const vc_kzg_vk* vk, size_t N, size_t P, const uint64_t* q_ptr,
                                  size_t Q, const uint64_t* com_xy, const uint8_t* com_inf, const uint64_t* z,
                                  const uint64_t* y, const uint64_t* d_xy, const uint8_t* d_inf, const uint64_t* kzg_xy,
                                  const uint8_t* kzg_inf, const uint64_t* kzg_y, uint8_t* results);

/* ---------------------------------------------------------------- KZG verification on BLS12-381
 * A verifying key has a curve: VC_CURVE_BN254 (every call above that takes no curve argument, as
 * before) or VC_CURVE_BLS12_381 (csrc/pairing_bls.hpp: the ate pairing over the 64 bits of
 * |x|, x = -0xd201000000010000). vc_kzg_verify, vc_kzg_verify_many, vc_kzg_batch_fold and
 * vc_kzg_verify_batch dispatch on the key's curve; their contracts are the ones above with the
 * BLS12-381 layouts below. A context whose curve is not the key's is VC_E_INVALID.
 * vc_multiproof_verify_kzg and the verkle calls stay BN254: VC_E_INVALID for a BLS12-381 key.
 *
 * BLS12-381 layouts (canonical little-endian u64):
 *   Fr   4 u64, below r.
 *   G1   12 u64: x[6] y[6], below p, on y^2 = x^3 + 4 (vc_kzg_prove_many's 2 NL), plus a u8
 *        identity flag. So com_xy / proof_xy are n x 12 and p1_xy / p2_xy are 12 u64.
 *   G2   24 u64: x.c0[6] x.c1[6] y.c0[6] y.c1[6] (an Fq2 element is c0 + c1 u, u^2 = -1), on the
 *        twist y^2 = x^3 + 4 (1 + u), plus a u8 identity flag.
 * The domain generator is omega = 7^((r - 1) / size), vc_kzg_setup's for this curve.
 *
 * Status and verdict rules are the BN254 ones with one addition. G1 of BLS12-381 has a cofactor,
 * and a point of E(Fq) outside the subgroup of order r pairs to one with every point of G2
 * (pi + T, T of small order, would verify whenever pi does). So a G1 input that is on the curve
 * but outside the subgroup is malformed, exactly as a point off the curve is: verdict 0 with VC_OK
 * in vc_kzg_verify / vc_kzg_verify_many, *malformed = 1 in vc_kzg_batch_fold, *result = 0 with
 * VC_OK in vc_kzg_verify_batch, VC_E_INVALID in vc_bls12_381_pairing_check. The test is
 * phi^2(P) + [x^2] P == O, the one the MSM runs over whole tables; it is complete. The identity
 * flag is a valid input and is not tested; flagged coordinates are not read.
 * A malformed key ([s]_2 with a coordinate >= p, off the twist, outside the subgroup of order r,
 * or the identity) is VC_E_INVALID, as is a curve other than the two above. */
/* [secret]_2 = secret * H on the curve (H: its standard G2 generator); secret below the curve's r */
int vc_kzg_g2_from_secret_curve(int curve, const uint64_t* secret_fr, uint64_t* out_g2_xy, uint8_t* out_g2_inf);
/* vc_kzg_vk_new for the curve; g2_xy in the curve's G2 layout (16 or 24 u64) */
int vc_kzg_vk_new_curve(int curve, const uint64_t* g2_xy, uint8_t g2_inf, size_t size, vc_kzg_vk** vk);
/* vc_kzg_batch_challenge for the curve: hash_to_field(seed, dst = "vkzg-kzg-batch") reduced mod
 * the curve's r (48 expanded bytes for both curves) */
int vc_kzg_batch_challenge_curve(int curve, const uint8_t seed[32], uint64_t* rho_fr);
/* vc_bn254_pairing_check's contract on BLS12-381 (g1_xy n x 12, g2_xy n x 24 u64): VC_E_INVALID
 * also for a G1 input outside the subgroup */
int vc_bls12_381_pairing_check(size_t n, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                               const uint8_t* g2_inf, int* result);

/* ---------------------------------------------------------------- KZG subvector verification
 * The verifier of vc_kzg_prove_subvector_many's proofs (the statement is there). Host code on both
 * curves, no context, no GPU. Its key holds powers of s: [s^t]_1 for t < K and [s^t]_2 for t <= K,
 * in the curve's G1 / G2 layouts without identity flags, and verifies sets of up to K indices. */
typedef struct vc_kzg_svk vc_kzg_svk;
/* the powers from the secret, the counterpart of vc_kzg_g2_from_secret for tests and trusted setups
 * (g1_out: K x 2 NL u64, g2_out: (K + 1) x 4 NL u64). VC_E_INVALID for K == 0, a secret >= r or 0. */
int vc_kzg_powers_from_secret(int curve, const uint64_t* secret_fr, size_t K, uint64_t* g1_out, uint64_t* g2_out);
/* The key of a domain of `size` (a power of two in [2, 2^28]), 1 <= K <= size. Every point is checked:
 * coordinates below p, on its curve, G2 in the subgroup of order r (on BLS12-381 G1 too),
 * g1[0] = G and g2[0] = H; anything else is VC_E_INVALID. That the powers belong to one s is NOT
 * checked (it would take a pairing per power): the key is trusted input, as an SRS is. */
int vc_kzg_svk_new(int curve, size_t size, size_t K, const uint64_t* g1_powers, const uint64_t* g2_powers,
                   vc_kzg_svk** svk);
void vc_kzg_svk_free(vc_kzg_svk* svk);
/* One subvector proof: *result = 1 when e(pi, [Z_S(s)]_2) == e(C - [I(s)]_1, H), else 0. idx: k
 * indices, y: k x 4 u64 in the indices' order (any order, the y permuted with the indices).
 * The monomial coefficients of Z_S and of I = sum y_i c_i Z_S / (X - w^i) cost O(k^2) field
 * multiplies; [Z_S(s)]_2 and [I(s)]_1 are joint double-and-adds over the key's powers.
 * VC_E_RANGE for k > K; VC_E_INVALID for a bad index set (k == 0, an index >= size, a repeated
 * index: the verifier's own input) or a null argument. Malformed proof content -- a coordinate >= p,
 * a point off the curve, a y >= r, on BLS12-381 a G1 point outside the subgroup -- gives *result = 0
 * with VC_OK, as vc_kzg_verify_many. The identity flag is a valid C and a valid proof. */
int vc_kzg_verify_subvector(const vc_kzg_svk* svk, const uint64_t* com_xy, uint8_t com_inf, const uint32_t* idx,
                            size_t k, const uint64_t* y, const uint64_t* proof_xy, uint8_t proof_inf, int* result);

/* ---------------------------------------------------------------- KZG subvector batch verification
 * n subvector proofs (C_j, S_j, y_j, pi_j), one combined verdict: are all of them valid? With one
 * challenge rho and the weights rho^j the coefficients of Z_j = sum_t z_{j,t} X^t and
 * I_j = sum_t a_{j,t} X^t move onto the G1 side (Kmax = max_j |S_j|, z_{j,t} = 0 above |S_j|):
 *   P_t = sum_j rho^j z_{j,t} pi_j (t = 0 .. Kmax),  a_t = sum_j rho^j a_{j,t} (t < Kmax),
 *   P_H = P_0 + sum_t a_t [s^t]_1 - sum_j rho^j C_j,
 *   accept  <=>  e(P_H, H) prod_{t = 1 .. Kmax} e(P_t, [s^t]_2) == 1.
 * The left side is prod_j E_j^(rho^j), E_j the single verifier's product: a batch with an invalid
 * entry is accepted for at most n - 1 values of rho (D(rho) = sum_j d_j rho^j). Every G2 point is a
 * point of the key; their Miller lines are tabulated on the first batch call of a key (once,
 * thread-safe; vc_kzg_svk_new makes none), and the check is one multi-Miller loop over the host pool
 * with one final exponentiation.
 *
 * Layout, vc_kzg_prove_subvector_many's: com_xy / proof_xy n x 2 NL u64 with n identity flags,
 * idx_off n + 1 u32, idx idx_off[n] u32, y idx_off[n] x 4 u64, y[p] belonging to idx[p].
 * ctx: a context of the key's curve; the device path takes domains of 2 <= size <= 1024 (the
 * prover's; VC_E_RANGE above). ctx == NULL: the same fold on the host pool, for any size the key takes
 * (the check of the fold on a machine without a GPU, not a product path).
 *
 * Status, decided on the host before any GPU work, the outputs untouched: VC_E_INVALID for an index
 * >= size, a repeated index inside one set, an empty set, a non-monotone idx_off, a null argument,
 * rho >= r, a context whose curve is not the key's; VC_E_RANGE for a set of more than K indices.
 * Malformed proof content -- a coordinate >= p, a point off the curve, a y >= r, on BLS12-381 a G1
 * point outside the subgroup -- is *malformed = 1 (vc_kzg_subvector_batch_fold) or *result = 0
 * (vc_kzg_verify_subvector_batch) with VC_OK. The identity flag is a valid C_j and a valid pi_j. */
/* rho for a seed: hash_to_field(seed, dst = "vkzg-kzg-subv-batch") reduced mod the curve's r */
int vc_kzg_subvector_batch_challenge(int curve, const uint8_t seed[32], uint64_t* rho_fr);
/* The fold alone: *kmax_out = Kmax and Kmax + 1 canonical affine points with identity flags, P_H
 * first, then P_1 .. P_Kmax (p_xy: room for (K + 1) x 2 NL u64, p_inf: K + 1). n == 0: Kmax = 0 and
 * P_H the identity. With *malformed = 1 the points are not written. */
int vc_kzg_subvector_batch_fold(vc_ctx* ctx, const vc_kzg_svk* svk, size_t n, const uint64_t* com_xy,
                                const uint8_t* com_inf, const uint32_t* idx_off, const uint32_t* idx,
                                const uint64_t* y, const uint64_t* proof_xy, const uint8_t* proof_inf,
                                const uint64_t* rho_fr, size_t* kmax_out, uint64_t* p_xy, uint8_t* p_inf,
                                int* malformed);
/* *result = 1 when the combined check accepts. seed32: 32 bytes the verifier draws after it holds the
 * inputs (a given seed makes the call deterministic); NULL draws OS entropy. results: NULL, or n
 * bytes: all 1 on accept, vc_kzg_verify_subvector's verdicts (over the host pool; they need no
 * context) on reject. n == 0: VC_OK with *result = 1. */
int vc_kzg_verify_subvector_batch(vc_ctx* ctx, const vc_kzg_svk* svk, size_t n, const uint64_t* com_xy,
                                  const uint8_t* com_inf, const uint32_t* idx_off, const uint32_t* idx,
                                  const uint64_t* y, const uint64_t* proof_xy, const uint8_t* proof_inf,
                                  const uint8_t* seed32, int* result, uint8_t* results);

#ifdef __cplusplus
}
#endif
#endif /* VC_SCHEME_H */

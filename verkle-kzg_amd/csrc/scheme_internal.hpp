// Internal declarations shared by the protocol-layer translation units.
#pragma once
#include <stdint.h>

#include <functional>
#include <vector>

#include "../../include/vc_scheme.h"
#include "host/fr.hpp"

namespace vk {

Fr transcript_digest(vc_transcript* t, const char* label);
void transcript_append_point(vc_transcript* t, const uint64_t* xy, bool inf, const char* label);
void transcript_append_fr(vc_transcript* t, const Fr& mont, const char* label);
void expand_message_xmd(const uint8_t* msg, size_t n, const uint8_t* dst, size_t dlen, size_t out_len, uint8_t* out);
// ark-ff 0.4 DefaultFieldHasher<Sha256, 128> into the scalar field F: ceil((bits + 128) / 8) = 48
// bytes for a 254- or a 255-bit modulus, read big-endian and reduced mod r (Montgomery out)
template <class F = BN254Fr>
inline fe<F> hash_to_fr(const uint8_t* msg, size_t n, const uint8_t* dst, size_t dlen) {
    uint8_t u[48];
    expand_message_xmd(msg, n, dst, dlen, sizeof u, u);
    return fe_from_be_bytes_mod<F>(u, sizeof u);
}
void compress_g1(const uint64_t* xy, bool inf, uint8_t out[32]);
// grow the transcript state by n bytes and return the start of the new region (callers that
// serialise many records on several threads)
uint8_t* transcript_extend(vc_transcript* t, size_t n);
// transcript_digest of the state followed by nrec records of rec bytes (made by fill(lo, hi, out)
// chunk by chunk, never stored whole) and the label; pool_ok: make them on the host pool
using RecordFill = std::function<void(size_t lo, size_t hi, uint8_t* out)>;
Fr transcript_digest_records(vc_transcript* t, size_t nrec, size_t rec, const RecordFill& fill, const char* label,
                             bool pool_ok);
int kzg_vk_curve(const vc_kzg_vk* vk);  // the key's curve (pairing_host.cpp)
Fr to_data_item_host(const uint64_t* xy, bool inf);
// [w, x_0 .. x_{K-1}] (Montgomery) of entries [lo, lo + cnt) of vc_ipa_verify_many's arrays into
// chal[0 .. cnt (K + 1)), on the host pool; transcripts: NULL, or handles indexed by entry (NULL:
// fresh "ipa"), advanced as vc_ipa_verify advances them (ipa_verify.hip)
void ipa_host_challenges(size_t lo, size_t cnt, int K, const uint64_t* com_xy, const uint8_t* com_inf,
                         const uint64_t* points, const uint64_t* y, const uint64_t* l_xy, const uint8_t* l_inf,
                         const uint64_t* r_xy, const uint8_t* r_inf, vc_transcript** transcripts, Fr* chal);

// ---- host helpers of the protocol layer, BN254 (scheme.hip describes them)
struct Table;
// ---- the inner many-verifiers over device arrays (the multiproof many-verifier, mp_verify.hip)
// vc_ipa_verify_many's device half (ipa_verify.hip): a workspace for chunks of <= chunk proofs of
// size N, then per chunk the field kernel, the fixed commit and the curve kernel over device
// arrays in vc_ipa_verify_many's layouts (32-bit words) and device challenges [w, x_0 .. x_{K-1}]
// (Montgomery). The point arrays are rewritten. laps: null, or {field, fixed commit, curve} sums in us.
struct IpaVerifyWork;
int ipa_verify_work_new(vc_ctx* ctx, size_t N, size_t chunk, IpaVerifyWork** out);
void ipa_verify_work_free(IpaVerifyWork* w);
int ipa_verify_dev(vc_ctx* ctx, Table* t, IpaVerifyWork* w, size_t cnt, const uint32_t* d_chal, const uint32_t* d_tip,
                   const uint32_t* d_y, const uint32_t* d_point, uint32_t* d_com, const uint8_t* d_cinf, uint32_t* d_l,
                   const uint8_t* d_linf, uint32_t* d_r, const uint8_t* d_rinf, uint8_t* d_out, double* laps);
// vc_kzg_verify_many's kernel over device arrays, BN254 key (pairing.hip): n verdict bytes at d_out
int kzg_verify_dev(vc_ctx* ctx, const vc_kzg_vk* vk, size_t n, const uint32_t* d_com, const uint8_t* d_cinf,
                   const uint32_t* d_points, const uint32_t* d_proof, const uint8_t* d_pinf, const uint32_t* d_y,
                   uint8_t* d_out);
BN254G1::Acc acc_of(const uint64_t* xy, bool inf);  // canonical affine (or the identity) -> accumulator
void aff_of(const BN254G1::Acc& a, uint64_t* xy, uint8_t* inf);
std::vector<Fr> host_batch_inv(const std::vector<Fr>& v);  // 1 / 0 = 0
std::vector<Fr> barycentric(size_t size, const Fr& point, const Fr& omega);
bool barycentric_panics(size_t size, const Fr& point);
int commit_batch(vc_ctx* ctx, Table* t, size_t width, const Fr* sc, size_t batch, uint64_t* out_xy, uint8_t* out_inf,
                 const std::function<void()>* overlap = nullptr);
constexpr size_t HOST_MSM_MAX = 64;
int host_msm(const uint64_t* xy, const uint8_t* inf, const Fr* sc, size_t n, BN254G1::Acc* out);
int msm_points(vc_ctx* ctx, const uint64_t* xy, const uint8_t* inf, const std::vector<Fr>& sc, BN254G1::Acc* out,
               bool filled = false);

// ---- what the multiproof takes from the other protocols
// trs: NULL, or per proof NULL (a fresh "ipa") or the transcript to continue (ipa.hip)
int ipa_prove_impl(vc_ctx* ctx, Table* t, size_t N, const std::vector<std::vector<Fr>>& data,
                   const std::vector<BN254G1::Acc>& coms, const std::vector<Fr>& points, vc_transcript** trs,
                   vc_ipa_proof* proofs);
int ipa_verify_impl(vc_ctx* ctx, Table* t, size_t N, const BN254G1::Acc& com, const Fr& point, const vc_ipa_proof* pr,
                    vc_transcript* tr_in, int* result);
// the BN254 opening of `size` canonical host evaluations at a canonical point (kzg_open.hip)
int kzg_open_bn254(vc_ctx* ctx, Table* t, size_t size, const uint64_t* evals, const uint64_t* point,
                   uint64_t* proof_xy, uint8_t* proof_inf, uint64_t* y);

// A multiproof whose evaluation rows are sparse and already (mostly) on the device -- the verkle
// tree proofs (verkle_proof.hip): the per-point sums S[row(z_i)][k] += r^i f_i[k] are accumulated from the
// rows' non-zeros instead of Q x N dense evaluations. The n_rows distinct rows are given in CSR
// form: row d's non-zeros are [row_ptr[d], row_ptr[d + 1]) of col / src, columns strictly ascending;
// src s means the canonical Fr value d_item[4 s] (s < n_item; device memory) or, with MP_SRC_AUX
// set, aux[4 (s & ~MP_SRC_AUX)] (aux: n_aux host values, uploaded). Query i opens row q_row[i]
// (many queries may share a row). The transcript over all (C, z, y) runs on a helper thread while
// the rows' descriptors and the queries' plan are built and uploaded; then r's powers, the sums,
// and mp_finish (G = 1). The proof equals vc_multiproof_prove's for the same queries with the rows
// written out densely. N must be a multiple of 32.
constexpr uint32_t MP_SRC_AUX = 0x80000000u;
struct MpSparse {
    size_t n_rows = 0;
    const uint32_t* row_ptr = nullptr;  // n_rows + 1
    const uint32_t* col = nullptr;
    const uint32_t* src = nullptr;
    const uint32_t* q_row = nullptr;    // Q
    const uint64_t* d_item = nullptr;   // device, n_item x 4 u64
    size_t n_item = 0;
    const uint64_t* aux = nullptr;  // host, n_aux x 4 u64
    size_t n_aux = 0;
};
int mp_prove_sparse(vc_ctx* ctx, int scheme, int table, size_t N, size_t Q, const uint64_t* com_xy,
                    const uint8_t* com_inf, const uint64_t* z, const uint64_t* y, const MpSparse& sp, uint64_t* d_xy,
                    uint8_t* d_inf, vc_ipa_proof* ipa_proof, uint64_t* kzg_xy, uint8_t* kzg_inf, uint64_t* kzg_y);

}  // namespace vk

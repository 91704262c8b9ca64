// The BLS12-381 entry points behind the curve dispatch of the KZG-verification C ABI, in plain
// types only: the dispatching files (pairing_host.cpp, pairing.hip, kzg_batch.hip) include this and
// not pairing_bls.hpp, so their device code holds no BLS12-381 text.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct vc_ctx;
struct vc_kzg_vk;
struct vc_kzg_vk_bls;

namespace vk {
namespace blsk {
// pairing_bls_host.cpp
int g2_from_secret(const uint64_t* secret_fr, uint64_t* out_g2_xy, uint8_t* out_g2_inf);
int vk_tables_new(const uint64_t* g2_xy, uint8_t g2_inf, size_t size, vc_kzg_vk_bls** out);
void vk_tables_free(vc_kzg_vk_bls* t);
int verify(const vc_kzg_vk* vk, const uint64_t* com_xy, uint8_t com_inf, const uint64_t* point_fr,
           const uint64_t* proof_xy, uint8_t proof_inf, const uint64_t* y_fr, int* result);
int pairing_check(size_t n, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf,
                  int* result);
// pairing_bls.hip
int verify_many(vc_ctx* ctx, const vc_kzg_vk* vk, size_t n, const uint64_t* com_xy, const uint8_t* com_inf,
                const uint64_t* points, const uint64_t* proof_xy, const uint8_t* proof_inf, const uint64_t* y,
                uint8_t* results);
// kzg_batch_bls.hip
int batch_challenge(const uint8_t seed[32], uint64_t* rho_fr);
int batch_fold(vc_ctx* ctx, const vc_kzg_vk* vk, size_t n, const uint64_t* com_xy, const uint8_t* com_inf,
               const uint64_t* points, const uint64_t* proof_xy, const uint8_t* proof_inf, const uint64_t* y,
               const uint64_t* rho_fr, uint64_t* p1_xy, uint8_t* p1_inf, uint64_t* p2_xy, uint8_t* p2_inf,
               int* malformed);
int verify_batch(vc_ctx* ctx, const vc_kzg_vk* vk, size_t n, const uint64_t* com_xy, const uint8_t* com_inf,
                 const uint64_t* points, const uint64_t* proof_xy, const uint8_t* proof_inf, const uint64_t* y,
                 const uint8_t* seed32, int* result, uint8_t* results);
}  // namespace blsk
}  // namespace vk

// Host side of KZG verification (include/vc_scheme.h): the verifying key with its tabulated
// Miller-loop lines, verify_point for one opening, the general pairing-product check. Pure host
// code over csrc/pairing.hpp: no context, no GPU. A BLS12-381 key or curve argument goes to
// pairing_bls_host.cpp (vk::blsk); everything without a curve argument means BN254.
#include <atomic>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vc_scheme.h"
#include "kzg_batch.hpp"
#include "pairing_bls_entry.hpp"
#include "pairing_internal.hpp"

using namespace vk;
using namespace vk::bn;

namespace {

// G2 in the ABI layout (x.c0 x.c1 y.c0 y.c1, canonical) -> Montgomery; false for a coordinate >= p
bool g2_load(const uint64_t* xy, bool inf, G2Aff& out) {
    out = G2Aff{fq2_zero(), fq2_zero(), inf};
    if (inf) return true;
    Fq* dst[4] = {&out.x.c0, &out.x.c1, &out.y.c0, &out.y.c1};
    for (int k = 0; k < 4; k++) {
        uint32_t w[8];
        memcpy(w, xy + 4 * k, 32);
        if (!words_below_modulus<BN254Fq>(w)) return false;
        *dst[k] = canon_to_mont<BN254Fq>(xy + 4 * k);
    }
    return true;
}
void g2_store(const G2Aff& p, uint64_t* xy, uint8_t* inf) {
    memset(xy, 0, 128);
    *inf = p.inf ? 1 : 0;
    if (p.inf) return;
    mont_to_canon<BN254Fq>(p.x.c0, xy);
    mont_to_canon<BN254Fq>(p.x.c1, xy + 4);
    mont_to_canon<BN254Fq>(p.y.c0, xy + 8);
    mont_to_canon<BN254Fq>(p.y.c1, xy + 12);
}
bool fr_words(const uint64_t* fr, uint32_t* w) {  // canonical words; false when >= r
    memcpy(w, fr, 32);
    return words_below_modulus<BN254Fr>(w);
}
bool is_bls(const vc_kzg_vk* vk) { return vk && vk->curve == VC_CURVE_BLS12_381; }

}  // namespace

int vk::kzg_vk_curve(const vc_kzg_vk* vk) { return vk->curve; }

bool vk::kzg_pair_check(const vc_kzg_vk* vk, const G1A& P1, const G1A& P2) {
    return kzgb::pair_check(P1, P2, vk->lines, vk->lines + PC::ATE_LINES);
}

extern "C" {

int vc_kzg_g2_from_secret(const uint64_t* secret_fr, uint64_t* out_g2_xy, uint8_t* out_g2_inf) {
    uint32_t s[8];
    if (!secret_fr || !out_g2_xy || !out_g2_inf || !fr_words(secret_fr, s)) return VC_E_INVALID;
    g2_store(g2_mul(g2_generator(), s, 8), out_g2_xy, out_g2_inf);
    return VC_OK;
}

int vc_kzg_g2_from_secret_curve(int curve, const uint64_t* secret_fr, uint64_t* out_g2_xy, uint8_t* out_g2_inf) {
    if (curve == VC_CURVE_BN254) return vc_kzg_g2_from_secret(secret_fr, out_g2_xy, out_g2_inf);
    if (curve == VC_CURVE_BLS12_381) return blsk::g2_from_secret(secret_fr, out_g2_xy, out_g2_inf);
    return VC_E_INVALID;
}

int vc_kzg_vk_new_curve(int curve, const uint64_t* g2_xy, uint8_t g2_inf, size_t size, vc_kzg_vk** out) {
    if (curve != VC_CURVE_BN254 && curve != VC_CURVE_BLS12_381) return VC_E_INVALID;
    if (!g2_xy || !out || size == 0 || (size & (size - 1)) || size > (size_t(1) << 28)) return VC_E_INVALID;
    G2Aff s2{fq2_zero(), fq2_zero(), true};
    vc_kzg_vk_bls* tables = nullptr;
    if (curve == VC_CURVE_BN254) {
        if (g2_inf || !g2_load(g2_xy, false, s2) || !g2_on_twist(s2) || !g2_in_subgroup(s2)) return VC_E_INVALID;
    } else {
        const int st = blsk::vk_tables_new(g2_xy, g2_inf, size, &tables);
        if (st != VC_OK) return st;
    }
    vc_kzg_vk* vk = new (std::nothrow) vc_kzg_vk();
    if (!vk) {
        blsk::vk_tables_free(tables);
        return VC_E_OOM;
    }
    static std::atomic<uint64_t> next_uid{1};  // one sequence for both curves: the contexts' cache key
    vk->uid = next_uid.fetch_add(1);
    vk->size = size;
    vk->curve = curve;
    vk->bls = tables;
    if (curve == VC_CURVE_BN254) {
        vk->omega = bn254_group_gen(size);
        vk->s2 = s2;
        ate_line_table(s2, vk->lines);
        ate_line_table(g2_generator(), vk->lines + PC::ATE_LINES);
    }
    *out = vk;
    return VC_OK;
}

int vc_kzg_vk_new(const uint64_t* g2_xy, uint8_t g2_inf, size_t size, vc_kzg_vk** out) {
    return vc_kzg_vk_new_curve(VC_CURVE_BN254, g2_xy, g2_inf, size, out);
}

void vc_kzg_vk_free(vc_kzg_vk* vk) {
    if (vk) blsk::vk_tables_free(vk->bls);
    delete vk;
}

int vc_kzg_verify(const vc_kzg_vk* vk, const uint64_t* com_xy, uint8_t com_inf, const uint64_t* point_fr,
                  const uint64_t* proof_xy, uint8_t proof_inf, const uint64_t* y_fr, int* result) {
    if (is_bls(vk)) return blsk::verify(vk, com_xy, com_inf, point_fr, proof_xy, proof_inf, y_fr, result);
    if (!vk || (!com_xy && !com_inf) || !point_fr || (!proof_xy && !proof_inf) || !y_fr || !result) return VC_E_INVALID;
    *result = 0;
    uint32_t y[8], pt[8], w[16];
    if (!fr_words(y_fr, y) || !fr_words(point_fr, pt)) return VC_OK;
    G1P C{fe_zero<BN254Fq>(), fe_zero<BN254Fq>()}, pi = C;
    if (!com_inf) {
        memcpy(w, com_xy, 64);
        if (!g1_load(w, C)) return VC_OK;
    }
    if (!proof_inf) {
        memcpy(w, proof_xy, 64);
        if (!g1_load(w, pi)) return VC_OK;
    }
    uint32_t p[8];
    kzg_eval_point(vk->omega, vk->size, pt, p);
    *result = kzg_check(C, com_inf != 0, pi, proof_inf != 0, y, p, vk->lines, vk->lines + PC::ATE_LINES) ? 1 : 0;
    return VC_OK;
}

int vc_bn254_pairing_check(size_t n, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                           const uint8_t* g2_inf, int* result) {
    if (!result || (n && (!g1_xy || !g1_inf || !g2_xy || !g2_inf)) || n > (size_t(1) << 20)) return VC_E_INVALID;
    std::vector<G1Eval> P(n);
    std::vector<G2Aff> Q(n);
    for (size_t i = 0; i < n; i++) {
        G1P a{fe_zero<BN254Fq>(), fe_zero<BN254Fq>()};
        if (!g1_inf[i]) {
            uint32_t w[16];
            memcpy(w, g1_xy + 8 * i, 64);
            if (!g1_load(w, a)) return VC_E_INVALID;
        }
        P[i] = g1_eval_aff(a.x, a.y, g1_inf[i] != 0);
        if (!g2_load(g2_xy + 16 * i, g2_inf[i] != 0, Q[i]) || !g2_on_twist(Q[i]) || !g2_in_subgroup(Q[i]))
            return VC_E_INVALID;
    }
    *result = pairing_product_is_one((int)n, P.data(), Q.data()) ? 1 : 0;
    return VC_OK;
}

int vc_bls12_381_pairing_check(size_t n, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                               const uint8_t* g2_inf, int* result) {
    return blsk::pairing_check(n, g1_xy, g1_inf, g2_xy, g2_inf, result);
}

}  // extern "C"

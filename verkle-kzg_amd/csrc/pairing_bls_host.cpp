// Host side of KZG verification on BLS12-381 (include/vc_scheme.h): the key's tables, verify_point
// for one opening, the general pairing-product check. Pure host code over csrc/pairing_bls.hpp: no
// context, no GPU. pairing_host.cpp's entry points dispatch here on the curve.
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vc_scheme.h"
#include "host/fr.hpp"
#include "kzg_batch_bls.hpp"
#include "pairing_bls_internal.hpp"
#include "pairing_internal.hpp"

namespace vk {
namespace blsk {

using namespace bls;

namespace {
constexpr int G2W = 4 * NL / 2;  // u64 words of a G2 point: 24

// G2 in the ABI layout (x.c0 x.c1 y.c0 y.c1, canonical) -> Montgomery; false for a coordinate >= p
bool g2_load(const uint64_t* xy, bool inf, G2Aff& out) {
    out = G2Aff{fq2_zero(), fq2_zero(), inf};
    if (inf) return true;
    bls::Fq* dst[4] = {&out.x.c0, &out.x.c1, &out.y.c0, &out.y.c1};
    for (int k = 0; k < 4; k++) {
        uint32_t w[NL];
        memcpy(w, xy + 6 * k, 4 * NL);
        if (!words_below_modulus<BLS381Fq>(w)) return false;
        *dst[k] = canon_to_mont<BLS381Fq>(xy + 6 * k);
    }
    return true;
}
void g2_store(const G2Aff& p, uint64_t* xy, uint8_t* inf) {
    memset(xy, 0, 8 * G2W);
    *inf = p.inf ? 1 : 0;
    if (p.inf) return;
    mont_to_canon<BLS381Fq>(p.x.c0, xy);
    mont_to_canon<BLS381Fq>(p.x.c1, xy + 6);
    mont_to_canon<BLS381Fq>(p.y.c0, xy + 12);
    mont_to_canon<BLS381Fq>(p.y.c1, xy + 18);
}
bool fr_words(const uint64_t* fr, uint32_t* w) {  // canonical words; false when >= r
    memcpy(w, fr, 32);
    return words_below_modulus<BLS381Fr>(w);
}
}  // namespace

bool pair_check(const vc_kzg_vk* vk, const G1A& P1, const G1A& P2) {
    return kzgb_bls::pair_check(P1, P2, vk->bls->lines, vk->bls->lines + PC::ATE_LINES);
}

int g2_from_secret(const uint64_t* secret_fr, uint64_t* out_g2_xy, uint8_t* out_g2_inf) {
    uint32_t s[8];
    if (!secret_fr || !out_g2_xy || !out_g2_inf || !fr_words(secret_fr, s)) return VC_E_INVALID;
    g2_store(g2_mul(g2_generator(), s, 8), out_g2_xy, out_g2_inf);
    return VC_OK;
}

int vk_tables_new(const uint64_t* g2_xy, uint8_t g2_inf, size_t size, vc_kzg_vk_bls** out) {
    G2Aff s2;
    if (g2_inf || !g2_load(g2_xy, false, s2) || !g2_on_twist(s2) || !g2_in_subgroup(s2)) return VC_E_INVALID;
    vc_kzg_vk_bls* t = new (std::nothrow) vc_kzg_vk_bls();
    if (!t) return VC_E_OOM;
    t->omega = group_gen_t<BLS381Fr>(size, fr_generator<BLS381Fr>());
    t->s2 = s2;
    ate_line_table(s2, t->lines);
    ate_line_table(g2_generator(), t->lines + PC::ATE_LINES);
    *out = t;
    return VC_OK;
}
void vk_tables_free(vc_kzg_vk_bls* t) { delete t; }

int verify(const vc_kzg_vk* vk, const uint64_t* com_xy, uint8_t com_inf, const uint64_t* point_fr,
           const uint64_t* proof_xy, uint8_t proof_inf, const uint64_t* y_fr, int* result) {
    if (!vk || !vk->bls || (!com_xy && !com_inf) || !point_fr || (!proof_xy && !proof_inf) || !y_fr || !result)
        return VC_E_INVALID;
    *result = 0;
    uint32_t y[8], pt[8], w[2 * NL];
    if (!fr_words(y_fr, y) || !fr_words(point_fr, pt)) return VC_OK;
    G1P C{fe_zero<BLS381Fq>(), fe_zero<BLS381Fq>()}, pi = C;
    if (!com_inf) {
        memcpy(w, com_xy, sizeof w);
        if (!g1_load(w, C)) return VC_OK;
    }
    if (!proof_inf) {
        memcpy(w, proof_xy, sizeof w);
        if (!g1_load(w, pi)) return VC_OK;
    }
    uint32_t p[8];
    kzg_eval_point(vk->bls->omega, vk->size, pt, p);
    const LineCoef* lines = vk->bls->lines;
    *result = kzg_check(C, com_inf != 0, pi, proof_inf != 0, y, p, lines, lines + PC::ATE_LINES) ? 1 : 0;
    return VC_OK;
}

int pairing_check(size_t n, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf,
                  int* result) {
    if (!result || (n && (!g1_xy || !g1_inf || !g2_xy || !g2_inf)) || n > (size_t(1) << 20)) return VC_E_INVALID;
    std::vector<G1Eval> P(n);
    std::vector<G2Aff> Q(n);
    for (size_t i = 0; i < n; i++) {
        G1P a{fe_zero<BLS381Fq>(), fe_zero<BLS381Fq>()};
        if (!g1_inf[i]) {
            uint32_t w[2 * NL];
            memcpy(w, g1_xy + NL * i, sizeof w);
            if (!g1_load(w, a)) return VC_E_INVALID;
        }
        P[i] = g1_eval_aff(a.x, a.y, g1_inf[i] != 0);
        if (!g2_load(g2_xy + G2W * i, g2_inf[i] != 0, Q[i]) || !g2_on_twist(Q[i]) || !g2_in_subgroup(Q[i]))
            return VC_E_INVALID;
    }
    *result = pairing_product_is_one((int)n, P.data(), Q.data()) ? 1 : 0;
    return VC_OK;
}

}  // namespace blsk
}  // namespace vk

// Host side of KZG verification (include/vc_scheme.h): the verifying key with its tabulated
// Miller-loop lines, verify_point for one opening, the general pairing-product check. Pure host
// code over pairing_common.hpp with pairing.hpp / pairing_bls.hpp: no context, no GPU. One text
// for both curves (C: a curve of kzg_curves.hpp); a key's curve or the curve argument selects the
// instantiation, and everything without a curve argument means BN254.
#include <atomic>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vc_scheme.h"
#include "host/fr.hpp"
#include "pairing_internal.hpp"

using namespace vk;
using namespace vk::ate;

namespace {

template <class Fr>
bool fr_words(const uint64_t* fr, uint32_t* w) {  // canonical words; false when >= r
    memcpy(w, fr, 32);
    return words_below_modulus<Fr>(w);
}

template <class C>
int g2_from_secret(const uint64_t* secret_fr, uint64_t* out_g2_xy, uint8_t* out_g2_inf) {
    uint32_t s[8];
    if (!secret_fr || !out_g2_xy || !out_g2_inf || !fr_words<typename C::Fr>(secret_fr, s)) return VC_E_INVALID;
    g2_store(g2_mul(g2_generator<typename C::Fq>(), s, 8), out_g2_xy, out_g2_inf);
    return VC_OK;
}

// a key of curve C: [s]_2 checked (not the identity, on the twist, of order r), its tables made
template <class C>
int vk_new(const uint64_t* g2_xy, uint8_t g2_inf, size_t size, vc_kzg_vk** out) {
    using Fq = typename C::Fq;
    G2AffT<Fq> s2;
    if (g2_inf || !g2_load(g2_xy, false, s2) || !g2_on_twist(s2) || !g2_in_subgroup(s2)) return VC_E_INVALID;
    KzgKey<C>* key = new (std::nothrow) KzgKey<C>();
    if (!key) return VC_E_OOM;
    key->size = size;
    key->curve = C::CURVE;
    key->omega = group_gen_t<typename C::Fr>(size, fr_generator<typename C::Fr>());
    key->s2 = s2;
    ate_line_table(s2, key->lines);
    ate_line_table(g2_generator<Fq>(), key->lines + C::PC::ATE_LINES);
    *out = key;
    return VC_OK;
}

template <class C>
int verify(const KzgKey<C>& key, const uint64_t* com_xy, uint8_t com_inf, const uint64_t* point_fr,
           const uint64_t* proof_xy, uint8_t proof_inf, const uint64_t* y_fr, int* result) {
    using Fq = typename C::Fq;
    if ((!com_xy && !com_inf) || !point_fr || (!proof_xy && !proof_inf) || !y_fr || !result) return VC_E_INVALID;
    *result = 0;
    uint32_t y[8], pt[8], w[C::PW];
    if (!fr_words<typename C::Fr>(y_fr, y) || !fr_words<typename C::Fr>(point_fr, pt)) return VC_OK;
    SWAff<Fq> Cm{fe_zero<Fq>(), fe_zero<Fq>()}, pi = Cm;
    if (!com_inf) {
        memcpy(w, com_xy, sizeof w);
        if (!g1_load(w, Cm)) return VC_OK;
    }
    if (!proof_inf) {
        memcpy(w, proof_xy, sizeof w);
        if (!g1_load(w, pi)) return VC_OK;
    }
    uint32_t p[8];
    kzg_eval_point(key.omega, key.size, pt, p);
    *result = kzg_check(Cm, com_inf != 0, pi, proof_inf != 0, y, p, key.lines, key.lines + C::PC::ATE_LINES) ? 1 : 0;
    return VC_OK;
}

template <class C>
int pairing_check(size_t n, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf,
                  int* result) {
    using Fq = typename C::Fq;
    if (!result || (n && (!g1_xy || !g1_inf || !g2_xy || !g2_inf)) || n > (size_t(1) << 20)) return VC_E_INVALID;
    std::vector<G1EvalT<Fq>> P(n);
    std::vector<G2AffT<Fq>> Q(n);
    for (size_t i = 0; i < n; i++) {
        SWAff<Fq> a{fe_zero<Fq>(), fe_zero<Fq>()};
        if (!g1_inf[i]) {
            uint32_t w[C::PW];
            memcpy(w, g1_xy + C::PW / 2 * i, sizeof w);
            if (!g1_load(w, a)) return VC_E_INVALID;
        }
        P[i] = g1_eval_aff(a.x, a.y, g1_inf[i] != 0);
        if (!g2_load(g2_xy + C::PW * i, g2_inf[i] != 0, Q[i]) || !g2_on_twist(Q[i]) || !g2_in_subgroup(Q[i]))
            return VC_E_INVALID;
    }
    *result = pairing_product_is_one((int)n, P.data(), Q.data()) ? 1 : 0;
    return VC_OK;
}

}  // namespace

int vk::kzg_vk_curve(const vc_kzg_vk* vk) { return vk->curve; }

extern "C" {

int vc_kzg_g2_from_secret_curve(int curve, const uint64_t* secret_fr, uint64_t* out_g2_xy, uint8_t* out_g2_inf) {
    if (curve == VC_CURVE_BN254) return g2_from_secret<BN254Kzg>(secret_fr, out_g2_xy, out_g2_inf);
    if (curve == VC_CURVE_BLS12_381) return g2_from_secret<BLS381Kzg>(secret_fr, out_g2_xy, out_g2_inf);
    return VC_E_INVALID;
}

int vc_kzg_g2_from_secret(const uint64_t* secret_fr, uint64_t* out_g2_xy, uint8_t* out_g2_inf) {
    return vc_kzg_g2_from_secret_curve(VC_CURVE_BN254, secret_fr, out_g2_xy, out_g2_inf);
}

int vc_kzg_vk_new_curve(int curve, const uint64_t* g2_xy, uint8_t g2_inf, size_t size, vc_kzg_vk** out) {
    if (curve != VC_CURVE_BN254 && curve != VC_CURVE_BLS12_381) return VC_E_INVALID;
    if (!g2_xy || !out || size == 0 || (size & (size - 1)) || size > (size_t(1) << 28)) return VC_E_INVALID;
    vc_kzg_vk* key = nullptr;
    const int st = curve == VC_CURVE_BN254 ? vk_new<BN254Kzg>(g2_xy, g2_inf, size, &key)
                                           : vk_new<BLS381Kzg>(g2_xy, g2_inf, size, &key);
    if (st != VC_OK) return st;
    static std::atomic<uint64_t> next_uid{1};  // one sequence for both curves: the contexts' cache key
    key->uid = next_uid.fetch_add(1);
    *out = key;
    return VC_OK;
}

int vc_kzg_vk_new(const uint64_t* g2_xy, uint8_t g2_inf, size_t size, vc_kzg_vk** out) {
    return vc_kzg_vk_new_curve(VC_CURVE_BN254, g2_xy, g2_inf, size, out);
}

void vc_kzg_vk_free(vc_kzg_vk* vk) {  // as what it was allocated as
    if (!vk) return;
    if (vk->curve == VC_CURVE_BLS12_381) delete static_cast<KzgKey<BLS381Kzg>*>(vk);
    else delete static_cast<KzgKey<BN254Kzg>*>(vk);
}

int vc_kzg_verify(const vc_kzg_vk* vk, const uint64_t* com_xy, uint8_t com_inf, const uint64_t* point_fr,
                  const uint64_t* proof_xy, uint8_t proof_inf, const uint64_t* y_fr, int* result) {
    if (!vk) return VC_E_INVALID;
    if (vk->curve == VC_CURVE_BLS12_381)
        return verify(kzg_key<BLS381Kzg>(vk), com_xy, com_inf, point_fr, proof_xy, proof_inf, y_fr, result);
    return verify(kzg_key<BN254Kzg>(vk), com_xy, com_inf, point_fr, proof_xy, proof_inf, y_fr, result);
}

int vc_bn254_pairing_check(size_t n, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                           const uint8_t* g2_inf, int* result) {
    return pairing_check<BN254Kzg>(n, g1_xy, g1_inf, g2_xy, g2_inf, result);
}

int vc_bls12_381_pairing_check(size_t n, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                               const uint8_t* g2_inf, int* result) {
    return pairing_check<BLS381Kzg>(n, g1_xy, g1_inf, g2_xy, g2_inf, result);
}

}  // extern "C"

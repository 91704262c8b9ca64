// Host side of KZG subvector proofs (include/vc_scheme.h): the weights c_i, the verifying key with
// the powers [s^t]_1 and [s^t]_2, the verifier, and the powers from a secret for tests and trusted
// setups. Pure host code over pairing_common.hpp with pairing.hpp / pairing_bls.hpp: no context, no
// GPU. One text for both curves (C: a curve of kzg_curves.hpp).
//
// The verifier of e(pi, [Z_S(s)]_2) == e(C - [I(s)]_1, H) forms the monomial coefficients of Z_S and
// I on the host (O(k^2) field multiplies) and the two points A = sum z_t [s^t]_2 and -B = sum I_t
// [s^t]_1 - C by joint double-and-add: one doubling chain of 256 steps for all k + 1 (or k) terms,
// G2 in Jacobian coordinates over Fq2 and G1 in XYZZ, so one Fq2 inversion (A to affine, for the
// Miller loop's affine lines) per verdict instead of pairing_common.hpp's g2_mul's one per step.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vc_scheme.h"
#include "host/fr.hpp"
#include "pairing_internal.hpp"

using namespace vk;
using namespace vk::ate;

namespace {

// ---------------------------------------------------------------- G2, Jacobian over Fq2 (a = 0)
template <class F>
struct G2Jac {
    Fq2T<F> X, Y, Z;  // Z = 0: the identity
};
template <class F>
G2Jac<F> g2j_zero() {
    return G2Jac<F>{fq2_one<F>(), fq2_one<F>(), fq2_zero<F>()};
}
template <class F>
G2Jac<F> g2j_dbl(const G2Jac<F>& p) {  // dbl-2009-l
    if (fq2_is_zero(p.Z)) return p;
    const Fq2T<F> A = fq2_sqr(p.X), B = fq2_sqr(p.Y), C = fq2_sqr(B);
    const Fq2T<F> D = fq2_dbl(fq2_sub(fq2_sub(fq2_sqr(fq2_add(p.X, B)), A), C));
    const Fq2T<F> E = fq2_add(fq2_dbl(A), A), Fv = fq2_sqr(E);
    G2Jac<F> r;
    r.X = fq2_sub(Fv, fq2_dbl(D));
    r.Y = fq2_sub(fq2_mul(E, fq2_sub(D, r.X)), fq2_dbl(fq2_dbl(fq2_dbl(C))));
    r.Z = fq2_dbl(fq2_mul(p.Y, p.Z));
    return r;
}
template <class F>
G2Jac<F> g2j_madd(const G2Jac<F>& p, const G2AffT<F>& q) {  // madd-2007-bl; q not the identity
    if (fq2_is_zero(p.Z)) return G2Jac<F>{q.x, q.y, fq2_one<F>()};
    const Fq2T<F> Z1Z1 = fq2_sqr(p.Z), U2 = fq2_mul(q.x, Z1Z1), S2 = fq2_mul(fq2_mul(q.y, p.Z), Z1Z1);
    const Fq2T<F> H = fq2_sub(U2, p.X), rr = fq2_dbl(fq2_sub(S2, p.Y));
    if (fq2_is_zero(H)) {
        if (fq2_is_zero(rr)) return g2j_dbl(G2Jac<F>{q.x, q.y, fq2_one<F>()});
        return g2j_zero<F>();
    }
    const Fq2T<F> HH = fq2_sqr(H), I = fq2_dbl(fq2_dbl(HH)), J = fq2_mul(H, I), V = fq2_mul(p.X, I);
    G2Jac<F> r;
    r.X = fq2_sub(fq2_sub(fq2_sqr(rr), J), fq2_dbl(V));
    r.Y = fq2_sub(fq2_mul(rr, fq2_sub(V, r.X)), fq2_dbl(fq2_mul(p.Y, J)));
    r.Z = fq2_sub(fq2_sub(fq2_sqr(fq2_add(p.Z, H)), Z1Z1), HH);
    return r;
}
template <class F>
G2AffT<F> g2j_affine(const G2Jac<F>& p) {
    if (fq2_is_zero(p.Z)) return G2AffT<F>{fq2_zero<F>(), fq2_zero<F>(), true};
    const Fq2T<F> zi = fq2_inv(p.Z), zi2 = fq2_sqr(zi);
    return G2AffT<F>{fq2_mul(p.X, zi2), fq2_mul(p.Y, fq2_mul(zi2, zi)), false};
}
// sum_t k_t Q_t, the k_t as 8 canonical words each, by one doubling chain
template <class F>
G2Jac<F> g2j_msm(const G2AffT<F>* Q, const uint32_t* k, size_t n) {
    G2Jac<F> r = g2j_zero<F>();
    for (int i = 7; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            r = g2j_dbl(r);
            for (size_t t = 0; t < n; t++)
                if ((k[8 * t + i] >> b) & 1) r = g2j_madd(r, Q[t]);
        }
    return r;
}
template <class F>
bool g2j_in_subgroup(const G2AffT<F>& q) {  // [r] Q == O
    using Fr = typename KzgCurve<F>::Fr;
    uint32_t r[8];
    for (int i = 0; i < 8; i++) r[i] = Fr::p(i);
    return fq2_is_zero(g2j_msm(&q, r, 1).Z);
}
// the same for G1 in XYZZ (pairing_common.hpp's g1_dbl / g1_madd)
template <class F>
SWAcc<F> g1_msm(const SWAff<F>* P, const uint32_t* k, size_t n) {
    SWAcc<F> r = KzgCurve<F>::G1::zero();
    for (int i = 7; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            r = g1_dbl(r);
            for (size_t t = 0; t < n; t++)
                if ((k[8 * t + i] >> b) & 1) r = g1_madd(r, P[t], false);
        }
    return r;
}

// ---------------------------------------------------------------- layouts
template <class F>
void g1_store(const SWAcc<F>& p, uint64_t* xy) {  // p not the identity
    const fe<F> izzz = fq_inv(p.zzz), t = fq_mul(izzz, p.zz), izz = fq_mul(t, t);
    mont_to_canon<F>(fq_mul(p.x, izz), xy);
    mont_to_canon<F>(fq_mul(p.y, izzz), xy + F::N / 2);
}
template <class Fr>
void fr_canon_words(const fe<Fr>& a, uint32_t* w) {
    const fe<Fr> c = fe_from_mont<Fr>(a);
    for (int i = 0; i < 8; i++) w[i] = c.v[i];
}

// ---------------------------------------------------------------- the index set
inline bool size_ok(size_t size) { return size >= 2 && !(size & (size - 1)) && size <= (size_t(1) << 28); }
// k >= 1 distinct indices below size
bool index_set_ok(const uint32_t* idx, size_t k, size_t size) {
    if (!idx || k == 0 || k > size) return false;
    std::vector<uint32_t> s(idx, idx + k);
    std::sort(s.begin(), s.end());
    if (s.back() >= size) return false;
    return std::adjacent_find(s.begin(), s.end()) == s.end();
}
template <class C>
int weights(size_t N, const uint32_t* idx, size_t k, uint64_t* c_out) {
    using Fr = typename C::Fr;
    std::vector<fe<Fr>> x, c;
    sub_weights<Fr>(group_gen_t<Fr>(N, fr_generator<Fr>()), idx, k, x, c);
    for (size_t i = 0; i < k; i++) mont_to_canon<Fr>(c[i], c_out + 4 * i);
    return VC_OK;
}

template <class C>
int powers_from_secret(const uint64_t* secret_fr, size_t K, uint64_t* g1_out, uint64_t* g2_out) {
    using Fq = typename C::Fq;
    using Fr = typename C::Fr;
    uint32_t w[8];
    memcpy(w, secret_fr, 32);
    if (!words_below_modulus<Fr>(w)) return VC_E_INVALID;
    const fe<Fr> s = canon_to_mont<Fr>(secret_fr);
    if (fe_is_zero<Fr>(s)) return VC_E_INVALID;  // [0]_1 is the identity: no coordinates
    const SWAff<Fq> G = C::g1_generator();
    const G2AffT<Fq> H = g2_generator<Fq>();
    fe<Fr> p = fe_one<Fr>();
    for (size_t t = 0; t <= K; t++) {
        fr_canon_words<Fr>(p, w);
        if (t < K) g1_store<Fq>(g1_msm<Fq>(&G, w, 1), g1_out + C::PW / 2 * t);
        uint8_t inf;  // never set: s^t is not zero
        g2_store<Fq>(g2j_affine(g2j_msm<Fq>(&H, w, 1)), g2_out + C::PW * t, &inf);
        p = fe_mul<Fr>(p, s);
    }
    return VC_OK;
}

template <class C>
int svk_new(size_t size, size_t K, const uint64_t* g1_powers, const uint64_t* g2_powers, vc_kzg_svk** out) {
    using Fq = typename C::Fq;
    SubKey<C>* key = new (std::nothrow) SubKey<C>();
    if (!key) return VC_E_OOM;
    key->size = size;
    key->K = K;
    key->curve = C::CURVE;
    key->omega = group_gen_t<typename C::Fr>(size, fr_generator<typename C::Fr>());
    key->g1.resize(K);
    key->g2.resize(K + 1);
    bool ok = true;
    for (size_t t = 0; t < K && ok; t++) {  // on the curve and, with a cofactor, in the subgroup
        uint32_t w[C::PW];
        memcpy(w, g1_powers + C::PW / 2 * t, sizeof w);
        ok = g1_load(w, key->g1[t]);
    }
    for (size_t t = 0; t <= K && ok; t++)
        ok = g2_load(g2_powers + C::PW * t, false, key->g2[t]) && g2_on_twist(key->g2[t]) && g2j_in_subgroup(key->g2[t]);
    if (ok) {
        const SWAff<Fq> G = C::g1_generator();
        const G2AffT<Fq> H = g2_generator<Fq>();
        ok = fe_eq<Fq>(key->g1[0].x, G.x) && fe_eq<Fq>(key->g1[0].y, G.y) && fq2_eq(key->g2[0].x, H.x) &&
             fq2_eq(key->g2[0].y, H.y);
    }
    if (!ok) {
        delete key;
        return VC_E_INVALID;
    }
    *out = key;
    return VC_OK;
}

template <class C>
int verify(const SubKey<C>& key, const uint64_t* com_xy, uint8_t com_inf, const uint32_t* idx, size_t k,
           const uint64_t* y, const uint64_t* proof_xy, uint8_t proof_inf, int* result) {
    using Fq = typename C::Fq;
    using Fr = typename C::Fr;
    if ((!com_xy && !com_inf) || !y || (!proof_xy && !proof_inf) || !result) return VC_E_INVALID;
    if (!index_set_ok(idx, k, key.size)) return VC_E_INVALID;
    if (k > key.K) return VC_E_RANGE;
    *result = 0;
    // ---- malformed content: verdict 0
    uint32_t w[C::PW];
    std::vector<fe<Fr>> yv(k);
    for (size_t i = 0; i < k; i++) {
        uint32_t yw[8];
        memcpy(yw, y + 4 * i, 32);
        if (!words_below_modulus<Fr>(yw)) return VC_OK;
        yv[i] = canon_to_mont<Fr>(y + 4 * i);
    }
    SWAff<Fq> Cm{fe_zero<Fq>(), fe_zero<Fq>()}, pi = Cm;
    if (!com_inf) {
        memcpy(w, com_xy, sizeof w);
        if (!g1_load(w, Cm)) return VC_OK;
    }
    if (!proof_inf) {
        memcpy(w, proof_xy, sizeof w);
        if (!g1_load(w, pi)) return VC_OK;
    }
    // ---- Z_S and I in the monomial basis
    std::vector<fe<Fr>> x, c;
    sub_weights<Fr>(key.omega, idx, k, x, c);
    std::vector<fe<Fr>> z(k + 1, fe_zero<Fr>()), I(k, fe_zero<Fr>()), b(k);
    z[0] = fe_one<Fr>();
    for (size_t i = 0; i < k; i++)  // z <- z (X - x_i)
        for (size_t t = i + 1;; t--) {
            const fe<Fr> lower = t ? z[t - 1] : fe_zero<Fr>();
            z[t] = fe_sub<Fr>(lower, fe_mul<Fr>(x[i], z[t]));
            if (!t) break;
        }
    for (size_t i = 0; i < k; i++) {  // I += y_i c_i Z_S / (X - x_i), the quotient by synthetic division
        const fe<Fr> yc = fe_mul<Fr>(yv[i], c[i]);
        b[k - 1] = z[k];
        for (size_t t = k - 1; t > 0; t--) b[t - 1] = fe_add<Fr>(z[t], fe_mul<Fr>(x[i], b[t]));
        for (size_t t = 0; t < k; t++) I[t] = fe_add<Fr>(I[t], fe_mul<Fr>(yc, b[t]));
    }
    // ---- A = [Z_S(s)]_2, -B = [I(s)]_1 - C
    std::vector<uint32_t> zw(8 * (k + 1)), iw(8 * k);
    for (size_t t = 0; t <= k; t++) fr_canon_words<Fr>(z[t], &zw[8 * t]);
    for (size_t t = 0; t < k; t++) fr_canon_words<Fr>(I[t], &iw[8 * t]);
    const G2AffT<Fq> A = g2j_affine(g2j_msm<Fq>(key.g2.data(), zw.data(), k + 1));
    SWAcc<Fq> nB = g1_msm<Fq>(key.g1.data(), iw.data(), k);
    if (!com_inf) nB = g1_madd(nB, Cm, true);
    // ---- e(pi, A) e(-B, H) == 1
    const G1EvalT<Fq> P[2] = {g1_eval_aff(pi.x, pi.y, proof_inf != 0), g1_eval_acc(nB)};
    const G2AffT<Fq> Q[2] = {A, g2_generator<Fq>()};
    *result = pairing_product_is_one(2, P, Q) ? 1 : 0;
    return VC_OK;
}

}  // namespace

extern "C" {

int vc_kzg_subvector_weights(int curve, size_t N, const uint32_t* idx, size_t k, uint64_t* c_out) {
    if ((curve != VC_CURVE_BN254 && curve != VC_CURVE_BLS12_381) || !size_ok(N) || !c_out) return VC_E_INVALID;
    if (!index_set_ok(idx, k, N)) return VC_E_INVALID;
    return curve == VC_CURVE_BN254 ? weights<BN254Kzg>(N, idx, k, c_out) : weights<BLS381Kzg>(N, idx, k, c_out);
}

int vc_kzg_powers_from_secret(int curve, const uint64_t* secret_fr, size_t K, uint64_t* g1_out, uint64_t* g2_out) {
    if (!secret_fr || !g1_out || !g2_out || K == 0 || K > (size_t(1) << 28)) return VC_E_INVALID;
    if (curve == VC_CURVE_BN254) return powers_from_secret<BN254Kzg>(secret_fr, K, g1_out, g2_out);
    if (curve == VC_CURVE_BLS12_381) return powers_from_secret<BLS381Kzg>(secret_fr, K, g1_out, g2_out);
    return VC_E_INVALID;
}

int vc_kzg_svk_new(int curve, size_t size, size_t K, const uint64_t* g1_powers, const uint64_t* g2_powers,
                   vc_kzg_svk** svk) {
    if (curve != VC_CURVE_BN254 && curve != VC_CURVE_BLS12_381) return VC_E_INVALID;
    if (!size_ok(size) || K == 0 || K > size || !g1_powers || !g2_powers || !svk) return VC_E_INVALID;
    return curve == VC_CURVE_BN254 ? svk_new<BN254Kzg>(size, K, g1_powers, g2_powers, svk)
                                   : svk_new<BLS381Kzg>(size, K, g1_powers, g2_powers, svk);
}

void vc_kzg_svk_free(vc_kzg_svk* svk) {  // as what it was allocated as
    if (!svk) return;
    if (svk->curve == VC_CURVE_BLS12_381) delete static_cast<SubKey<BLS381Kzg>*>(svk);
    else delete static_cast<SubKey<BN254Kzg>*>(svk);
}

int vc_kzg_verify_subvector(const vc_kzg_svk* svk, const uint64_t* com_xy, uint8_t com_inf, const uint32_t* idx,
                            size_t k, const uint64_t* y, const uint64_t* proof_xy, uint8_t proof_inf, int* result) {
    if (!svk) return VC_E_INVALID;
    if (svk->curve == VC_CURVE_BLS12_381)
        return verify(sub_key<BLS381Kzg>(svk), com_xy, com_inf, idx, k, y, proof_xy, proof_inf, result);
    return verify(sub_key<BN254Kzg>(svk), com_xy, com_inf, idx, k, y, proof_xy, proof_inf, result);
}

}  // extern "C"

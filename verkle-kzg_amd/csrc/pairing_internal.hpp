// The KZG verifying key shared by the host verifier (pairing_host.cpp), the batched device
// verifier (pairing.hip) and the batch fold (kzg_batch.hip): what every key has, and behind it the
// tables of the key's own curve (vk::KzgKey<C>, C a curve of kzg_curves.hpp). The C ABI hands out
// vc_kzg_vk*; an entry point looks at `curve` and goes on with kzg_key<C>.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string.h>

#include <memory>
#include <mutex>
#include <vector>

#include "host/fr.hpp"
#include "pairing.hpp"
#include "pairing_bls.hpp"

struct vc_kzg_vk {
    uint64_t uid = 0;  // unique per key ever made, one sequence for all curves (a freed key's address
                       // can come back): the contexts key their uploaded copies of the tables on it
    size_t size = 0;   // the domain
    int curve = 0;     // VC_CURVE_BN254 or VC_CURVE_BLS12_381
};

namespace vk {
template <class C>
struct KzgKey : vc_kzg_vk {
    fe<typename C::Fr> omega;         // the domain's generator (Montgomery)
    ate::G2AffT<typename C::Fq> s2;  // [s]_2
    // Miller-loop lines of [s]_2, then of H
    ate::LineCoefT<typename C::Fq> lines[2 * C::PC::ATE_LINES];
};
// a key of curve C::CURVE as what it was allocated as
template <class C>
inline const KzgKey<C>& kzg_key(const vc_kzg_vk* vk) {
    return *static_cast<const KzgKey<C>*>(vk);
}
int kzg_vk_curve(const vc_kzg_vk* vk);

// G2 in the ABI layout (x.c0 x.c1 y.c0 y.c1, canonical) -> Montgomery; false for a coordinate >= p
// (the host entry points: pairing_host.cpp, kzg_sub_host.cpp)
template <class F>
inline bool g2_load(const uint64_t* xy, bool inf, ate::G2AffT<F>& out) {
    constexpr int NW = F::N / 2;  // u64 words of a coordinate
    out = ate::G2AffT<F>{ate::fq2_zero<F>(), ate::fq2_zero<F>(), inf};
    if (inf) return true;
    fe<F>* dst[4] = {&out.x.c0, &out.x.c1, &out.y.c0, &out.y.c1};
    for (int k = 0; k < 4; k++) {
        uint32_t w[F::N];
        memcpy(w, xy + NW * k, sizeof w);
        if (!ate::words_below_modulus<F>(w)) return false;
        *dst[k] = canon_to_mont<F>(xy + NW * k);
    }
    return true;
}
template <class F>
inline void g2_store(const ate::G2AffT<F>& p, uint64_t* xy, uint8_t* inf) {
    constexpr int NW = F::N / 2;
    memset(xy, 0, 8 * 4 * NW);
    *inf = p.inf ? 1 : 0;
    if (p.inf) return;
    mont_to_canon<F>(p.x.c0, xy);
    mont_to_canon<F>(p.x.c1, xy + NW);
    mont_to_canon<F>(p.y.c0, xy + 2 * NW);
    mont_to_canon<F>(p.y.c1, xy + 3 * NW);
}
}  // namespace vk

// The key of subvector proofs (kzg_sub_host.cpp makes and frees it; kzg_subv.hip reads it too).
struct vc_kzg_svk {
    size_t size = 0;  // the domain
    size_t K = 0;     // g1: K powers, g2: K + 1
    int curve = 0;
};

namespace vk {
template <class C>
struct SubKey : vc_kzg_svk {
    fe<typename C::Fr> omega;  // the domain's generator (Montgomery)
    std::vector<SWAff<typename C::Fq>> g1;
    std::vector<ate::G2AffT<typename C::Fq>> g2;
    // Miller-loop lines of [s^t]_2 for the batch verifier alone: lines[t] is the table of [s^t]_2
    // (t = 0: H), ATE_LINES entries. Made on first use and grown under the lock, each table an
    // allocation of its own that never moves: a caller copies the pointers it needs while it holds
    // the lock. vc_kzg_svk_new makes none of them.
    mutable std::mutex lines_mu;
    mutable std::vector<std::unique_ptr<ate::LineCoefT<typename C::Fq>[]>> lines;
};
// x_i = w^idx[i] and c_i = 1 / prod_{l != i} (x_i - x_l), one inversion for all (Montgomery):
// the single verifier and the batch fold's host path
template <class Fr>
inline void sub_weights(const fe<Fr>& omega, const uint32_t* idx, size_t k, std::vector<fe<Fr>>& x,
                        std::vector<fe<Fr>>& c) {
    x.resize(k);
    c.resize(k);
    for (size_t i = 0; i < k; i++) x[i] = fe_pow_u64<Fr>(omega, idx[i]);
    std::vector<fe<Fr>> pre(k);
    fe<Fr> run = fe_one<Fr>();
    for (size_t i = 0; i < k; i++) {
        fe<Fr> d = fe_one<Fr>();
        for (size_t l = 0; l < k; l++)
            if (l != i) d = fe_mul<Fr>(d, fe_sub<Fr>(x[i], x[l]));
        c[i] = d;
        pre[i] = run;
        run = fe_mul<Fr>(run, d);
    }
    fe<Fr> inv = fe_inv_bin<Fr>(run);
    for (size_t i = k; i-- > 0;) {
        const fe<Fr> d = c[i];
        c[i] = fe_mul<Fr>(inv, pre[i]);
        inv = fe_mul<Fr>(inv, d);
    }
}
template <class C>
inline const SubKey<C>& sub_key(const vc_kzg_svk* k) {
    return *static_cast<const SubKey<C>*>(k);
}
}  // namespace vk

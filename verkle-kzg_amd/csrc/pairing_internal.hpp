// The KZG verifying key shared by the host verifier (pairing_host.cpp), the batched device
// verifier (pairing.hip) and the batch fold (kzg_batch.hip): what every key has, and behind it the
// tables of the key's own curve (vk::KzgKey<C>, C a curve of kzg_curves.hpp). The C ABI hands out
// vc_kzg_vk*; an entry point looks at `curve` and goes on with kzg_key<C>.
#pragma once
#include <stddef.h>
#include <stdint.h>

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
}  // namespace vk

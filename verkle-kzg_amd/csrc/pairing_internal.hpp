// The KZG verifying key shared by the host verifier (pairing_host.cpp) and the batched device
// verifier (pairing.hip). A BLS12-381 key keeps its own tables (pairing_bls_internal.hpp) behind
// `bls`; the BN254 members are then unused.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "host/fr.hpp"
#include "pairing.hpp"

struct vc_kzg_vk_bls;

struct vc_kzg_vk {
    uint64_t uid = 0;  // unique per key ever made (a freed key's address can come back): the
                       // contexts key their uploaded copies of the tables on it
    size_t size = 0;   // the domain
    vk::Fr omega;      // its generator (Montgomery)
    vk::bn::G2Aff s2;  // [s]_2
    // Miller-loop lines of [s]_2, then of H
    vk::bn::LineCoef lines[2 * vk::bn::PC::ATE_LINES];
    int curve = 0;                 // VC_CURVE_BN254 or VC_CURVE_BLS12_381
    vc_kzg_vk_bls* bls = nullptr;  // the BLS12-381 key's tables (owned; vc_kzg_vk_free)
};

namespace vk {
// e(P1, [s]_2) e(P2, H) == 1 over the key's tables for two points of G1 as accumulators, the
// identity included (pairing_host.cpp; the batch verifier's final check: vc_kzg_verify's inputs
// cannot express it)
bool kzg_pair_check(const vc_kzg_vk* vk, const bn::G1A& P1, const bn::G1A& P2);
int kzg_vk_curve(const vc_kzg_vk* vk);
}  // namespace vk

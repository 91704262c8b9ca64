// The BLS12-381 half of the KZG verifying key (pairing_internal.hpp's vc_kzg_vk::bls), shared by
// the host verifier (pairing_bls_host.cpp), the batched device verifier (pairing_bls.hip) and the
// batch fold (kzg_batch_bls.hip); their entry points are declared in pairing_bls_entry.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pairing_bls.hpp"
#include "pairing_bls_entry.hpp"

struct vc_kzg_vk_bls {
    vk::bls::FrE omega;  // the domain's generator 7^((r - 1) / size) (Montgomery)
    vk::bls::G2Aff s2;   // [s]_2
    // Miller-loop lines of [s]_2, then of H
    vk::bls::LineCoef lines[2 * vk::bls::PC::ATE_LINES];
};

namespace vk {
namespace blsk {
// e(P1, [s]_2) e(P2, H) == 1 over the key's tables, the identity included (pairing_bls_host.cpp)
bool pair_check(const vc_kzg_vk* vk, const bls::G1A& P1, const bls::G1A& P2);
}  // namespace blsk
}  // namespace vk

// The two pairing curves of KZG verification, each described once. Everything above the field
// engine that is the same for both -- the tower, the G2 law, the opening check
// (pairing_common.hpp), the batch fold (kzg_batch.hpp), the kernels and their drivers
// (pairing.hip, kzg_batch.hip) and the host entry points (pairing_host.cpp) -- is one text over
// one of these types; pairing.hpp and pairing_bls.hpp hold only what a curve does differently.
//
// Inlining policy on the device (OOL_ADDS). Every multiply and square of the tower is an
// out-of-line function (VK_PFN) on both curves: the reason is code size, and one copy of each tower
// function per kernel. The additions differ. On BN254 (8 limbs) fq_add / fq_sub, and the Fq2 and
// Fq6 sums built from them, are inline, and fq_neg is fe_neg. On BLS12-381 (12 limbs) the same
// six functions are out of line as well and fq_neg goes through fq_sub: BN254's code object is
// 2.5 times the BLS12-381 one because its add / subtract chains are inlined into every tower
// function, and the 12-limb chains would be half as long again. Each curve keeps the choice its
// kernels were shaped and measured with; pairing_common.hpp reads the flag.
#pragma once
#include "../../include/vc_msm.h"
#include "ec.hpp"
#include "pairing_bls_consts.hpp"
#include "pairing_consts.hpp"

namespace vk {

struct BN254Kzg {
    using Fq = BN254Fq;
    using Fr = BN254Fr;
    using G1 = BN254G1;  // y^2 = x^3 + 3, cofactor 1: on the curve is in the group
    using PC = BN254Pairing;
    static constexpr int CURVE = VC_CURVE_BN254;
    static constexpr int PW = G1::AFF_WORDS;   // 32-bit words of a G1 point in the ABI: 16
    static constexpr bool OOL_ADDS = false;
    static constexpr bool G1_COFACTOR = false;
    static constexpr bool X_NEGATIVE = false;
    static constexpr const char* VERIFY_LAUNCH = "kzg_verify";
    static constexpr const char* PREP_LAUNCH = "kzg_batch_prep";
    VK_HD static SWAff<Fq> g1_generator() {  // (1, 2)
        const fe<Fq> one = fe_one<Fq>();
        return SWAff<Fq>{one, fe_add<Fq>(one, one)};
    }
};

struct BLS381Kzg {
    using Fq = BLS381Fq;
    using Fr = BLS381Fr;
    using G1 = BLS381G1;  // y^2 = x^3 + 4, with a cofactor: g1_load tests the subgroup
    using PC = BLS381Pairing;
    static constexpr int CURVE = VC_CURVE_BLS12_381;
    static constexpr int PW = G1::AFF_WORDS;   // 24
    static constexpr bool OOL_ADDS = true;
    static constexpr bool G1_COFACTOR = true;
    static constexpr bool X_NEGATIVE = true;  // the Miller loop runs over |x|: one conjugation after it
    static constexpr const char* VERIFY_LAUNCH = "kzg_verify_bls";
    static constexpr const char* PREP_LAUNCH = "kzg_bls_batch_prep";
    VK_HD static SWAff<Fq> g1_generator() {
        SWAff<Fq> g;
        for (int j = 0; j < Fq::N; j++) {
            g.x.v[j] = PC::g1c(0, j);
            g.y.v[j] = PC::g1c(1, j);
        }
        return g;
    }
};

// the description of the curve with base field F
template <class F>
struct KzgCurveOf;
template <>
struct KzgCurveOf<BN254Fq> {
    using type = BN254Kzg;
};
template <>
struct KzgCurveOf<BLS381Fq> {
    using type = BLS381Kzg;
};
template <class F>
using KzgCurve = typename KzgCurveOf<F>::type;

}  // namespace vk

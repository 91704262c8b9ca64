// The point of a KZG opening (KZG::prove_point, kzg/mod.rs:136-154), host + gfx950 device from one
// source: its class (in the domain at m / at N / outside), the vanishing value z^N - 1, and the
// status every opening call decides on the host before any GPU work. The single open
// (kzg_open.hip) and the batch (kzg_many.hip) share this text, so they reject the same points.
#pragma once
#include "ff.hpp"
#include "../../include/vc_msm.h"

namespace vk {
namespace kzgm {

constexpr uint32_t KM_OUTSIDE = 0xffffffffu;  // the point is not below or at N: the barycentric branch
constexpr uint32_t KM_AT_N = 0xfffffffeu;     // the point equals N: the reference panics (Appendix B.4)

template <class F>
VK_HD fe<F> words_load(const uint32_t* w) {  // the words as they are (no conversion)
    fe<F> r;
    for (int i = 0; i < F::N; i++) r.v[i] = w[i];
    return r;
}
// canonical words below the modulus
template <class F>
VK_HD bool words_canonical(const uint32_t* w) {
    for (int i = F::N - 1; i >= 0; i--)
        if (w[i] != F::p(i)) return w[i] < F::p(i);
    return false;
}

// prove_point's branch: the canonical point as an integer. m < N: in the domain at m.
template <class F>
VK_HD uint32_t classify(const uint32_t* z, uint32_t N) {
    uint32_t hi = 0;
    for (int k = 1; k < F::N; k++) hi |= z[k];
    if (hi != 0 || z[0] > N) return KM_OUTSIDE;
    return z[0] == N ? KM_AT_N : z[0];
}

// D = z^N - 1, N = 2^lgN (Montgomery in and out). Zero exactly for the domain's elements.
template <class F>
VK_HD fe<F> vanishing(const fe<F>& z, int lgN) {
    fe<F> p = z;
    for (int k = 0; k < lgN; k++) p = fe_sqr<F>(p);
    return fe_sub<F>(p, fe_one<F>());
}

// The status of an opening at the point z (F::N canonical words as the caller gave them) over the
// domain of N = 2^lgN < 2^31 elements, *cls its class when VC_OK:
//   VC_E_INVALID  z >= r;
//   VC_E_DOMAIN   z == N (vanishing_at(size) is out of bounds in the reference, Appendix B.4), or z is
//                 a domain element that is not below N (z^N == 1: the reference divides by zero,
//                 precompute.rs:86 -- r - 1 = w^(N / 2) is one for every N >= 2).
template <class F>
inline int point_status(const uint32_t* z, uint32_t N, int lgN, uint32_t* cls) {
    if (!words_canonical<F>(z)) return VC_E_INVALID;
    const uint32_t c = classify<F>(z, N);
    if (c == KM_AT_N) return VC_E_DOMAIN;
    if (c == KM_OUTSIDE && fe_is_zero<F>(vanishing<F>(fe_to_mont<F>(words_load<F>(z)), lgN))) return VC_E_DOMAIN;
    *cls = c;
    return VC_OK;
}

}  // namespace kzgm
}  // namespace vk

// What scheme.hip, ipa.hip, kzg_open.hip and multiproof.hip share and nobody else sees: the BN254
// aliases and the one-line conversions (scheme_internal.hpp declares the functions that cross files).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "ctx.hpp"
#include "ec.hpp"
#include "scheme_internal.hpp"
#include "host/pool.hpp"

namespace vk {

using F = BN254Fr;
using C = BN254G1;
using Acc = C::Acc;

inline Fr fr_of(const uint64_t* w) { return canon_to_mont<F>(w); }
inline void canon_of(const Fr& a, uint64_t* w) { mont_to_canon<F>(a, w); }
inline Fr fr_u64(uint64_t v) { return mont_from_u64<F>(v); }
inline bool is_pow2(size_t n) { return n && !(n & (n - 1)); }
inline bool proof_ok(const vc_ipa_proof* p) { return p && p->l_xy && p->r_xy && p->l_inf && p->r_inf; }

}  // namespace vk

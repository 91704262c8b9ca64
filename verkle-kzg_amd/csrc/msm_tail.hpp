// Launchers of the latency-bound Pippenger tail kernels (msm_tail.hip); the bit stage's geometry
// (msm_tail_plan) is in msm_plan.hpp.
#pragma once
#include "ctx.hpp"
#include "ec.hpp"
#include "ec29.hpp"
#include "msm_plan.hpp"

namespace vk {
// the fix-up by pointer jumping: reads the longest chain back (host sync) and runs exactly the
// rounds it needs
// raw radix-29 accumulator of curve C (what k_msm_accumulate writes)
template <class C>
using FAcc = typename Fast29<C>::type::Acc;
template <class C>
int msm_tail_fixup(vc_ctx* ctx, Lane L, uint32_t T, const uint32_t* Lp, uint32_t M, FAcc<C>* buckets, FAcc<C>* carry,
                   const uint8_t* through, const FAcc<C>* owner, const uint32_t* owner_b,
                   const uint32_t* d_chain_max);
template <class C>
int msm_tail_fixup_walk(vc_ctx* ctx, Lane L, const uint32_t* offsets, uint32_t NBtot, uint32_t M, FAcc<C>* buckets,
                        const FAcc<C>* carry, const FAcc<C>* owner, uint32_t limit, const uint32_t* owner_b = nullptr,
                        const uint8_t* through = nullptr, uint32_t Tmax = 0);
// Direct completion of the reduction: `out` is the device address of fine-grained page-locked
// memory, each final-stage block writes its point there, block 0 also copies *chain_src (the
// accumulate's longest chain) to *chain_dst, and then the block's flag takes `epoch` (system-scope
// release). The host polls the flags instead of a read-back copy and a stream wait.
struct TailDirect {
    uint32_t* flags = nullptr;
    uint32_t epoch = 0;
    const uint32_t* chain_src = nullptr;
    uint32_t* chain_dst = nullptr;
};
template <class C>
int msm_tail_reduce(vc_ctx* ctx, Lane L, const FAcc<C>* buckets, const uint32_t* offsets, uint32_t NB, int W,
                    uint32_t Lseg, uint32_t S, uint32_t J, FAcc<C>* accs, FAcc<C>* Rs, FAcc<C>* partial,
                    typename C::Acc* out, bool residue = false, const TailDirect* direct = nullptr);
}  // namespace vk

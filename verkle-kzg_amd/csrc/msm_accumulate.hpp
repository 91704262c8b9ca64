// The balanced bucket accumulate of the Pippenger MSM (msm.hip) and of the sparse commits
// (sparse_commit.hip): a template, instantiated by whoever launches it.
#pragma once
#include <type_traits>
#include "msm_tail.hpp"  // FAcc, ec29.hpp

namespace vk {
constexpr uint32_t NONE = 0xffffffffu;

// Start record of accumulate thread t (first sorted entry t M), written by the fine sort pass
// from the bucket starts it holds in LDS: the bucket b that holds entry t M, that bucket's
// [begin, end) in the sorted entries, and the end of bucket b + 1 (0: b is the last bucket of
// its coarse bin, whose block does not know it). The accumulate reads its record instead of
// searching offsets[]. One aligned 16-B load.
struct alignas(16) AccStart {
    uint32_t b, begin, end, next_end;
};

// ------------------------------------------------------------------ bucket accumulation
// The bases / phi / fixed-base tables read here are in the packed-29 form (x R', ec29.hpp)
// and the adds run in radix-2^29 arithmetic. Buckets and pieces are stored raw (radix-29) for
// the fix-up and the reduction (msm_tail.hip), which run the same arithmetic; converting them
// to the ec.hpp form at the three store sites (4 multiplies each) put ~50 KB of rarely-run code
// into the loop and cost 7 % of the kernel.
// BT: the base entry type -- packed-29 C::Aff (tables), the limb form of the fixed-base tables
// the sparse commits read (ec29.hpp FbE: the limbs in a 128-B entry), or the signed limb form of the
// shared-window copies (SW29::AffN: x, y, -y -- the entry's sign picks the y to load)
template <class FC, class BT, class = void>
struct is_affn : std::false_type {};
template <class FC, class BT>
struct is_affn<FC, BT, std::void_t<typename FC::AffN>> : std::is_same<BT, typename FC::AffN> {};
template <class FC, class BT, class = void>
struct is_affp : std::false_type {};
template <class FC, class BT>
struct is_affp<FC, BT, std::void_t<typename FC::AffP>> : std::is_same<BT, typename FC::AffP> {};
// a fixed-base table entry (FbE: the limbs in .u, padded to a 128-B line)
template <class C, class BT>
struct is_fbe : std::is_same<BT, FbE<C>> {};

template <class C, class BT = typename C::Aff>
__global__ void __launch_bounds__(256) VK_ACC_OCC k_msm_accumulate(
    const BT* __restrict__ bases, const BT* __restrict__ phi, uint32_t nphi,
    const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ offsets, uint32_t NBtot, uint32_t M,
    typename Fast29<C>::type::Acc* __restrict__ buckets, typename Fast29<C>::type::Acc* __restrict__ carry_in,
    uint8_t* __restrict__ through, typename Fast29<C>::type::Acc* __restrict__ owner_piece,
    uint32_t* __restrict__ owner_bucket, uint32_t* __restrict__ chain_max,
    unsigned long long* __restrict__ clk, const AccStart* __restrict__ starts) {
    using FC = typename Fast29<C>::type;
    using Aff = BT;
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t L = offsets[NBtot];  // entry count, read on the device: no host round trip
    uint32_t k = t * M;                 // grid sized for the n*W upper bound
    if (k >= L) return;
    // clock stamp (timing passes only: clk is null otherwise): shader cycles and 100 MHz ticks
    const bool stamp = clk != nullptr && t == 0;
    if (stamp) {
        clk[0] = __builtin_amdgcn_s_memtime();
        clk[1] = __builtin_amdgcn_s_memrealtime();
    }
    uint32_t e = min(k + M, L);
    owner_bucket[t] = NONE;
    through[t] = 0;
    // bucket b with offsets[b] <= k < offsets[b+1]: the thread's start record when the sort wrote
    // them (uniform over the grid), else a search of offsets[] (~log2 NBtot dependent loads)
    uint32_t b, bbeg, bend, nxt;  // nxt: the end of bucket b + 1, loaded a bucket ahead (0: not known)
    if (starts != nullptr) {
        const AccStart s = starts[t];
        b = s.b;
        bbeg = s.begin;
        bend = s.end;
        nxt = s.next_end;
    } else {
        uint32_t lo = 0, hi = NBtot;  // invariant offsets[lo] <= k < offsets[hi]
        while (hi - lo > 1) {
            uint32_t mid = (lo + hi) >> 1;
            if (offsets[mid] <= k) lo = mid;
            else hi = mid;
        }
        b = lo;
        bbeg = offsets[b];
        bend = offsets[b + 1];
        nxt = 0;
    }
    // threads from the bucket's owner (the thread that holds its first entry) to this one: 0 when
    // the bucket begins here, else its first piece is a carry piece (the bucket is open to the left)
    uint32_t left_open = t - bbeg / M;
    typename FC::Acc acc = FC::zero();
    // entry j < nphi: bases[j]; j >= nphi: phi[j - nphi] (the GLV endomorphism images)
    auto base_of = [&](uint32_t j) -> const Aff* { return j < nphi ? bases + j : phi + (j - nphi); };
    constexpr bool SN = is_affn<FC, BT>::value;
    constexpr bool SP = is_affp<FC, BT>::value;  // pair layout: the sign picks the record
    constexpr bool FBE = is_fbe<C, BT>::value;   // fixed-base entries: the limbs, not the padding
    using Pre = std::conditional_t<SN || SP || FBE, typename FC::Aff, Aff>;  // the prefetched entry
    auto fetch = [&](uint32_t id) -> Pre {
        if constexpr (FBE) {
            return base_of(id & 0x7fffffffu)->u;
        } else if constexpr (SP) {
            const Aff* r = bases + 2 * (size_t)(id & 0x7fffffffu) + (id >> 31);
            typename FC::Aff a;
            a.x = r->x;
            a.y = r->y;
            return a;
        } else {
            const Aff* b = base_of(id & 0x7fffffffu);
            if constexpr (SN) {
                typename FC::Aff a;
                a.x = b->x;
                // y or -y through the address (a select of values would load both)
                a.y = *reinterpret_cast<const decltype(a.y)*>(reinterpret_cast<const char*>(&b->y) +
                                                              ((id >> 31) ? sizeof(a.y) : 0u));
                return a;
            } else {
                return *b;
            }
        }
    };
    uint32_t idx = sorted[k];
    uint32_t idx2 = sorted[min(k + 1, e - 1)];
    Pre P = fetch(idx);
    while (true) {
        uint32_t cur = idx;
        typename FC::Aff Q;
        if constexpr (SN || SP || FBE) Q = P;
        else Q = FC::load(&P);
        // prefetch the next base; its entry index was loaded an iteration earlier, so the gather's
        // address waits on no load. Unconditional (the thread's last entry again at its end): under
        // `if (k + 1 < e)` the loaded registers were copied into P's behind waits on the loads
        // just issued
        idx = idx2;
        idx2 = sorted[min(k + 2, e - 1)];
        P = fetch(idx);
        acc = FC::madd(acc, Q, !SN && !SP && (cur >> 31) != 0);
        k++;
        if (k == bend || k == e) {
            bool right_open = (k == e) && (bend > e);
            if (!left_open && !right_open) {
                buckets[b] = acc;
            } else if (left_open) {
                carry_in[t] = acc;
                through[t] = right_open ? 2 : 1;  // 1: carry piece ending here, 2: bucket continues
                // chain end: chain length = carry threads of this bucket
                if (!right_open && left_open >= 2) atomicMax(chain_max, left_open);
            } else {
                owner_piece[t] = acc;
                owner_bucket[t] = b;
            }
            if (k == e) break;
            left_open = 0;
            acc = FC::zero();
            // the next bucket's end was loaded when this one was entered, so no load issued here is
            // needed before the next add. Slow path: empty buckets follow (their ends are <= k) or
            // the end is not known (0): walk offsets[] (k < e <= offsets[NBtot] ends it)
            if (nxt > k) {
                b++;
                bend = nxt;
            } else {
                do {
                    b++;
                    bend = offsets[b + 1];
                } while (bend <= k);
            }
            nxt = offsets[min(b + 2, NBtot)];
        }
    }
    if (stamp) {
        clk[2] = __builtin_amdgcn_s_memtime();
        clk[3] = __builtin_amdgcn_s_memrealtime();
    }
}

// radix-29 bucket accumulators -> ec.hpp form, non-empty buckets only (empty ones keep what the
// caller put there)
template <class C>
__global__ void __launch_bounds__(256) k_fast_store(const FAcc<C>* __restrict__ a, uint32_t n,
                                                   const uint32_t* __restrict__ offsets, typename C::Acc* __restrict__ o) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && offsets[i + 1] > offsets[i]) o[i] = Fast29<C>::type::store(a[i]);
}
}  // namespace vk

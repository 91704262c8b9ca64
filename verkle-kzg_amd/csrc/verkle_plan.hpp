// The device-resident verkle commitment's host integer logic (verkle_commit_dev.hip): the delta plan
// made from the insert-time slot log, each internal level's lists, and the dense-level rule both
// commitment paths share. Host only: tests/cpp/verkle_plan_check.cpp runs it without a GPU.
#pragma once
#include <cstdlib>
#include <functional>

#include "verkle_trie.hpp"

namespace vk {

// VKZG_VERKLE_DENSE (read per call): 0 = every level sparse, 1 = every level dense, unset = by size
inline int verkle_dense_mode() {
    const char* env = getenv("VKZG_VERKLE_DENSE");
    return env ? atoi(env) : -1;
}
// a level of B rows commits as dense rows on the fixed-base latency path (vc_msm_batch; the root's
// one commit 0.44 -> 0.11 ms) when it has <= 64 rows: the sparse path's ~10
// latency-bound launches and host round trips cost ~0.35 ms even for one row; larger levels stay
// sparse (dense measured slower at 65 rows, equal at 65,536 x 4: profiles/r04/verkle/)
inline bool verkle_dense_level(int dense_mode, size_t B) { return dense_mode == 1 || (dense_mode != 0 && B <= 64); }

// Delta rows: an updated internal node whose last commitment is in the mirror (base) is
// C_old + sum over its changed slots of (item(child now) - item(child then)) L_slot, instead of
// its full row (~160 children per level-1 node of a 65,536-key tree, ~2 of them changed by a
// 1 % update). The changed slots are the slot log's (first entry per slot: the child at the last
// commitment); snap_ids lists the children whose old items the rows subtract (snapshotted by the
// caller before the commitment's scatters overwrite them). While the plan lives, plan_slot[id] is
// node id's plan and snap_slot[id] its index in snap_ids; both are -1 again once it dies.
struct DeltaPlan {
    struct Plan {
        uint64_t seen[4];
        uint32_t start, cnt;  // its entries in plan_e: (slot, snapshot index; -1: the slot was empty)
    };
    std::vector<Plan> plans;
    std::vector<std::pair<uint8_t, int32_t>> plan_e;
    std::vector<uint32_t> snap_ids;

    // enabled = false (or an empty log): no plans, every row is committed in full
    explicit DeltaPlan(VTrie& t, bool enabled = true) : t_(t) {
        if (!enabled || t.slog.empty()) return;
        // pass 1: a plan per logged parent, the first entry per (parent, slot) kept; snapshot slots
        std::vector<int32_t> kept(t.slog.size(), -1);  // its plan, or -1 for a repeated slot
        for (size_t i = 0; i < t.slog.size(); i++) {
            const auto& L = t.slog[i];
            int32_t p = t.plan_slot[L.parent];
            if (p < 0) {
                p = (int32_t)plans.size();
                plans.push_back(Plan{{0, 0, 0, 0}, 0, 0});
                t.plan_slot[L.parent] = p;
                plan_nodes_.push_back(L.parent);
            }
            Plan& P = plans[p];
            if ((P.seen[L.slot >> 6] >> (L.slot & 63)) & 1) continue;
            P.seen[L.slot >> 6] |= 1ull << (L.slot & 63);
            P.cnt++;
            kept[i] = p;
            if (L.old >= 0 && t.snap_slot[L.old] < 0) {
                t.snap_slot[L.old] = (int32_t)snap_ids.size();
                snap_ids.push_back((uint32_t)L.old);
            }
        }
        // pass 2: the entries grouped by plan
        uint32_t run = 0;
        for (auto& P : plans) {
            P.start = run;
            run += P.cnt;
            P.cnt = 0;
        }
        plan_e.resize(run);
        for (size_t i = 0; i < t.slog.size(); i++) {
            if (kept[i] < 0) continue;
            const auto& L = t.slog[i];
            Plan& P = plans[kept[i]];
            plan_e[P.start + P.cnt++] = {L.slot, L.old >= 0 ? t.snap_slot[L.old] : -1};
        }
    }
    ~DeltaPlan() {
        for (int id : plan_nodes_) t_.plan_slot[id] = -1;
        for (uint32_t id : snap_ids) t_.snap_slot[id] = -1;
    }
    DeltaPlan(const DeltaPlan&) = delete;
    DeltaPlan& operator=(const DeltaPlan&) = delete;
    // the delta row of node `id`, or null: its row is committed in full
    const Plan* row(int id) const {
        if (plans.empty() || !t_.base[id] || t_.plan_slot[id] < 0) return nullptr;
        return &plans[t_.plan_slot[id]];
    }

private:
    VTrie& t_;
    std::vector<int> plan_nodes_;  // nodes whose plan_slot is set
};

// One internal level's lists (column, child id[, snapshot index] per non-zero, node ids[, the
// delta rows' add ids]) in one buffer for one upload: ints only, the values are the children's
// items in the mirror (minus the snapshot for a delta row).
// Layout: cols | child | ids | (any_delta) sidx | add_ids
struct LevelLists {
    int level = -1, status = VC_OK;
    size_t B = 0, nnz = 0, o_child = 0, o_ids = 0, o_sidx = 0, o_add = 0, o_end = 0;
    bool any_delta = false, dense = false;
    uvec<uint64_t> ptr;
    uint8_t* pin = nullptr;
};
// the lists of t.dirty_int[level] into buffer(bytes) (page-locked in the commitment); L.status is
// VC_E_OOM when the buffer cannot be had. A dense level (verkle_dense_level) commits full rows
// (delta rows would not shorten the latency path's dependent adds).
inline void level_lists(const VTrie& t, int level, const DeltaPlan& plan, int dense_mode, HostPool& pool,
                        const std::function<uint8_t*(size_t)>& buffer, LevelLists& L) {
    const std::vector<int>& lv = t.dirty_int[level];
    const size_t B = lv.size();
    L.level = level;
    L.B = B;
    std::vector<const DeltaPlan::Plan*> rplan(B, nullptr);
    bool any_delta = false;
    L.dense = verkle_dense_level(dense_mode, B);
    if (!L.dense)
        for (size_t b = 0; b < B; b++)
            if ((rplan[b] = plan.row(lv[b]))) any_delta = true;
    L.any_delta = any_delta;
    L.ptr.resize(B + 1);
    uvec<uint64_t>& ptr = L.ptr;
    ptr[0] = 0;
    for (size_t b = 0; b < B; b++)
        ptr[b + 1] = ptr[b] + (rplan[b] ? rplan[b]->cnt : t.nodes[lv[b]].children.v.size());
    const size_t nnz = ptr[B], nz1 = std::max<size_t>(nnz, 1);
    L.nnz = nnz;
    L.o_child = nz1 * 4;
    L.o_ids = L.o_child + nz1 * 4;
    L.o_sidx = L.o_ids + B * 4;
    L.o_add = L.o_sidx + (any_delta ? nz1 * 4 : 0);
    L.o_end = L.o_add + (any_delta ? B * 4 : 0);
    uint8_t* pin = buffer(L.o_end);
    L.pin = pin;
    L.status = pin ? VC_OK : VC_E_OOM;
    if (!pin) return;
    uint32_t* cols = reinterpret_cast<uint32_t*>(pin);
    uint32_t* child = reinterpret_cast<uint32_t*>(pin + L.o_child);
    uint32_t* ids = reinterpret_cast<uint32_t*>(pin + L.o_ids);
    int32_t* sidx = reinterpret_cast<int32_t*>(pin + L.o_sidx);
    uint32_t* add_ids = reinterpret_cast<uint32_t*>(pin + L.o_add);
    pool_for(pool, 0, B, 256, [&](size_t b) {
        size_t j = ptr[b];
        const VNode& n = t.nodes[lv[b]];
        ids[b] = (uint32_t)lv[b];
        if (rplan[b]) {
            for (uint32_t q = 0; q < rplan[b]->cnt; q++) {
                const auto& e = plan.plan_e[rplan[b]->start + q];
                cols[j] = e.first;
                child[j] = (uint32_t)n.children.find(e.first)->second;
                sidx[j] = e.second;
                j++;
            }
        } else {
            for (auto& kv : n.children.v) {
                cols[j] = kv.first;
                child[j] = (uint32_t)kv.second;
                if (any_delta) sidx[j] = -1;
                j++;
            }
        }
        if (any_delta) add_ids[b] = rplan[b] ? (uint32_t)lv[b] : 0xffffffffu;
    });
}

}  // namespace vk

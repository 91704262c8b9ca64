// The verkle commitment with host-built rows (gen_commitment, node.rs:205-277, level-batched): every
// level's rows are built on the host with their values, committed through vc_msm_batch_sparse +
// vc_to_data_item_batch (or the dense latency path) and the results stored in the tree's host
// arrays. The path of the sharded and group commitments, and VKZG_VERKLE_DEV=0's.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scheme_internal.hpp"
#include "verkle_internal.hpp"
#include "verkle_plan.hpp"

namespace vk {
namespace {

// results of one batched commit: a row's affine point, identity flag and to_data_item
// (written in full by the commits: uninitialised staging, host/pool.hpp uvec)
struct RowResults {
    uvec<uint64_t> xy, items;
    uvec<uint8_t> inf;
    void resize(size_t B) {
        xy.resize(B * 8);
        inf.resize(B);
        items.resize(B * 4);
    }
};

struct HostCommit {
    vc_ctx* ctx;
    int table;
    vc_verkle* t;
    const Shard* sh;  // this rank's slices of every level, one all-gather per level
    const Multi* mu;  // every level's rows cut into member slices
    HostPool& pool = host_pool();
    const int dense_mode = verkle_dense_mode();
    uvec<uint64_t> dense;
    RowResults res, res4;  // kept across levels (res: the c1 / c2 rows, then every internal level; res4: the width-4 rows)
    std::chrono::steady_clock::time_point tic = std::chrono::steady_clock::now();

    void lap(const char* what) {
        if (!verbose()) return;
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[verkle] %s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - tic).count());
        tic = now;
    }
    // fn(i) for i in [0, count) on the pool (independent per-item writes)
    template <class Fn>
    void for_each(size_t count, Fn fn) {
        pool_for(pool, 0, count, 4096, fn);
    }
    // this rank's slice of a level of B rows
    void slice(size_t B, size_t* lo, size_t* hi) const {
        *lo = sh ? B * sh->rank / sh->world : 0;
        *hi = sh ? B * (sh->rank + 1) / sh->world : B;
    }

    // dense rows (vc_msm_batch: the fixed-base batched commit over the first `width` bases); the
    // <= 64 points' to_data_item on the host (compress + mod r, no inversion: already affine)
    int commit_dense(const Rows& r, size_t width, RowResults& out) {
        const size_t B = r.n();
        dense.resize(B * width * 4);
        for_each(B, [&](size_t b) {
            uint64_t* row = &dense[b * width * 4];
            memset(row, 0, width * 32);
            for (uint64_t e = r.ptr[b]; e < r.ptr[b + 1]; e++) memcpy(row + 4 * (size_t)r.cols[e], &r.vals[4 * e], 32);
        });
        VK_TRY(vc_msm_batch(ctx, table, width, dense.data(), B, 0, out.xy.data(), out.inf.data()));
        for (size_t b = 0; b < B; b++) {
            const Fr it = to_data_item_host(&out.xy[8 * b], out.inf[b] != 0);
            mont_to_canon<BN254Fr>(it, &out.items[4 * b]);
        }
        lap("dense commit + to_data_item");
        return VC_OK;
    }
    // member k commits rows [B k / G, B (k + 1) / G) of the level on its own device
    int commit_members(const Rows& r, RowResults& out) {
        const size_t B = r.n();
        const int G = (int)mu->ctx.size();
        std::vector<int> st(G, VC_OK);
        mu->run([&](int k) {
            size_t a, e;
            shard_range(B, k, G, &a, &e);
            if (a == e) return;
            std::vector<uint64_t> rp(e - a + 1);
            const uint64_t base = r.ptr[a];
            for (size_t i = 0; i <= e - a; i++) rp[i] = r.ptr[a + i] - base;
            const uint32_t* cols = r.cols.size() ? r.cols.data() + base : nullptr;
            const uint64_t* vals = r.vals.size() ? r.vals.data() + 4 * base : nullptr;
            st[k] = msm_batch_sparse_items_guarded(mu->ctx[k], mu->table[k], e - a, rp.data(), cols, vals,
                                                   out.xy.data() + 8 * a, out.inf.data() + a, out.items.data() + 4 * a);
        });
        for (int s : st)
            if (s != VC_OK) return s;
        lap("sparse commit + to_data_item (members)");
        return VC_OK;
    }
    // the rows' commitments and items by one of three routes: dense (small levels of one context),
    // the group's members, or this context's sparse commit
    int commit_rows(const Rows& r, size_t width, RowResults& out) {
        const size_t B = r.n();
        out.resize(B);
        if (B == 0) return VC_OK;
        lap("build rows");
        if (!mu && verkle_dense_level(dense_mode, B)) return commit_dense(r, width, out);
        if (mu) return commit_members(r, out);
        // the rows' commitments and their to_data_item values in one call (items computed on the
        // device from the normalised points: no second upload / read-back per level)
        VK_TRY(msm_batch_sparse_items_guarded(ctx, table, B, r.ptr.data(), r.cols.data(), r.vals.data(), out.xy.data(),
                                              out.inf.data(), out.items.data()));
        lap("sparse commit + to_data_item");
        return VC_OK;
    }

    void put(int id, const uint64_t* rxy, uint8_t rinf, const uint64_t* ritem) {
        memcpy(&t->cxy[8 * (size_t)id], rxy, 64);
        t->cinf[id] = rinf;
        memcpy(&t->item[4 * (size_t)id], ritem, 32);
        t->has_commit[id] = 1;
    }
    // the sharded exchange: every rank's slice of the level as VK_NODE_REC-word records behind its
    // status word, all-gathered, so every rank stores the whole level.
    // st: this rank's status for the level -- a failed share still enters the exchange with it
    // (include/vc_comm.h), so every rank stops at the same level with an error
    int exchange_level(const std::vector<int>& ids, size_t lo, size_t hi, const RowResults& got, int st) {
        constexpr size_t REC = VK_NODE_REC;
        const size_t B = ids.size(), bmax = (B + sh->world - 1) / sh->world, slot = 1 + bmax * REC;
        std::vector<uint64_t> send(slot, 0), recv(slot * sh->world);
        send[0] = (uint64_t)(uint32_t)st;
        for (size_t b = 0; st == VC_OK && b < hi - lo; b++) {
            memcpy(&send[1 + b * REC], &got.xy[b * 8], 64);
            memcpy(&send[1 + b * REC + 8], &got.items[b * 4], 32);
            send[1 + b * REC + 12] = got.inf[b];
        }
        VK_TRY(sh->allgather(send.data(), send.size() * 8, recv.data()));
        if (st != VC_OK) return st;
        for (int k = 0; k < sh->world; k++)
            if ((int32_t)(uint32_t)recv[(size_t)k * slot] != VC_OK) return VC_E_PEER;
        for (int k = 0; k < sh->world; k++) {
            const size_t a = B * k / sh->world, e = B * (k + 1) / sh->world;
            const uint64_t* src = &recv[(size_t)k * slot + 1];
            for_each(e - a, [&](size_t b) {
                const uint64_t* rec = src + b * REC;
                put(ids[a + b], rec, (uint8_t)rec[12], rec + 8);
            });
        }
        return VC_OK;
    }
    // the nodes ids[lo, hi) of a level got these results here: store them (with a shard, the whole level)
    int store_level(const std::vector<int>& ids, size_t lo, size_t hi, const RowResults& got, int st) {
        if (sh) return exchange_level(ids, lo, hi, got, st);
        if (st != VC_OK) return st;
        for_each(hi - lo, [&](size_t b) { put(ids[lo + b], &got.xy[b * 8], got.inf[b], &got.items[b * 4]); });
        return VC_OK;
    }

    // extension nodes: c1, c2 (width N), then [1, stem, c1, c2] (width 4) -- both steps only need
    // the node's own values, so a rank runs both on its slice and exchanges once
    int extension_level(const std::vector<int>& exts) {
        const int N = t->N;
        size_t lo, hi;
        slice(exts.size(), &lo, &hi);
        Rows r12 = build_rows(pool, lo, hi, (size_t)N, [&](size_t e, Rows& r) { ext_rows(*t, exts[e], r); },
                              [&](size_t e, int stage) { ext_prefetch(*t, exts[e], stage); });
        int st = commit_rows(r12, (size_t)N, res);
        Rows rx;
        if (st == VC_OK) rx = build_rows(pool, lo, hi, 4, [&](size_t e, Rows& r) {
            const VNode& n = t->nodes[exts[e]];
            uint64_t one[4] = {1, 0, 0, 0}, stem_item[4];
            item_of_bytes(n.stem.data(), N, stem_item);  // bytes_to_item(stem.to_bytes())
            r.add(0, one);
            r.add(1, stem_item);
            r.add(2, &res.items[(2 * (e - lo)) * 4]);
            r.add(3, &res.items[(2 * (e - lo) + 1) * 4]);
            r.end_row();
        }, [&](size_t e, int stage) {
            if (stage == 0) __builtin_prefetch(t->nodes[exts[e]].stem.data());
        });
        if (st == VC_OK) st = commit_rows(rx, 4, res4);
        return store_level(exts, lo, hi, res4, st);
    }
    // one depth of internal nodes (HACK in the reference: width hard-coded 256); a parent needs
    // its children's items, so every depth is one exchange
    int internal_level(const std::vector<int>& lv) {
        size_t lo, hi;
        slice(lv.size(), &lo, &hi);
        size_t kids = 0;  // children of the slice (the rows' non-zero bound)
        for (size_t b = lo; b < hi; b++) kids += t->nodes[lv[b]].children.v.size();
        Rows ri = build_rows(pool, lo, hi, hi > lo ? (kids + hi - lo - 1) / (hi - lo) : 1, [&](size_t b, Rows& r) {
            for (auto& kv : t->nodes[lv[b]].children) r.add(kv.first, &t->item[4 * (size_t)kv.second]);
            r.end_row();
        }, [&](size_t b, int stage) {
            const VNode& n = t->nodes[lv[b]];
            if (stage == 0) {
                __builtin_prefetch(&n);
                __builtin_prefetch(reinterpret_cast<const char*>(&n) + 64);
            } else if (!n.children.v.empty()) {
                __builtin_prefetch(n.children.v.data());
            }
        });
        const int st = commit_rows(ri, 256, res);
        return store_level(lv, lo, hi, res, st);
    }
};

}  // namespace

int verkle_commitment(vc_ctx* ctx, int table, vc_verkle* t, uint64_t* out_xy, uint8_t* out_inf, const Shard* sh,
                      const Multi* mu) {
    if (!ctx || !t || !out_xy || !out_inf || (sh && mu)) return VC_E_INVALID;
    // the host path reads and writes the host arrays: bring them up to date, and drop the device
    // mirror afterwards (it would miss this call's results)
    VK_TRY(mirror_pull(t));
    struct DropMirror {
        vc_verkle* t;
        ~DropMirror() { t->dev.release(); }
    } drop{t};
    DeltaGuard delta_guard{t};
    HostCommit H{ctx, table, t, sh, mu};
    std::vector<int> exts;
    std::vector<std::vector<int>> internals;  // by depth
    collect_dirty(*t, H.pool, exts, internals);
    H.lap("collect dirty");
    if (!exts.empty()) VK_TRY(H.extension_level(exts));
    for (int depth = (int)internals.size() - 1; depth >= 0; depth--) VK_TRY(H.internal_level(internals[depth]));  // deepest first
    memcpy(out_xy, &t->cxy[0], 64);
    *out_inf = t->cinf[0];
    t->clear_dirty();
    delta_guard.ok = true;
    return VC_OK;
}

}  // namespace vk

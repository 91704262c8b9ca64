// Verkle tree (reference verkle-tree/src/{lib,node}.rs) with level-batched commitments on the
// GPU engine: the C ABI's tree calls (include/vc_verkle.h) over the host trie (verkle_trie.hpp), the
// device mirror's management and the choice of commitment path -- device-resident levels
// (verkle_commit_dev.hip) or host-built rows (verkle_commit_host.cpp). Proofs: verkle_proof.hip.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "verkle_internal.hpp"

extern "C" {

vc_verkle* vc_verkle_new(int key_len) {
    if (key_len < 2 || key_len > 32) return nullptr;
    vc_verkle* t = new vc_verkle();
    vk::trie_init(*t, key_len);
    t->grow_results();
    return t;
}

void vc_verkle_free(vc_verkle* t) { delete t; }

int vc_verkle_insert(vc_verkle* t, const uint8_t* key, const uint8_t* value) {
    if (!t || !key || !value) return VC_E_INVALID;
    const int st = vk::trie_insert(*t, key, value);
    t->grow_results();
    return st;
}

int vc_verkle_get(const vc_verkle* t, const uint8_t* key, uint8_t* value, int* found) {
    if (!t || !key || !value || !found) return VC_E_INVALID;
    *found = vk::trie_get(*t, key, value) ? 1 : 0;
    return VC_OK;
}

int vc_verkle_path(const vc_verkle* t, const uint8_t* key, size_t max_len, uint8_t* units, size_t* len) {
    if (!t || !key || !len) return VC_E_INVALID;
    return vk::trie_path(*t, key, max_len, units, len);
}

// diagnostics (tools/verkle_nodes.py): per node id, type (0 internal, 1 extension), level and the
// committed item (the device mirror's values brought to the host first)
int vc_verkle_debug_nodes(vc_verkle* t, size_t max, uint8_t* type, int32_t* level, uint64_t* items, size_t* n) {
    if (!t || !n) return VC_E_INVALID;
    VK_TRY(vk::mirror_pull(t));
    const size_t m = std::min(max, t->nodes.size());
    for (size_t i = 0; i < m; i++) {
        if (type) type[i] = t->nodes[i].ext ? 1 : 0;
        if (level) level[i] = t->nodes[i].level;
        if (items) memcpy(items + 4 * i, &t->item[4 * i], 32);
    }
    *n = t->nodes.size();
    return VC_OK;
}

// diagnostics (tools/verkle_host_probe.py, no GPU): the device path's extension host stage (rows
// built and merged into a plain buffer) over every extension node, `reps` times; *us = the median
int vc_verkle_debug_ext_stage(vc_verkle* t, int reps, double* us) {
    if (!t || !us || reps < 1) return VC_E_INVALID;
    return vk::verkle_debug_ext_stage(t, reps, us);
}

int vc_verkle_stats(const vc_verkle* t, size_t* internal, size_t* extension, size_t* dirty) {
    if (!t) return VC_E_INVALID;
    vk::trie_stats(*t, internal, extension, dirty);
    return VC_OK;
}

// gen_commitment (node.rs:205-277), level-batched
int vc_verkle_commitment(vc_ctx* ctx, int table, vc_verkle* t, uint64_t* out_xy, uint8_t* out_inf) {
    // the device-resident levels; VKZG_VERKLE_DEV=0 (read per call, A/B probe) takes the host path
    const char* env = getenv("VKZG_VERKLE_DEV");
    if (env && atoi(env) == 0) return vk::verkle_commitment(ctx, table, t, out_xy, out_inf, nullptr);
    return vk::verkle_commitment_dev(ctx, table, t, out_xy, out_inf);
}

}  // extern "C"

namespace vk {

int verkle_debug_ext_stage(vc_verkle* t, int reps, double* us) {
    std::vector<int> exts;
    for (size_t i = 0; i < t->nodes.size(); i++)
        if (t->nodes[i].ext) exts.push_back((int)i);
    std::vector<ExtRows16> cache;
    std::vector<uint8_t> buf;
    std::vector<double> ts, tbs;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        ExtStage X;
        double tb = 0;
        VK_TRY(ext_stage(*t, exts, host_pool(), cache,
                         [&](size_t bytes) -> uint8_t* {
                             if (buf.size() < bytes) buf.resize(bytes);
                             return buf.data();
                         },
                         &X, &tb));
        ts.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        tbs.push_back(tb);
    }
    if (verbose()) {  // one thread over the whole level, and the stem items alone
        ExtRows16 r;
        r.reserve(exts.size(), exts.size() * 4);
        auto c0 = std::chrono::steady_clock::now();
        for (size_t e = 0; e < exts.size(); e++) ext_rows16(*t, exts[e], r);
        auto c1 = std::chrono::steady_clock::now();
        uint64_t acc = 0, w[4];
        for (size_t e = 0; e < exts.size(); e++) {
            item_of_bytes(t->nodes[exts[e]].stem.data(), t->N, w);
            acc ^= w[0];
        }
        auto c2 = std::chrono::steady_clock::now();
        fprintf(stderr, "[ext stage] one thread: rows %.1f us, stem items alone %.1f us (%llu), sizeof(VNode) %zu\n",
                std::chrono::duration<double, std::micro>(c1 - c0).count(),
                std::chrono::duration<double, std::micro>(c2 - c1).count(), (unsigned long long)(acc & 1), sizeof(VNode));
    }
    std::sort(ts.begin(), ts.end());
    std::sort(tbs.begin(), tbs.end());
    *us = ts[ts.size() / 2];
    if (verbose())
        fprintf(stderr, "[ext stage] %zu extensions, %u threads: build %.1f us, total %.1f us (medians)\n", exts.size(),
                host_pool().size(), tbs[tbs.size() / 2], *us);
    return VC_OK;
}

// ---- device mirror (VerkleDev) management
int mirror_pull(vc_verkle* t) {
    VerkleDev& D = t->dev;
    if (t->host_valid) return VC_OK;
    const size_t n = std::min(t->nodes.size(), D.cap);
    if (D.ctx_uid && n) {
        DeviceScope on(D.dev);  // the mirror's device, the caller's restored on return (a move to
                                // another context allocates the new mirror on that one's device)
        VK_CHECK_HIP(hipMemcpy(t->item.data(), D.item, n * 32, hipMemcpyDeviceToHost));
        VK_CHECK_HIP(hipMemcpy(t->cxy.data(), D.cxy, n * 64, hipMemcpyDeviceToHost));
        VK_CHECK_HIP(hipMemcpy(t->cinf.data(), D.inf, n, hipMemcpyDeviceToHost));
    }
    t->host_valid = true;
    return VC_OK;
}
int verkle_pull_host(vc_verkle* t) { return mirror_pull(t); }

int mirror_prepare(vc_ctx* ctx, vc_verkle* t) {
    VerkleDev& D = t->dev;
    const size_t n = t->nodes.size();
    if (D.ctx_uid != ctx->uid) {  // first use, or another context: rebuild from the host arrays
        VK_TRY(mirror_pull(t));
        D.release();
        VK_CHECK_HIP(hipSetDevice(ctx->device));  // (both restore it; allocations below are ctx's)
    }
    const bool fresh = D.ctx_uid == 0;
    if (D.cap < n) {  // (with room: a tree that grows by an update's splits keeps its buffers)
        const size_t cap = std::max<size_t>({n + n / 4, 2 * D.cap, 1024});
        void* blk = nullptr;  // one allocation: items, commitments, flags
        size_t blk_bytes = 0;
        VK_TRY(pool_take(ctx, cap * (32 + 64 + 1), &blk, &blk_bytes));
        void* p[3] = {blk, static_cast<uint8_t*>(blk) + cap * 32, static_cast<uint8_t*>(blk) + cap * 96};
        if (!fresh && D.cap) {  // keep the committed results (every id < the old capacity)
            VK_CHECK_HIP(hipMemcpyAsync(p[0], D.item, D.cap * 32, hipMemcpyDeviceToDevice, ctx->stream));
            VK_CHECK_HIP(hipMemcpyAsync(p[1], D.cxy, D.cap * 64, hipMemcpyDeviceToDevice, ctx->stream));
            VK_CHECK_HIP(hipMemcpyAsync(p[2], D.inf, D.cap, hipMemcpyDeviceToDevice, ctx->stream));
            VK_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        }
        if (D.item) pool_put(ctx, D.item, D.blk_bytes);  // (the block's start; this context's, copied above)
        D.item = p[0];
        D.cxy = p[1];
        D.inf = p[2];
        D.cap = cap;
        D.blk_bytes = blk_bytes;
    }
    if (fresh) {  // the host arrays are current (mirror_pull above): upload them -- unless no node
        // has a commitment yet (a fresh tree: every value is written by this commitment)
        if (t->dirty_count() < n) {
            VK_CHECK_HIP(hipMemcpyAsync(D.item, t->item.data(), n * 32, hipMemcpyHostToDevice, ctx->stream));
            VK_CHECK_HIP(hipMemcpyAsync(D.cxy, t->cxy.data(), n * 64, hipMemcpyHostToDevice, ctx->stream));
            VK_CHECK_HIP(hipMemcpyAsync(D.inf, t->cinf.data(), n, hipMemcpyHostToDevice, ctx->stream));
        }
        D.ctx_uid = ctx->uid;
        D.dev = ctx->device;
    }
    return VC_OK;
}

}  // namespace vk

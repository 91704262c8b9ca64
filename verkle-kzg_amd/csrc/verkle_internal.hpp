// Shared by the verkle translation units (verkle.cpp, verkle_commit_host.cpp, verkle_commit_dev.hip,
// verkle_proof.hip): the tree with its per-node results and device mirror.
#pragma once
#include "../../include/vc_scheme.h"
#include "../../include/vc_verkle.h"
#include "comm.hpp"
#include "ctx.hpp"
#include "verkle_rows.hpp"

// Device mirror of the tree's per-node results (one context's device): commitments, flags and
// to_data_item values indexed by node id, so a level's rows gather their children's items on the
// device and nothing travels back between levels (verkle_commit_dev.hip)
struct VerkleDev {
    uint64_t ctx_uid = 0;  // the context whose device holds it (0: none)
    int dev = -1;
    void* item = nullptr;  // [cap] x 4 u64 (the start of the one allocation)
    void* cxy = nullptr;   // [cap] x 8 u64
    void* inf = nullptr;   // [cap] u8
    size_t cap = 0, blk_bytes = 0;
    // the block comes from the context's pool and goes back to it (a fresh tree's mirror then
    // costs no hipMalloc: ~0.4 ms of a 4-ms full commitment)
    void release() {
        vk::pool_return_uid(ctx_uid, dev, item, blk_bytes);  // one block: item, then cxy, then inf
        item = cxy = inf = nullptr;
        cap = blk_bytes = 0;
        ctx_uid = 0;
        dev = -1;
    }
    ~VerkleDev() { release(); }
};

struct vc_verkle : vk::VTrie {
    // per-node results (node id order): canonical affine commitment, identity flag, to_data_item
    std::vector<uint64_t> cxy;
    std::vector<uint8_t> cinf;
    std::vector<uint64_t> item;
    VerkleDev dev;
    bool host_valid = true;  // false: the device mirror holds newer results than cxy / cinf / item
    // the result arrays in step with the nodes (after every call that may add some)
    void grow_results() {
        const size_t n = nodes.size();
        cxy.resize(8 * n, 0);
        cinf.resize(n, 1);
        item.resize(4 * n, 0);
    }
};

namespace vk {

// drop_delta unless the commitment reached its end (ok = true)
struct DeltaGuard {
    vc_verkle* t;
    bool ok = false;
    ~DeltaGuard() {
        if (!ok) t->drop_delta();
    }
};

// a node's record where the paths pass results around (the sharded all-gather's wire format, the
// proofs' gather out of the mirror): commitment (8 u64) | item (4) | flag (1)
constexpr size_t VK_NODE_REC = 13;

// the mirror's results -> the host arrays (before a host-path commitment or a move to another
// context's device)
int mirror_pull(vc_verkle* t);
// a mirror on ctx's device holding every committed node's results, with room for every node
int mirror_prepare(vc_ctx* ctx, vc_verkle* t);

}  // namespace vk

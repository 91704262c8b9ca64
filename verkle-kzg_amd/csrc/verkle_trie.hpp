// The verkle tree's host data structure (reference verkle-tree/src/{lib,node}.rs): nodes, insert /
// get / path, the dirty lists and the slot log the device path's delta rows are planned from.
// Host only (plain C++17, no device or result state: that is vc_verkle in verkle_internal.hpp), so
// tests/cpp/verkle_plan_check.cpp builds it with g++.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/vc_verkle.h"
#include "host/fr.hpp"
#include "host/pool.hpp"

namespace vk {

// a sorted run of entries whose first one lives inside the owner (an extension node of random
// keys holds one leaf: its rows are built from the node's own cache lines, no second miss into
// the heap); std::vector's API subset FlatMap uses
template <class T>
struct InlineVec {
    uint32_t n = 0;
    T inl[1];
    std::vector<T> heap;  // n >= 2: every entry here
    T* begin() { return n <= 1 ? inl : heap.data(); }
    T* end() { return begin() + n; }
    const T* begin() const { return n <= 1 ? inl : heap.data(); }
    const T* end() const { return begin() + n; }
    T* data() { return begin(); }
    const T* data() const { return begin(); }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    T* insert(T* it, const T& v) {
        const size_t k = (size_t)(it - begin());
        if (n == 0) {
            inl[0] = v;
            n = 1;
            return inl;
        }
        if (n == 1) heap.assign(inl, inl + 1);
        heap.insert(heap.begin() + (std::ptrdiff_t)k, v);
        n++;
        return heap.data() + k;
    }
};

// unit -> V, sorted by unit in one vector: the std::map API subset the tree uses, without a heap
// node per entry (pointer chasing made the commitment's node walks ~150 ns per node)
template <class V, class Vec = std::vector<std::pair<uint8_t, V>>>
struct FlatMap {
    Vec v;
    using iterator = decltype(v.begin());
    using const_iterator = decltype(static_cast<const Vec&>(v).begin());
    iterator begin() { return v.begin(); }
    iterator end() { return v.end(); }
    const_iterator begin() const { return v.begin(); }
    const_iterator end() const { return v.end(); }
    iterator lower(uint8_t k) {
        return std::lower_bound(v.begin(), v.end(), k, [](const std::pair<uint8_t, V>& a, uint8_t b) { return a.first < b; });
    }
    const_iterator lower(uint8_t k) const {
        return std::lower_bound(v.begin(), v.end(), k, [](const std::pair<uint8_t, V>& a, uint8_t b) { return a.first < b; });
    }
    iterator find(uint8_t k) {
        auto it = lower(k);
        return (it != v.end() && it->first == k) ? it : v.end();
    }
    const_iterator find(uint8_t k) const {
        auto it = lower(k);
        return (it != v.end() && it->first == k) ? it : v.end();
    }
    V& operator[](uint8_t k) {
        auto it = lower(k);
        if (it == v.end() || it->first != k) it = v.insert(it, {k, V{}});
        return it->second;
    }
};

// two cache lines (the row builders prefetch both); the commitment state is in vc_verkle's arrays
struct alignas(64) VNode {
    bool ext = false;
    int level = 0;                                           // internal: depth below the root
    std::array<uint8_t, 32> stem{};                          // extension: the full key (node.rs:45)
    using Leaf = std::pair<uint8_t, std::array<uint8_t, 32>>;
    FlatMap<std::array<uint8_t, 32>, InlineVec<Leaf>> leaves;  // extension: unit -> value
    FlatMap<int> children;                                   // internal: unit -> node
};

// LE bytes -> canonical Fr words (from_le_bytes_mod_order): < 31 bytes is already < r; 32
// bytes (< 2^256 < 6r) by at most five subtractions of r; longer inputs by the generic path
inline void item_of_bytes(const uint8_t* b, size_t len, uint64_t out[4]) {
    if (len <= 32) {
        uint8_t w[32] = {0};
        memcpy(w, b, len);
        memcpy(out, w, 32);
        static const uint64_t R[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL,
                                      0x30644e72e131a029ULL};  // BN254 r
        // v mod r with one quotient estimate: q = floor(v_3 / r_3) (<= 5) is floor(v / r) or one
        // more (r_3 ~ 2^61.6 dwarfs the lower limbs' share), so v - q r lies in [-r, r): one
        // conditional add (the compare-and-subtract loop it replaces mispredicted ~48 ns per stem)
        const uint64_t q = out[3] / R[3];
        typedef unsigned __int128 u128;
        u128 mc = 0, br = 0;
        for (int i = 0; i < 4; i++) {
            mc += (u128)q * R[i];
            const u128 d = (u128)out[i] - (uint64_t)mc - (uint64_t)br;
            out[i] = (uint64_t)d;
            br = (d >> 64) & 1;
            mc >>= 64;
        }
        if ((uint64_t)mc + (uint64_t)br) {  // negative: add r back
            u128 c = 0;
            for (int i = 0; i < 4; i++) {
                c += (u128)out[i] + R[i];
                out[i] = (uint64_t)c;
                c >>= 64;
            }
        }
        return;
    }
    mont_to_canon<BN254Fr>(fe_from_le_bytes_mod<BN254Fr>(b, len), out);
}

// The tree without its results: nodes, per-node flags, dirty lists and the slot log
struct VTrie {
    int N = 3;
    std::vector<VNode> nodes;  // nodes[0] = root (internal)
    // per-node flags (compact: the commitment's bookkeeping touches no node lines)
    std::vector<uint8_t> has_commit, queued;
    // dirty nodes, kept at insert time: every extension, and the internal nodes by level (an insert
    // clears the commitments on its path; new nodes start dirty)
    std::vector<int> dirty_ext;
    std::vector<std::vector<int>> dirty_int;
    // delta updates (verkle_commit_dev.hip): base[id] = the node's stored commitment is its last
    // successful one, and every change of its slots since is in slog as (parent, slot, the child the
    // slot held then: -1 = empty) -- logged at insert time for base parents only
    struct SlotLog {
        int parent, old;
        uint8_t slot;
    };
    std::vector<uint8_t> base;
    std::vector<SlotLog> slog;
    // scratch of the commitment's delta plan (verkle_plan.hpp DeltaPlan), per node id (-1 outside a
    // call): the node's plan / its snapshot index (persistent arrays: no hash maps per call)
    std::vector<int32_t> plan_slot, snap_slot;
    void log_slot(int parent, uint8_t slot, int old) {
        if (base[parent]) slog.push_back({parent, old, slot});
    }
    // (the owner's per-node result arrays grow after an insert: vc_verkle::grow_results)
    int add(VNode&& n) {
        nodes.push_back(std::move(n));
        has_commit.push_back(0);
        queued.push_back(0);
        base.push_back(0);
        plan_slot.push_back(-1);
        snap_slot.push_back(-1);
        return (int)nodes.size() - 1;
    }
    void mark(int id) {  // commitment cleared (node.rs:150-152 commitment = None)
        has_commit[id] = 0;
        if (queued[id]) return;
        queued[id] = 1;
        const VNode& n = nodes[id];
        if (n.ext) {
            dirty_ext.push_back(id);
        } else {
            if ((int)dirty_int.size() <= n.level) dirty_int.resize(n.level + 1);
            dirty_int[n.level].push_back(id);
        }
    }
    size_t dirty_count() const {
        size_t c = dirty_ext.size();
        for (auto& lv : dirty_int) c += lv.size();
        return c;
    }
    void clear_dirty() {  // after a commitment: every listed node is committed
        for (int id : dirty_ext) has_commit[id] = 1, queued[id] = 0, base[id] = 1;
        for (auto& lv : dirty_int)
            for (int id : lv) has_commit[id] = 1, queued[id] = 0, base[id] = 1;
        dirty_ext.clear();
        dirty_int.clear();
        slog.clear();
    }
    // a failed commitment may have stored some dirty nodes' new results already: their stored
    // commitments are no delta bases any more (the retry recommits them in full)
    void drop_delta() {
        for (int id : dirty_ext) base[id] = 0;
        for (auto& lv : dirty_int)
            for (int id : lv) base[id] = 0;
        slog.clear();
    }
};

// an empty tree of key length N: the root is Node::new_internal(vec![]), level 0, dirty
inline void trie_init(VTrie& t, int N) {
    t.N = N;
    t.mark(t.add(VNode()));
}

inline int trie_new_ext(VTrie& t, const uint8_t* stem, uint8_t unit, const uint8_t* value) {
    VNode n;
    n.ext = true;
    memcpy(n.stem.data(), stem, t.N);
    std::array<uint8_t, 32> v;
    memcpy(v.data(), value, 32);
    n.leaves[unit] = v;
    const int id = t.add(std::move(n));
    t.mark(id);
    return id;
}

// first d > cur with a[d] != b[d] (or N) -- KeyMethods::next_diff_depth (lib.rs:49-58)
inline int next_diff_depth(const uint8_t* a, const uint8_t* b, int cur, int N) {
    int d = cur + 1;
    while (d < N && a[d] == b[d]) d++;
    return d;
}

// get_stem (node.rs:74-95)
inline int find_stem(const VTrie& t, const uint8_t* stem) {
    int cur = 0, depth = 0;
    while (true) {
        const VNode& n = t.nodes[cur];
        if (n.ext) return memcmp(n.stem.data(), stem, t.N) == 0 ? cur : -1;
        if (depth >= t.N) return -1;
        auto it = n.children.find(stem[depth]);
        if (it == n.children.end()) return -1;
        cur = it->second;
        depth++;
    }
}

// Node::insert (node.rs:133-204), iteratively. The walk is checked before anything changes,
// so the reference's panic case leaves the tree untouched.
inline int trie_insert(VTrie& t, const uint8_t* key, const uint8_t* value) {
    const int N = t.N;
    const uint8_t* stem = key;       // split(): the stem keeps every unit (lib.rs:61-67)
    const uint8_t unit = key[N - 1];
    // dry run: find where the walk ends and reject the panic case first
    std::vector<int> path;
    int cur = 0, depth = 0;
    enum { INTO_EXT, NEW_EXT, SPLIT } action;
    int parent_k = -1;
    while (true) {
        path.push_back(cur);
        VNode& n = t.nodes[cur];
        if (n.ext) {
            if (memcmp(n.stem.data(), stem, N) != 0) return VC_E_INVALID;  // reference panics here
            action = INTO_EXT;
            break;
        }
        if (depth >= N) return VC_E_INVALID;
        const uint8_t k = stem[depth];
        auto it = n.children.find(k);
        if (it == n.children.end()) {
            action = NEW_EXT;
            parent_k = k;
            break;
        }
        VNode& c = t.nodes[it->second];
        if (c.ext && !(memcmp(c.stem.data(), stem, N) == 0 || depth == N - 2)) {
            // the reference indexes stem[d] out of bounds (panics) when no unit after `depth`
            // differs -- reachable only through its level-skipping splits
            if (next_diff_depth(c.stem.data(), stem, depth, N) >= N) return VC_E_INVALID;
            action = SPLIT;
            parent_k = k;
            break;
        }
        cur = it->second;
        depth++;
    }
    for (int p : path) t.mark(p);  // clear the commitments on the path
    // the path's slots (their children's items change) -- internal path[i] sits at depth i
    for (size_t i = 0; i + 1 < path.size(); i++) t.log_slot(path[i], stem[i], path[i + 1]);
    VNode* n = &t.nodes[cur];
    if (action == INTO_EXT) {
        std::array<uint8_t, 32> v;
        memcpy(v.data(), value, 32);
        n->leaves[unit] = v;
        return VC_OK;
    }
    if (action == NEW_EXT) {
        t.log_slot(cur, (uint8_t)parent_k, -1);
        int e = trie_new_ext(t, stem, unit, value);
        t.nodes[cur].children[(uint8_t)parent_k] = e;
        return VC_OK;
    }
    // SPLIT: new internal keyed by the first differing unit d (which may skip levels, as in
    // the reference: node.rs:176-185)
    const int old = t.nodes[cur].children[(uint8_t)parent_k];
    t.log_slot(cur, (uint8_t)parent_k, old);
    const std::array<uint8_t, 32> old_stem = t.nodes[old].stem;
    const int d = next_diff_depth(old_stem.data(), stem, depth, N);
    int e = trie_new_ext(t, stem, unit, value);
    VNode in;
    in.level = depth + 1;  // a child of `cur` (whose level is the walk depth)
    in.children[stem[d]] = e;
    in.children[old_stem[d]] = old;
    const int id = t.add(std::move(in));
    t.mark(id);
    t.nodes[cur].children[(uint8_t)parent_k] = id;
    return VC_OK;
}

inline bool trie_get(const VTrie& t, const uint8_t* key, uint8_t* value) {
    const int e = find_stem(t, key);
    if (e < 0) return false;
    auto it = t.nodes[e].leaves.find(key[t.N - 1]);
    if (it == t.nodes[e].leaves.end()) return false;
    memcpy(value, it->second.data(), 32);
    return true;
}

// path_to_stem (node.rs:97-120): (prefix, unit) for every internal node down to the
// extension; the prefix is key[0..=depth], so only the units are returned.
inline int trie_path(const VTrie& t, const uint8_t* key, size_t max_len, uint8_t* units, size_t* len) {
    size_t n = 0;
    int cur = 0;
    while (!t.nodes[cur].ext) {
        if ((int)n >= t.N) return VC_E_INVALID;
        auto it = t.nodes[cur].children.find(key[n]);
        if (it == t.nodes[cur].children.end()) return VC_E_INVALID;  // VerkleError::InvalidPath
        if (units && n < max_len) units[n] = key[n];
        n++;
        cur = it->second;
    }
    *len = n;
    return VC_OK;
}

inline void trie_stats(const VTrie& t, size_t* internal, size_t* extension, size_t* dirty) {
    size_t a = 0, b = 0, c = 0;
    for (size_t i = 0; i < t.nodes.size(); i++) {
        (t.nodes[i].ext ? b : a)++;
        if (!t.has_commit[i]) c++;
    }
    if (internal) *internal = a;
    if (extension) *extension = b;
    if (dirty) *dirty = c;
}

// The host commitment path's lists: dirty nodes reachable from the root, the internal ones by
// depth (clean subtrees are skipped: an insert clears every commitment on its path, so a clean
// node has clean descendants). Every rank of a sharded run holds the same tree, so every rank
// walks it to the same lists in the same order.
// The walk of the root's subtrees is split over the host pool (contiguous ranges of the root's
// children; the per-worker lists are concatenated in worker order, so the lists -- and a sharded
// run's slices -- are the same on every rank).
inline void collect_dirty(const VTrie& t, HostPool& P, std::vector<int>& exts, std::vector<std::vector<int>>& internals) {
    auto walk = [&](int root, int depth0, std::vector<int>& ex, std::vector<std::vector<int>>& in) {
        std::vector<std::pair<int, int>> stack{{root, depth0}};
        while (!stack.empty()) {
            auto [id, depth] = stack.back();
            stack.pop_back();
            const VNode& n = t.nodes[id];
            if (t.has_commit[id]) continue;
            if (n.ext) {
                ex.push_back(id);
                continue;
            }
            if ((int)in.size() <= depth) in.resize(depth + 1);
            in[depth].push_back(id);
            for (auto& kv : n.children) {  // (popped in reverse: fetch their lines meanwhile)
                __builtin_prefetch(&t.nodes[kv.second]);
                stack.push_back({kv.second, depth + 1});
            }
        }
    };
    const VNode& root = t.nodes[0];
    // (the branch depends only on the tree, never on this host's core count: ranks of a
    // sharded run with different pool sizes must produce the same lists; a one-thread pool
    // runs the same per-child walk serially)
    if (t.has_commit[0] || root.ext || root.children.v.size() < 2 || t.nodes.size() < 4096) {
        walk(0, 0, exts, internals);
        return;
    }
    internals.resize(1);
    internals[0].push_back(0);
    const auto& ch = root.children.v;
    const unsigned T = P.size();
    std::vector<std::vector<int>> ex(T);
    std::vector<std::vector<std::vector<int>>> in(T);
    auto part = [&](unsigned k) {
        for (size_t c = ch.size() * k / T; c < ch.size() * (k + 1) / T; c++) walk(ch[c].second, 1, ex[k], in[k]);
    };
    if (T == 1) part(0);
    else P.run(part);
    for (unsigned k = 0; k < T; k++) {
        exts.insert(exts.end(), ex[k].begin(), ex[k].end());
        if (internals.size() < in[k].size()) internals.resize(in[k].size());
        for (size_t d = 0; d < in[k].size(); d++)
            internals[d].insert(internals[d].end(), in[k][d].begin(), in[k][d].end());
    }
}

}  // namespace vk

// Row builders of the verkle commitment paths: sparse rows of (column, value) non-zeros built from
// the trie on the host pool, the extension nodes' c1 / c2 rows (node.rs:216-244) in the host path's
// and the device path's value widths, and the device path's extension host stage. Host only.
#pragma once
#include <chrono>
#include <functional>

#include "verkle_trie.hpp"

namespace vk {

// batched sparse commits (vc_msm_batch_sparse): rows of (column, value) non-zeros
struct Rows {
    uvec<uint64_t> ptr{0};
    uvec<uint32_t> cols;
    uvec<uint64_t> vals;
    void clear() {  // (capacity kept)
        ptr.assign(1, 0);
        cols.clear();
        vals.clear();
    }
    void reserve(size_t rows, size_t nnz) {
        ptr.reserve(rows + 1);
        cols.reserve(nnz);
        vals.reserve(4 * nnz);
    }
    void add(uint32_t col, const uint64_t* v) {
        if (!(v[0] | v[1] | v[2] | v[3])) return;  // zero scalars contribute nothing
        cols.push_back(col);
        vals.insert(vals.end(), v, v + 4);
    }
    void end_row() { ptr.push_back(cols.size()); }
    size_t n() const { return ptr.size() - 1; }
};

// rows of items [lo, hi) built by fn(i, R&) on the host pool, in item order, as per-worker parts
// (the node walks are pointer-chasing code: ~100-200 ns per node on one thread); one part when the
// range is small. pf(i, stage): software prefetch of item i's node data ahead of the walk (stage 0
// at 16 items ahead: the node; stage 1 at 8 ahead: what the node points to, its line now cached) --
// the walks are chains of dependent DRAM misses (~360 ns per extension node on 16 threads).
// nnz_per: the non-zeros expected per item (the thread-count rule's work estimate), nnz_res: those
// reserved per item.
// reuse (optional): parts of an earlier call, cleared and refilled -- their storage stays
// allocated (a fresh 65,536-extension level's part vectors cost ~0.1 ms of page faults per worker)
template <class R, class Fn, class Pf>
std::vector<R> build_parts(HostPool& pool, size_t lo, size_t hi, size_t nnz_per, size_t nnz_res, Fn fn, Pf pf,
                           std::vector<R>* reuse = nullptr) {
    const size_t count = hi - lo;
    auto walk_range = [&](size_t a, size_t b, R& r) {
        for (size_t i = a; i < std::min(b, a + 16); i++) pf(i, 0);
        for (size_t i = a; i < std::min(b, a + 8); i++) pf(i, 1);
        for (size_t i = a; i < b; i++) {
            if (i + 16 < b) pf(i + 16, 0);
            if (i + 8 < b) pf(i + 8, 1);
            fn(i, r);
        }
    };
    // by work, not rows: the 256 depth-1 nodes of a 65,536-key tree hold ~41K children (a
    // serial walk of their maps took 0.84 ms: profiles/r04/verkle/laps_before.txt)
    const unsigned T = (count >= 64 && count * nnz_per >= 16384)
                           ? (unsigned)std::min<size_t>(pool.size(), std::max<size_t>(1, count / 16))
                           : 1;
    std::vector<R> part;
    if (reuse) part.swap(*reuse);
    part.resize(T);
    auto run = [&](unsigned k) {  // the pool runs k < pool.size(): workers past T have no part
        if (k >= T) return;
        const size_t a = lo + count * k / T, b = lo + count * (k + 1) / T;
        // filled in a local object: the parts' vector headers share cache lines, and every
        // push_back updates its header (false sharing made 8 threads 1.6x one)
        R local = std::move(part[k]);
        local.clear();
        local.reserve(b - a, (b - a) * nnz_res);
        walk_range(a, b, local);
        part[k] = std::move(local);
    };
    if (T == 1) run(0);
    else pool.run(run);
    return part;
}

// the parts merged into one Rows (copied into place in parallel)
template <class Fn, class Pf>
Rows build_rows(HostPool& pool, size_t lo, size_t hi, size_t nnz_per, Fn fn, Pf pf) {
    std::vector<Rows> part = build_parts<Rows>(pool, lo, hi, nnz_per, nnz_per, fn, pf);
    const size_t T = part.size();
    if (T == 1) return std::move(part[0]);
    Rows out;
    std::vector<size_t> roff(T + 1, 0), noff(T + 1, 0);
    for (size_t k = 0; k < T; k++) {
        roff[k + 1] = roff[k] + part[k].n();
        noff[k + 1] = noff[k] + part[k].cols.size();
    }
    out.ptr.resize(roff[T] + 1);
    out.ptr[0] = 0;
    out.cols.resize(noff[T]);
    out.vals.resize(4 * noff[T]);
    pool.run([&](unsigned k) {
        if (k >= T) return;
        const Rows& r = part[k];
        for (size_t i = 1; i < r.ptr.size(); i++) out.ptr[roff[k] + i] = noff[k] + r.ptr[i];
        if (!r.cols.empty()) {
            memcpy(&out.cols[noff[k]], r.cols.data(), r.cols.size() * 4);
            memcpy(&out.vals[4 * noff[k]], r.vals.data(), r.vals.size() * 8);
        }
    });
    return out;
}

// The c1 / c2 slots of an extension node (node.rs:216-244): every leaf's 16-byte halves at
// positions (2 index) % N, (2 index + 1) % N of c1 (index < N / 2) or c2, in leaf order; a later
// write to the same position overwrites, as c1_values[index] = ... does. W: u64 words per value;
// val(half's 16 bytes, v[W]) writes the value into its slot. Positions < N <= 32: fixed slots, no allocation.
template <int W>
struct ExtSlots {
    struct PV {
        uint32_t pos;
        uint64_t v[W];
    };
    PV half[2][32];
    int cnt[2] = {0, 0};
    uint64_t* slot(int h, uint32_t pos) {  // the value at `pos` of half h (a new slot if none yet)
        int k = 0;
        while (k < cnt[h] && half[h][k].pos != pos) k++;
        if (k == cnt[h]) half[h][cnt[h]++].pos = pos;
        return half[h][k].v;
    }
    template <class Val>
    ExtSlots(const VNode& n, int N, Val val) {
        for (auto& kv : n.leaves) {
            const size_t index = kv.first;
            const int h = index < (size_t)(N / 2) ? 0 : 1;
            val(kv.second.data(), slot(h, (uint32_t)((2 * index) % N)));
            val(kv.second.data() + 16, slot(h, (uint32_t)((2 * index + 1) % N)));
        }
    }
};

// the host path's c1 / c2 rows of extension node `id`: canonical Fr values
inline void ext_rows(const VTrie& t, int id, Rows& r) {
    const ExtSlots<4> s(t.nodes[id], t.N, [](const uint8_t* b16, uint64_t* v) { item_of_bytes(b16, 16, v); });
    for (int h = 0; h < 2; h++) {
        for (int k = 0; k < s.cnt[h]; k++) r.add(s.half[h][k].pos, s.half[h][k].v);
        r.end_row();
    }
}
// the device path's extension rows: c1 / c2 as ext_rows, but with 16-byte values (a leaf half is
// below 2^128: the device widens them) and the node's raw stem bytes (the device reduces them mod r);
// stem[] is indexed by the row pair
struct ExtRows16 {
    uvec<uint64_t> ptr{0};
    uvec<uint32_t> cols;
    uvec<uint64_t> vals;  // 2 u64 per non-zero
    uvec<uint64_t> stem;  // 4 u64 per extension node (its raw stem bytes, LE)
    uint32_t maxlen = 0;  // longest row (<= 4: the sparse commit's chunks are the rows)
    void clear() {  // (capacity kept)
        ptr.assign(1, 0);
        cols.clear();
        vals.clear();
        stem.clear();
        maxlen = 0;
    }
    void reserve(size_t rows, size_t nnz) {
        ptr.reserve(2 * rows + 1);
        cols.reserve(nnz);
        vals.reserve(2 * nnz);
        stem.reserve(4 * rows);
    }
    size_t n() const { return ptr.size() - 1; }
};
inline void ext_rows16(const VTrie& t, int id, ExtRows16& r) {
    const VNode& n = t.nodes[id];
    const ExtSlots<2> s(n, t.N, [](const uint8_t* b16, uint64_t* v) { memcpy(v, b16, 16); });
    for (int h = 0; h < 2; h++) {
        for (int k = 0; k < s.cnt[h]; k++) {
            const uint64_t* v = s.half[h][k].v;
            if (!(v[0] | v[1])) continue;  // zero scalars contribute nothing
            r.cols.push_back(s.half[h][k].pos);
            r.vals.push_back(v[0]);
            r.vals.push_back(v[1]);
        }
        r.maxlen = std::max<uint32_t>(r.maxlen, (uint32_t)(r.cols.size() - r.ptr.back()));
        r.ptr.push_back(r.cols.size());
    }
    // the stem's raw LE bytes (zero beyond N): k_vk_ext_rows4 reduces them mod r on the device
    // (bytes_to_item(stem.to_bytes()), node.rs:248-250 -> lagrange_basis.rs:175-176) -- the host's
    // one-quotient reduction was ~35 % of this stage's single-thread time (profiles/r05/verkle/)
    r.stem.resize(r.stem.size() + 4);
    memcpy(r.stem.data() + r.stem.size() - 4, n.stem.data(), 32);
}

inline void ext_prefetch(const VTrie& t, int id, int stage) {
    const VNode& n = t.nodes[id];
    if (stage == 0) {
        __builtin_prefetch(&n);
        __builtin_prefetch(reinterpret_cast<const char*>(&n) + 64);
    } else if (!n.leaves.v.empty()) {
        __builtin_prefetch(n.leaves.v.data());
    }
}

// The extension level's host stage of the device path: c1 / c2 rows built in per-worker parts
// (with each node's raw stem bytes, reduced on the device), then merged in parallel straight into one
// buffer (page-locked in the commitment: the upload is plain DMA) laid out as row_ptr (2E + 1 u64) |
// stems (E x 32 B) |
// values (nnz x 2 u64) | node ids (E u32) | cols (nnz u32) -- everything after row_ptr goes up in one
// copy. `cache`: part storage kept between calls (no page faults on fresh vectors).
struct ExtStage {
    size_t nnz = 0, o_stem = 0, o_vals = 0, o_ids = 0, o_cols = 0, o_end = 0;
    uint32_t maxlen = 0;
    uint8_t* base = nullptr;
};
inline int ext_stage(const VTrie& t, const std::vector<int>& exts, HostPool& pool, std::vector<ExtRows16>& cache,
                     const std::function<uint8_t*(size_t)>& buffer, ExtStage* out, double* t_build = nullptr) {
    const size_t E = exts.size();
    const auto tb0 = std::chrono::steady_clock::now();
    std::vector<ExtRows16> parts = build_parts<ExtRows16>(
        pool, 0, E, (size_t)t.N, std::min<size_t>((size_t)t.N, 4), [&](size_t e, ExtRows16& r) { ext_rows16(t, exts[e], r); },
        [&](size_t e, int stage) { ext_prefetch(t, exts[e], stage); }, &cache);
    struct KeepParts {
        std::vector<ExtRows16>& p;
        std::vector<ExtRows16>& cache;
        ~KeepParts() { cache.swap(p); }
    } keep_parts{parts, cache};
    if (t_build) *t_build = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tb0).count();
    const size_t T = parts.size();
    std::vector<size_t> roff(T + 1, 0), noff(T + 1, 0), eoff(T + 1, 0);
    uint32_t maxlen = 0;
    for (size_t k = 0; k < T; k++) {
        roff[k + 1] = roff[k] + parts[k].n();
        noff[k + 1] = noff[k] + parts[k].cols.size();
        eoff[k + 1] = eoff[k] + parts[k].stem.size() / 4;
        maxlen = std::max(maxlen, parts[k].maxlen);
    }
    const size_t nnz = noff[T];
    ExtStage& X = *out;
    X.nnz = nnz;
    X.maxlen = maxlen;
    X.o_stem = (2 * E + 1) * 8;
    X.o_vals = X.o_stem + E * 32;
    X.o_ids = X.o_vals + nnz * 16;
    X.o_cols = X.o_ids + E * 4;
    X.o_end = X.o_cols + nnz * 4;
    uint8_t* pin = buffer(X.o_end);
    if (!pin) return VC_E_OOM;
    X.base = pin;
    uint64_t* rp = reinterpret_cast<uint64_t*>(pin);
    uint32_t* ids = reinterpret_cast<uint32_t*>(pin + X.o_ids);
    rp[0] = 0;
    auto merge = [&](unsigned k) {  // part k holds extensions [eoff[k], eoff[k + 1]) in order
        if (k >= T) return;
        const ExtRows16& r = parts[k];
        for (size_t i = 1; i < r.ptr.size(); i++) rp[roff[k] + i] = noff[k] + r.ptr[i];
        if (!r.stem.empty()) memcpy(pin + X.o_stem + eoff[k] * 32, r.stem.data(), r.stem.size() * 8);
        if (!r.cols.empty()) {
            memcpy(pin + X.o_vals + noff[k] * 16, r.vals.data(), r.vals.size() * 8);
            memcpy(pin + X.o_cols + noff[k] * 4, r.cols.data(), r.cols.size() * 4);
        }
        for (size_t e = eoff[k]; e < eoff[k + 1]; e++) ids[e] = (uint32_t)exts[e];
    };
    if (T == 1) merge(0);
    else pool.run(merge);
    return VC_OK;
}

}  // namespace vk

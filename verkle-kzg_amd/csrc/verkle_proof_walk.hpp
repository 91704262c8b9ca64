// Verkle tree proofs (include/vc_verkle.h): the host walk of the keys -- the query list as
// references to nodes, the nodes touched, the extensions proven. Nothing here needs a commitment,
// so vc_verkle_proof_size is this walk alone. Host only (the trie and ext_rows).
#pragma once
#include "verkle_rows.hpp"

namespace vk {

struct ProofWalk {
    // a query's commitment: kind 0 = node touched[ref], kind 1 = C_half number ref (2 ext + half - 1);
    // its y: 0 = the item of node touched[yref], 1 = one, 2 = the stem item of extension yref,
    // 3 = the item of C_half yref, 4 = the 16-byte literal leaf[yref]
    struct Query {
        uint8_t kind, ykind, z;
        uint32_t ref, yref;
    };
    std::vector<int> touched;  // node ids in first-occurrence order (touched[0] = the root)
    std::vector<int> exts;     // the proven extensions' node ids
    std::vector<uint32_t> ext_touched;  // and their indices in touched
    Rows hrows;  // their c1 / c2 rows (ext_rows: canonical values, zeros left out): rows 2 e, 2 e + 1
    std::vector<Query> queries;
    std::vector<std::pair<uint8_t, uint32_t>> coms;  // the proof's commitments as (kind, ref)
    std::vector<uint8_t> depth;
    std::vector<std::array<uint64_t, 2>> leaf;
};

// the value row `h` of `rows` holds at `col` (null: zero)
inline const uint64_t* row_value(const Rows& rows, size_t h, uint32_t col) {
    for (uint64_t e = rows.ptr[h]; e < rows.ptr[h + 1]; e++)
        if (rows.cols[e] == col) return &rows.vals[4 * e];
    return nullptr;
}

inline int proof_walk(const VTrie& t, const uint8_t* keys, size_t n, ProofWalk& W) {
    const int N = t.N;
    std::vector<int32_t> tidx(t.nodes.size(), -1), eidx(t.nodes.size(), -1);  // node id -> index in touched / exts
    std::vector<std::array<uint64_t, 4>> seen_n, seen_h;  // the z emitted per touched node / C_half
    std::vector<uint8_t> half_in;                          // C_half already among the commitments
    auto touch = [&](int id) -> uint32_t {
        if (tidx[id] >= 0) return (uint32_t)tidx[id];
        const uint32_t k = (uint32_t)W.touched.size();
        tidx[id] = (int32_t)k;
        W.touched.push_back(id);
        seen_n.push_back({0, 0, 0, 0});
        if (id != 0) W.coms.emplace_back((uint8_t)0, k);
        return k;
    };
    auto emit = [&](uint8_t kind, uint32_t ref, uint32_t z, uint8_t ykind, uint32_t yref) {
        auto& s = (kind ? seen_h : seen_n)[ref];
        if ((s[z >> 6] >> (z & 63)) & 1) return;
        s[z >> 6] |= 1ull << (z & 63);
        W.queries.push_back({kind, ykind, (uint8_t)z, ref, yref});
    };
    W.depth.resize(n);
    std::vector<int> path;
    for (size_t i = 0; i < n; i++) {
        const uint8_t* K = keys + i * (size_t)N;
        path.clear();
        int cur = 0;
        while (!t.nodes[cur].ext) {
            const size_t j = path.size();
            if ((int)j >= N - 1) return VC_E_INVALID;
            auto it = t.nodes[cur].children.find(K[j]);
            if (it == t.nodes[cur].children.end()) return VC_E_INVALID;
            path.push_back(cur);
            cur = it->second;
        }
        const VNode& E = t.nodes[cur];
        const uint8_t u = K[N - 1];
        auto lf = E.leaves.find(u);
        if (path.empty() || memcmp(E.stem.data(), K, N) != 0 || lf == E.leaves.end()) return VC_E_INVALID;
        const size_t d = path.size();
        W.depth[i] = (uint8_t)d;
        uint32_t ti[33];  // d <= N - 1 <= 31
        for (size_t j = 0; j < d; j++) ti[j] = touch(path[j]);
        ti[d] = touch(cur);
        if (eidx[cur] < 0) {
            eidx[cur] = (int32_t)W.exts.size();
            W.exts.push_back(cur);
            W.ext_touched.push_back(ti[d]);
            ext_rows(t, cur, W.hrows);
            seen_h.push_back({0, 0, 0, 0});
            seen_h.push_back({0, 0, 0, 0});
            half_in.push_back(0);
            half_in.push_back(0);
        }
        const uint32_t e = (uint32_t)eidx[cur];
        const int h = u < (uint8_t)(N / 2) ? 0 : 1;  // row of `rows`; half = h + 1
        const uint32_t hid = 2 * e + (uint32_t)h;
        if (!half_in[hid]) {
            half_in[hid] = 1;
            W.coms.emplace_back((uint8_t)1, hid);
        }
        // the row must hold this leaf's halves at its two slots (the % N folding can alias slots)
        uint64_t lo[2], hi[2];
        memcpy(lo, lf->second.data(), 16);
        memcpy(hi, lf->second.data() + 16, 16);
        const uint32_t zl = (uint32_t)((2 * (size_t)u) % N), zh = (uint32_t)((2 * (size_t)u + 1) % N);
        auto holds = [&](uint32_t col, const uint64_t* v) {
            const uint64_t* r = row_value(W.hrows, hid, col);
            return r ? (r[0] == v[0] && r[1] == v[1] && !(r[2] | r[3])) : !(v[0] | v[1]);
        };
        if (!holds(zl, lo) || !holds(zh, hi)) return VC_E_INVALID;
        for (size_t j = 0; j < d; j++) emit(0, ti[j], K[j], 0, ti[j + 1]);
        emit(0, ti[d], 0, 1, 0);
        emit(0, ti[d], 1, 2, e);
        emit(0, ti[d], 2 + (uint32_t)h, 3, hid);
        W.leaf.push_back({lo[0], lo[1]});
        emit(1, hid, zl, 4, (uint32_t)W.leaf.size() - 1);
        W.leaf.push_back({hi[0], hi[1]});
        emit(1, hid, zh, 4, (uint32_t)W.leaf.size() - 1);
    }
    return VC_OK;
}

}  // namespace vk

// Verkle tree proofs (include/vc_verkle.h): the keys' walk (verkle_proof_walk.hpp) turned into one
// multiproof over the touched nodes' rows -- the nodes' commitments and items gathered out of the
// device mirror, the proven extensions' c1 / c2 commitments made here -- and the verifier, which
// rebuilds the query list from the keys, values, depths and the proof's commitments.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "scheme_internal.hpp"
#include "verkle_internal.hpp"
#include "verkle_proof_walk.hpp"

namespace vk {

// the c1 / c2 commitments and items of the proven extensions (they are not kept in the mirror): one
// batched sparse commit of 2 E rows, results on the host (the proof carries them)
static int proof_halves(vc_ctx* ctx, int table, const ProofWalk& W, std::vector<uint64_t>& hxy, std::vector<uint8_t>& hinf,
                        std::vector<uint64_t>& hitem) {
    const size_t E = W.exts.size();
    const Rows& all = W.hrows;
    hxy.assign(2 * E * 8, 0);
    hinf.assign(2 * E, 1);
    hitem.assign(2 * E * 4, 0);
    if (all.cols.empty()) {  // every opened value is zero: identities
        for (size_t k = 0; k < 2 * E; k++) mont_to_canon<BN254Fr>(to_data_item_host(&hxy[8 * k], true), &hitem[4 * k]);
        return VC_OK;
    }
    return msm_batch_sparse_items_guarded(ctx, table, 2 * E, all.ptr.data(), all.cols.data(), all.vals.data(), hxy.data(),
                                          hinf.data(), hitem.data());
}

// (commitment, z, y) of every query; node(k) = (xy, inf, item) of touched node k
struct NodeRec {
    const uint64_t* xy;
    uint8_t inf;
    const uint64_t* item;
};
template <class NodeFn>
static void proof_queries_fill(const vc_verkle* t, const ProofWalk& W, NodeFn node, const uint64_t* hxy,
                               const uint8_t* hinf, const uint64_t* hitem, uint64_t* com_xy, uint8_t* com_inf,
                               uint64_t* z, uint64_t* y) {
    for (size_t q = 0; q < W.queries.size(); q++) {
        const ProofWalk::Query& Qy = W.queries[q];
        if (Qy.kind == 0) {
            const NodeRec r = node(Qy.ref);
            memcpy(com_xy + 8 * q, r.xy, 64);
            com_inf[q] = r.inf;
        } else {
            memcpy(com_xy + 8 * q, hxy + 8 * (size_t)Qy.ref, 64);
            com_inf[q] = hinf[Qy.ref];
        }
        if (com_inf[q]) memset(com_xy + 8 * q, 0, 64);
        z[q] = Qy.z;
        uint64_t* o = y + 4 * q;
        o[0] = o[1] = o[2] = o[3] = 0;
        switch (Qy.ykind) {
            case 0: memcpy(o, node(Qy.yref).item, 32); break;
            case 1: o[0] = 1; break;
            case 2: item_of_bytes(t->nodes[W.exts[Qy.yref]].stem.data(), (size_t)t->N, o); break;
            case 3: memcpy(o, hitem + 4 * (size_t)Qy.yref, 32); break;
            default: memcpy(o, W.leaf[Qy.yref].data(), 16); break;
        }
    }
}

// the touched nodes' records out of the mirror: rec[j] = commitment (8 u64) | item (4) | flag (1)
constexpr size_t PROOF_REC = VK_NODE_REC;
__global__ void k_vk_gather_nodes(const uint64_t* __restrict__ cxy, const uint64_t* __restrict__ item,
                                  const uint8_t* __restrict__ inf, const uint32_t* __restrict__ ids, size_t n,
                                  uint64_t* __restrict__ rec) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const size_t id = ids[j];
    uint64_t* o = rec + PROOF_REC * j;
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = cxy[8 * id + k];
#pragma unroll
    for (int k = 0; k < 4; k++) o[8 + k] = item[4 * id + k];
    o[12] = inf[id];
}

static int proof_table_ok(vc_ctx* ctx, int scheme, int table) {
    if (scheme != 0 && scheme != 1) return VC_E_TABLE;  // (no scheme this table could serve)
    Table* tab = ctx->table(table);
    if (!tab || tab->curve != VC_CURVE_BN254 || tab->n != (scheme == 0 ? 257u : 256u)) return VC_E_TABLE;
    return VC_OK;
}

static int verkle_prove(vc_ctx* ctx, int scheme, int table, vc_verkle* t, const uint8_t* keys, size_t n, uint64_t* root_xy,
                 uint8_t* root_inf, vc_verkle_proof* out) {
    Guard guard(ctx);
    VK_TRY(proof_table_ok(ctx, scheme, table));
    auto tic = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {  // (host laps; the GPU work is synchronised where the code waits anyway)
        if (!verbose()) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[verkle-prove] %s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - tic).count());
        tic = now;
    };
    ProofWalk W;
    VK_TRY(proof_walk(*t, keys, n, W));
    if (out->n_keys != n || out->n_com < W.coms.size()) return VC_E_INVALID;
    lap("walk");
    if (t->dirty_count()) {
        uint64_t rxy[8];
        uint8_t rinf;
        VK_TRY(vc_verkle_commitment(ctx, table, t, rxy, &rinf));
    }
    VK_TRY(mirror_prepare(ctx, t));
    const VerkleDev& D = t->dev;
    hipStream_t st = ctx->stream;
    const size_t T = W.touched.size(), Q = W.queries.size();
    // the touched nodes' commitments, flags and items in one launch and one copy
    std::vector<uint32_t> ids(W.touched.begin(), W.touched.end());
    for (uint32_t id : ids)
        if (id >= D.cap) return VC_E_INVALID;
    DevBuf d_ids(ctx), d_rec(ctx);
    VK_TRY(d_ids.ensure(T * 4));
    VK_TRY(d_rec.ensure(T * PROOF_REC * 8));
    std::vector<uint64_t> rec(T * PROOF_REC);
    VK_CHECK_HIP(hipMemcpyAsync(d_ids.p, ids.data(), T * 4, hipMemcpyHostToDevice, st));
    VK_LAUNCH(ctx, "verkle_gather_nodes", k_vk_gather_nodes, (unsigned)((T + 255) / 256), 256, 0,
              static_cast<const uint64_t*>(D.cxy), static_cast<const uint64_t*>(D.item), static_cast<const uint8_t*>(D.inf),
              d_ids.as<uint32_t>(), T, d_rec.as<uint64_t>());
    VK_CHECK_HIP(hipMemcpyAsync(rec.data(), d_rec.p, T * PROOF_REC * 8, hipMemcpyDeviceToHost, st));
    // (the half commits below end with a stream wait: the records are on the host after them)
    std::vector<uint64_t> hxy, hitem;
    std::vector<uint8_t> hinf;
    const int hs = proof_halves(ctx, table, W, hxy, hinf, hitem);
    VK_CHECK_HIP(hipStreamSynchronize(st));
    VK_TRY(hs);
    lap("mirror, node gather, half commits");
    std::vector<uint64_t> qxy(Q * 8), qz(Q), qy(Q * 4);
    std::vector<uint8_t> qinf(Q);
    proof_queries_fill(t, W, [&](uint32_t k) { return NodeRec{&rec[PROOF_REC * k], (uint8_t)rec[PROOF_REC * k + 12], &rec[PROOF_REC * k + 8]}; },
                       hxy.data(), hinf.data(), hitem.data(), qxy.data(), qinf.data(), qz.data(), qy.data());
    // the distinct rows opened, as (column, source) lists in column order: touched node k's is row k
    // -- an internal node's non-zeros are its children's items in the mirror, an extension's are
    // [1, stem item, item(c1), item(c2)] -- and C_half h's is row T + h, its leaf halves; the values the
    // mirror does not hold are literals (aux)
    const size_t E = W.exts.size(), R = T + 2 * E;
    std::vector<int32_t> ext_of(T, -1);
    for (size_t e = 0; e < E; e++) ext_of[W.ext_touched[e]] = (int32_t)e;
    std::vector<uint64_t> aux(4 + 12 * E + W.hrows.vals.size());
    aux[0] = 1, aux[1] = aux[2] = aux[3] = 0;
    const uint32_t aux_half = (uint32_t)(1 + 3 * E);  // then the half rows' values, as in hrows
    if (!W.hrows.vals.empty()) memcpy(&aux[4 * (size_t)aux_half], W.hrows.vals.data(), W.hrows.vals.size() * 8);
    std::vector<uint32_t> rptr(R + 1), rcol, rsrc;
    size_t kids = 0;
    for (int id : W.touched) kids += t->nodes[id].ext ? 4 : t->nodes[id].children.v.size();
    rcol.reserve(kids + W.hrows.cols.size());
    rsrc.reserve(kids + W.hrows.cols.size());
    for (size_t k = 0; k < T; k++) {
        rptr[k] = (uint32_t)rcol.size();
        const VNode& nd = t->nodes[W.touched[k]];
        if (!nd.ext) {
            for (auto& kv : nd.children.v) {  // (sorted by unit)
                rcol.push_back(kv.first);
                rsrc.push_back((uint32_t)kv.second);
            }
            continue;
        }
        const size_t e = (size_t)ext_of[k];
        uint64_t* a = &aux[4 * (1 + 3 * e)];
        item_of_bytes(nd.stem.data(), (size_t)t->N, a);
        memcpy(a + 4, &hitem[8 * e], 64);
        for (uint32_t c = 0; c < 4; c++) {
            rcol.push_back(c);
            rsrc.push_back(MP_SRC_AUX | (c ? (uint32_t)(3 * e + c) : 0u));
        }
    }
    for (size_t h = 0; h < 2 * E; h++) {
        rptr[T + h] = (uint32_t)rcol.size();
        std::pair<uint32_t, uint32_t> cs[32];  // (column, source): a row has at most N <= 32 non-zeros
        size_t m = 0;
        for (uint64_t k = W.hrows.ptr[h]; k < W.hrows.ptr[h + 1]; k++) cs[m++] = {W.hrows.cols[k], MP_SRC_AUX | (aux_half + (uint32_t)k)};
        std::sort(cs, cs + m);
        for (size_t k = 0; k < m; k++) {
            rcol.push_back(cs[k].first);
            rsrc.push_back(cs[k].second);
        }
    }
    rptr[R] = (uint32_t)rcol.size();
    std::vector<uint32_t> qrow(Q);
    for (size_t q = 0; q < Q; q++) qrow[q] = W.queries[q].kind ? (uint32_t)(T + W.queries[q].ref) : W.queries[q].ref;
    lap("queries, literals, rows");
    MpSparse sp;
    sp.n_rows = R;
    sp.row_ptr = rptr.data();
    sp.col = rcol.data();
    sp.src = rsrc.data();
    sp.q_row = qrow.data();
    sp.d_item = static_cast<const uint64_t*>(D.item);
    sp.n_item = std::min(t->nodes.size(), D.cap);
    sp.aux = aux.data();
    sp.n_aux = aux.size() / 4;
    uint64_t dxy[8], kxy[8], ky[4];
    uint8_t dinf = 1, kinf = 1;
    VK_TRY(mp_prove_sparse(ctx, scheme, table, 256, Q, qxy.data(), qinf.data(), qz.data(), qy.data(), sp, dxy, &dinf,
                           scheme == 0 ? &out->ipa : nullptr, kxy, &kinf, ky));
    lap("multiproof (transcript | plan, sums, finish)");
    memcpy(root_xy, &rec[0], 64);  // touched[0] is the root
    *root_inf = (uint8_t)rec[12];
    if (*root_inf) memset(root_xy, 0, 64);
    memcpy(out->depth, W.depth.data(), n);
    out->n_com = W.coms.size();
    for (size_t k = 0; k < W.coms.size(); k++) {
        const auto& c = W.coms[k];
        const uint64_t* xy = c.first ? &hxy[8 * (size_t)c.second] : &rec[PROOF_REC * c.second];
        out->com_inf[k] = c.first ? hinf[c.second] : (uint8_t)rec[PROOF_REC * c.second + 12];
        if (out->com_inf[k]) memset(out->com_xy + 8 * k, 0, 64);
        else memcpy(out->com_xy + 8 * k, xy, 64);
    }
    memcpy(out->d_xy, dxy, 64);
    out->d_inf = dinf;
    if (scheme == 1) {
        memcpy(out->kzg_proof_xy, kxy, 64);
        out->kzg_proof_inf = kinf;
        memcpy(out->kzg_y, ky, 32);
    }
    return VC_OK;
}

// the diagnostic's query list and dense rows, from the tree's host arrays
static int verkle_proof_queries(vc_ctx* ctx, int table, vc_verkle* t, const uint8_t* keys, size_t n, size_t max_q,
                         uint64_t* com_xy, uint8_t* com_inf, uint64_t* z, uint64_t* y, uint64_t* rows, size_t* Qout) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    VK_CHECK_HIP(hipSetDevice(ctx->device));
    ProofWalk W;
    VK_TRY(proof_walk(*t, keys, n, W));
    const size_t Q = W.queries.size();
    *Qout = Q;
    if (Q > max_q) return VC_E_RANGE;
    if (t->dirty_count()) {
        uint64_t rxy[8];
        uint8_t rinf;
        VK_TRY(vc_verkle_commitment(ctx, table, t, rxy, &rinf));
    }
    VK_TRY(verkle_pull_host(t));
    std::vector<uint64_t> hxy, hitem;
    std::vector<uint8_t> hinf;
    VK_TRY(proof_halves(ctx, table, W, hxy, hinf, hitem));
    proof_queries_fill(t, W, [&](uint32_t k) {
        const size_t id = (size_t)W.touched[k];
        return NodeRec{&t->cxy[8 * id], t->cinf[id], &t->item[4 * id]};
    }, hxy.data(), hinf.data(), hitem.data(), com_xy, com_inf, z, y);
    if (!rows) return VC_OK;
    std::vector<int32_t> ext_of(W.touched.size(), -1);
    for (size_t e = 0; e < W.exts.size(); e++) ext_of[W.ext_touched[e]] = (int32_t)e;
    memset(rows, 0, Q * 256 * 32);
    for (size_t q = 0; q < Q; q++) {
        const ProofWalk::Query& Qy = W.queries[q];
        uint64_t* row = rows + q * 256 * 4;
        if (Qy.kind == 1) {
            const Rows& r = W.hrows;
            for (uint64_t k = r.ptr[Qy.ref]; k < r.ptr[Qy.ref + 1]; k++) memcpy(row + 4 * (size_t)r.cols[k], &r.vals[4 * k], 32);
            continue;
        }
        const VNode& nd = t->nodes[W.touched[Qy.ref]];
        if (!nd.ext) {
            for (auto& kv : nd.children.v) memcpy(row + 4 * (size_t)kv.first, &t->item[4 * (size_t)kv.second], 32);
            continue;
        }
        row[0] = 1;
        item_of_bytes(nd.stem.data(), (size_t)t->N, row + 4);
        memcpy(row + 8, &hitem[8 * (size_t)ext_of[Qy.ref]], 64);
    }
    return VC_OK;
}

static int verkle_proof_size(const vc_verkle* t, const uint8_t* keys, size_t n, size_t* n_com, size_t* n_queries) {
    ProofWalk W;
    VK_TRY(proof_walk(*t, keys, n, W));
    *n_com = W.coms.size();
    *n_queries = W.queries.size();
    return VC_OK;
}

}  // namespace vk

extern "C" {

int vc_verkle_proof_size(const vc_verkle* t, const uint8_t* keys, size_t n, size_t* n_com, size_t* n_queries) {
    if (!t || !keys || n == 0 || !n_com || !n_queries) return VC_E_INVALID;
    return vk::verkle_proof_size(t, keys, n, n_com, n_queries);
}

int vc_verkle_prove(vc_ctx* ctx, int scheme, int table, vc_verkle* t, const uint8_t* keys, size_t n, uint64_t* root_xy,
                    uint8_t* root_inf, vc_verkle_proof* out) {
    if (!ctx || !t || !keys || n == 0 || !root_xy || !root_inf || !out || !out->depth || !out->com_xy || !out->com_inf ||
        ctx->curve != VC_CURVE_BN254)
        return VC_E_INVALID;
    if (scheme == 0 && (out->ipa.rounds != 8 || !out->ipa.l_xy || !out->ipa.l_inf || !out->ipa.r_xy || !out->ipa.r_inf))
        return VC_E_INVALID;
    return vk::verkle_prove(ctx, scheme, table, t, keys, n, root_xy, root_inf, out);
}

int vc_verkle_proof_queries(vc_ctx* ctx, int table, vc_verkle* t, const uint8_t* keys, size_t n, size_t max_q,
                            uint64_t* com_xy, uint8_t* com_inf, uint64_t* z, uint64_t* y, uint64_t* rows, size_t* Q) {
    if (!ctx || !t || !keys || n == 0 || !Q || (max_q && (!com_xy || !com_inf || !z || !y)) ||
        ctx->curve != VC_CURVE_BN254)
        return VC_E_INVALID;
    return vk::verkle_proof_queries(ctx, table, t, keys, n, max_q, com_xy, com_inf, z, y, rows, Q);
}

// The verifier: the query list rebuilt from (root, keys, values, depths, the proof's commitments).
// Commitment 0 below is the root, commitment k + 1 the proof's k-th.
int vc_verkle_verify(vc_ctx* ctx, int scheme, int table, const vc_kzg_vk* vk, int key_len, const uint64_t* root_xy,
                     uint8_t root_inf, const uint8_t* keys, const uint8_t* values32, size_t n,
                     const vc_verkle_proof* proof, int* result) {
    if (result) *result = 0;
    if (!ctx || !root_xy || !keys || !values32 || n == 0 || !proof || !result || !proof->depth ||
        (proof->n_com && (!proof->com_xy || !proof->com_inf)) || key_len < 2 || key_len > 32 ||
        (scheme != 0 && scheme != 1) || (scheme == 1 && !vk) || proof->n_keys != n || ctx->curve != VC_CURVE_BN254)
        return VC_E_INVALID;
    if (scheme == 0 && (!proof->ipa.l_xy || !proof->ipa.l_inf || !proof->ipa.r_xy || !proof->ipa.r_inf)) return VC_E_INVALID;
    const size_t N = (size_t)key_len, C = proof->n_com + 1;
    auto tic = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!vk::verbose()) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[verkle-verify] %s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - tic).count());
        tic = now;
    };
    struct Pos {
        bool ext;
        uint32_t com;
        std::string key;  // an extension's full key
    };
    // (hash maps: the ordered ones made this rebuild 14-24 ms of a 10,000-key verification)
    std::unordered_map<std::string, Pos> pos;  // the units before a position -> what sits there
    std::unordered_map<uint64_t, uint32_t> halves;  // (extension's commitment, half) -> C_half's
    pos.reserve(2 * n);
    halves.reserve(2 * n);
    struct VQ {
        uint32_t com, z;
        uint8_t ykind;  // 0: the item of commitment yref, 1: the literal lit[yref]
        uint32_t yref;
    };
    std::vector<VQ> vq;
    std::vector<std::array<uint64_t, 4>> lit;
    std::unordered_map<uint64_t, uint32_t> emitted;  // (commitment, z) -> its query
    emitted.reserve(8 * n);
    uint32_t next = 1;
    bool ok = true;
    auto same_y = [&](const VQ& a, const VQ& b) {
        if (a.ykind != b.ykind) return false;
        return a.ykind == 0 ? a.yref == b.yref : lit[a.yref] == lit[b.yref];
    };
    auto emit = [&](uint32_t com, uint32_t z, uint8_t ykind, uint32_t yref) {
        const VQ q{com, z, ykind, yref};
        auto it = emitted.find(((uint64_t)com << 32) | z);
        if (it != emitted.end()) {
            if (!same_y(vq[it->second], q)) ok = false;  // one opening, two claimed values
            return;
        }
        emitted.emplace(((uint64_t)com << 32) | z, (uint32_t)vq.size());
        vq.push_back(q);
    };
    auto literal = [&](const uint64_t* v) {
        lit.push_back({v[0], v[1], v[2], v[3]});
        return (uint32_t)lit.size() - 1;
    };
    const uint64_t one[4] = {1, 0, 0, 0};
    for (size_t i = 0; i < n && ok; i++) {
        const uint8_t* K = keys + i * N;
        const size_t d = proof->depth[i];
        if (d < 1 || d > N - 1) {
            ok = false;
            break;
        }
        uint32_t com[33];  // d <= N - 1 <= 31
        com[0] = 0;
        for (size_t j = 1; j <= d && ok; j++) {
            const std::string where(reinterpret_cast<const char*>(K), j);
            const bool ext = j == d;
            const std::string key = ext ? std::string(reinterpret_cast<const char*>(K), N) : std::string();
            auto it = pos.find(where);
            if (it == pos.end()) {
                if (next >= C) {
                    ok = false;
                    break;
                }
                it = pos.emplace(where, Pos{ext, next++, key}).first;
            } else if (it->second.ext != ext || it->second.key != key) {
                ok = false;  // two node kinds, or two extensions, at one position
                break;
            }
            com[j] = it->second.com;
        }
        if (!ok) break;
        const uint8_t u = K[N - 1];
        const int half = u < (uint8_t)(N / 2) ? 1 : 2;
        uint32_t hc;
        auto hi = halves.find(((uint64_t)com[d] << 2) | (uint64_t)half);
        if (hi == halves.end()) {
            if (next >= C) {
                ok = false;
                break;
            }
            hc = next++;
            halves.emplace(((uint64_t)com[d] << 2) | (uint64_t)half, hc);
        } else {
            hc = hi->second;
        }
        for (size_t j = 0; j < d; j++) emit(com[j], K[j], 0, com[j + 1]);
        emit(com[d], 0, 1, literal(one));
        uint64_t w[4];
        vk::item_of_bytes(K, N, w);
        emit(com[d], 1, 1, literal(w));
        emit(com[d], 1 + (uint32_t)half, 0, hc);
        const uint8_t* V = values32 + 32 * i;
        uint64_t lo[4] = {0, 0, 0, 0}, hv[4] = {0, 0, 0, 0};
        memcpy(lo, V, 16);
        memcpy(hv, V + 16, 16);
        emit(hc, (uint32_t)((2 * (size_t)u) % N), 1, literal(lo));
        emit(hc, (uint32_t)((2 * (size_t)u + 1) % N), 1, literal(hv));
    }
    if (!ok || next != C) return VC_OK;  // (verdict 0)
    lap("query list rebuilt");
    // the commitments' items, then the queries as arrays
    std::vector<uint64_t> cxy(C * 8, 0), items(C * 4);
    std::vector<uint8_t> cinf(C);
    cinf[0] = root_inf;
    if (!root_inf) memcpy(&cxy[0], root_xy, 64);
    for (size_t k = 0; k + 1 < C; k++) {
        cinf[k + 1] = proof->com_inf[k];
        if (!cinf[k + 1]) memcpy(&cxy[8 * (k + 1)], proof->com_xy + 8 * k, 64);
    }
    VK_TRY(vc_to_data_item_batch(ctx, cxy.data(), cinf.data(), C, items.data()));
    const size_t Q = vq.size();
    std::vector<uint64_t> qxy(Q * 8), qz(Q), qy(Q * 4);
    std::vector<uint8_t> qinf(Q);
    for (size_t q = 0; q < Q; q++) {
        memcpy(&qxy[8 * q], &cxy[8 * (size_t)vq[q].com], 64);
        qinf[q] = cinf[vq[q].com];
        qz[q] = vq[q].z;
        memcpy(&qy[4 * q], vq[q].ykind == 0 ? &items[4 * (size_t)vq[q].yref] : lit[vq[q].yref].data(), 32);
    }
    lap("items, query arrays");
    int st;
    if (scheme == 0)
        st = vc_multiproof_verify_ipa(ctx, table, 256, Q, qxy.data(), qinf.data(), qz.data(), qy.data(), proof->d_xy,
                                      proof->d_inf, &proof->ipa, result);
    else
        st = vc_multiproof_verify_kzg(ctx, vk, 256, Q, qxy.data(), qinf.data(), qz.data(), qy.data(), proof->d_xy,
                                      proof->d_inf, proof->kzg_proof_xy, proof->kzg_proof_inf, proof->kzg_y, result);
    lap("multiproof verification");
    if (st == VC_E_NOT_ON_CURVE) {  // a malformed point: a verdict, not an error
        *result = 0;
        return VC_OK;
    }
    return st;
}

}  // extern "C"

// Host check of the verkle commitment's host integer logic (verkle-kzg_amd/csrc/verkle_trie.hpp,
// verkle_rows.hpp, verkle_plan.hpp) for tests/test_verkle_plan_host.py: no GPU, no ctx.hpp.
// stdin: "N dense_mode rounds", then per round "count after" (after: 1 = clear_dirty, the commit
// succeeded; 0 = drop_delta, it failed) and count lines "key-hex value-hex". After each round one
// JSON line: the extension stage (built on a 4-worker pool and on a 1-worker pool), the delta plan's
// snapshots and every level's lists, nodes named by their walk path from the root.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../verkle-kzg_amd/csrc/verkle_plan.hpp"
#include "../../verkle-kzg_amd/csrc/verkle_rows.hpp"
using namespace vk;

static std::vector<std::string> g_path;  // node id -> "[u0, u1, ...]"

static void name_nodes(const VTrie& t) {
    g_path.assign(t.nodes.size(), "null");
    std::vector<std::pair<int, std::string>> stack{{0, ""}};
    while (!stack.empty()) {
        auto [id, p] = stack.back();
        stack.pop_back();
        g_path[id] = "[" + p + "]";
        for (auto& kv : t.nodes[id].children) stack.push_back({kv.second, p + (p.empty() ? "" : ", ") + std::to_string(kv.first)});
    }
}

static std::string hex(const uint8_t* b, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) s += d[b[i] >> 4], s += d[b[i] & 15];
    return s;
}
static void unhex(const char* s, uint8_t* out, size_t n) {
    for (size_t i = 0; i < n; i++) {
        unsigned v;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) exit(3);
        out[i] = (uint8_t)v;
    }
}

template <class T, class Fn>
static void list(const char* name, const T* v, size_t n, Fn item, const char* end = ", ") {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < n; i++) printf("%s%s", i ? ", " : "", item(v[i]).c_str());
    printf("]%s", end);
}
static std::string num(uint64_t v) { return std::to_string(v); }

// (a HostPool's threads are never joined: the pools live until the process exits)
static HostPool& pool_of(unsigned workers) {
    static HostPool* p4 = new HostPool(4);
    static HostPool* p1 = new HostPool(1);
    return workers == 4 ? *p4 : *p1;
}

static void show_ext_stage(const VTrie& t, unsigned workers) {
    HostPool& pool = pool_of(workers);
    std::vector<ExtRows16> cache;
    std::vector<uint8_t> buf;
    ExtStage X;
    const int st = ext_stage(t, t.dirty_ext, pool, cache, [&](size_t bytes) { buf.assign(bytes, 0xee); return buf.data(); }, &X);
    if (st != VC_OK) exit(4);
    const size_t E = t.dirty_ext.size();
    printf("{\"workers\": %u, \"parts\": %zu, \"E\": %zu, \"nnz\": %zu, \"maxlen\": %u, \"o_stem\": %zu, \"o_vals\": %zu, "
           "\"o_ids\": %zu, \"o_cols\": %zu, \"o_end\": %zu, \"size\": %zu, ",
           workers, cache.size(), E, X.nnz, X.maxlen, X.o_stem, X.o_vals, X.o_ids, X.o_cols, X.o_end, buf.size());
    const uint8_t* p = X.base;
    list("row_ptr", reinterpret_cast<const uint64_t*>(p), 2 * E + 1, num);
    printf("\"stems\": [");
    for (size_t e = 0; e < E; e++) printf("%s\"%s\"", e ? ", " : "", hex(p + X.o_stem + 32 * e, 32).c_str());
    printf("], \"vals\": [");
    for (size_t k = 0; k < X.nnz; k++) printf("%s\"%s\"", k ? ", " : "", hex(p + X.o_vals + 16 * k, 16).c_str());
    printf("], ");
    list("ids", reinterpret_cast<const uint32_t*>(p + X.o_ids), E, [](uint32_t id) { return g_path[id]; });
    list("cols", reinterpret_cast<const uint32_t*>(p + X.o_cols), X.nnz, num, "}");
}

static void show_level(const VTrie& t, int level, const DeltaPlan& plan, int dense_mode, HostPool& pool) {
    LevelLists L;
    std::vector<uint8_t> buf;
    level_lists(t, level, plan, dense_mode, pool, [&](size_t bytes) { buf.assign(bytes, 0xee); return buf.data(); }, L);
    if (L.status != VC_OK || L.level != level) exit(5);
    printf("{\"level\": %d, \"B\": %zu, \"nnz\": %zu, \"dense\": %s, \"any_delta\": %s, \"o_child\": %zu, \"o_ids\": %zu, "
           "\"o_sidx\": %zu, \"o_add\": %zu, \"o_end\": %zu, \"size\": %zu, ",
           level, L.B, L.nnz, L.dense ? "true" : "false", L.any_delta ? "true" : "false", L.o_child, L.o_ids, L.o_sidx,
           L.o_add, L.o_end, buf.size());
    auto by_path = [](uint32_t id) { return id == 0xffffffffu ? std::string("null") : g_path[id]; };
    list("ptr", L.ptr.data(), L.B + 1, num);
    list("cols", reinterpret_cast<const uint32_t*>(L.pin), L.nnz, num);
    list("child", reinterpret_cast<const uint32_t*>(L.pin + L.o_child), L.nnz, by_path);
    if (L.any_delta) {
        list("sidx", reinterpret_cast<const int32_t*>(L.pin + L.o_sidx), L.nnz, [](int32_t v) { return std::to_string(v); });
        list("add", reinterpret_cast<const uint32_t*>(L.pin + L.o_add), L.B, by_path);
    }
    list("ids", reinterpret_cast<const uint32_t*>(L.pin + L.o_ids), L.B, by_path, "}");
}

static size_t scratch_set(const VTrie& t) {  // entries of plan_slot / snap_slot that are not -1
    size_t c = 0;
    for (int32_t v : t.plan_slot) c += v != -1;
    for (int32_t v : t.snap_slot) c += v != -1;
    return c;
}

int main() {
    int N, dense_mode, rounds;
    if (scanf("%d %d %d", &N, &dense_mode, &rounds) != 3 || N < 2 || N > 32) return 2;
    VTrie t;
    trie_init(t, N);
    HostPool& pool = pool_of(4);
    static char ks[80], vs[80];
    for (int r = 0; r < rounds; r++) {
        int count, after;
        if (scanf("%d %d", &count, &after) != 2) return 2;
        for (int i = 0; i < count; i++) {
            uint8_t key[32] = {0}, val[32];
            if (scanf("%79s %79s", ks, vs) != 2) return 2;
            unhex(ks, key, (size_t)N);
            unhex(vs, val, 32);
            if (trie_insert(t, key, val) != VC_OK) return 6;  // (the test feeds accepted keys only)
        }
        name_nodes(t);
        printf("{\"ext\": [");
        show_ext_stage(t, 4);
        printf(", ");
        show_ext_stage(t, 1);
        printf("], ");
        size_t live;
        {
            const DeltaPlan plan(t);
            live = scratch_set(t);
            printf("\"plans\": %zu, \"scratch_live\": %zu, ", plan.plans.size(), live);
            list("snap_ids", plan.snap_ids.data(), plan.snap_ids.size(), num);
            list("snap", plan.snap_ids.data(), plan.snap_ids.size(), [](uint32_t id) { return g_path[id]; });
            printf("\"levels\": [");
            bool first = true;
            for (int level = (int)t.dirty_int.size() - 1; level >= 0; level--) {  // the commitment's order
                if (t.dirty_int[level].empty()) continue;
                if (!first) printf(", ");
                first = false;
                show_level(t, level, plan, dense_mode, pool);
            }
            printf("], ");
        }
        printf("\"scratch_after\": %zu}\n", scratch_set(t));
        if (after) t.clear_dirty();
        else t.drop_delta();
    }
    return 0;
}

// The device-resident verkle commitment (one context; vc_verkle_commitment's default): every level's
// rows are built, committed and turned into items on the device, the items stored into the mirror by
// node id, so the next level gathers its children's items there -- no per-level read-back or host
// row values for internal levels. The host builds only the extension leaf rows (values it alone
// holds, verkle_rows.hpp ext_stage) and each internal level's (column, child id) lists
// (verkle_plan.hpp).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "scheme_internal.hpp"
#include "verkle_internal.hpp"
#include "verkle_plan.hpp"

namespace vk {

__global__ void k_vk_gather(const uint64_t* __restrict__ item, const uint32_t* __restrict__ ids, size_t n,
                            uint64_t* __restrict__ out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t* s = item + 4 * (size_t)ids[j];
    uint64_t* o = out + 4 * j;
    o[0] = s[0];
    o[1] = s[1];
    o[2] = s[2];
    o[3] = s[3];
}
// a level's row values: item(child) - (sidx < 0 ? 0 : snap[sidx]) mod r (canonical Fr words) --
// a full row's entries have no old value, a delta row's the child's item at the last commitment
__global__ void k_vk_delta(const uint64_t* __restrict__ item, const uint32_t* __restrict__ child,
                           const int32_t* __restrict__ sidx, const uint64_t* __restrict__ snap, size_t n,
                           uint64_t* __restrict__ out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    fe<BN254Fr> a, b = fe_zero<BN254Fr>();
    memcpy(a.v, item + 4 * (size_t)child[j], 32);
    const int32_t k = sidx[j];
    if (k >= 0) memcpy(b.v, snap + 4 * (size_t)k, 32);
    const fe<BN254Fr> d = fe_sub<BN254Fr>(a, b);  // (canonical in, canonical out)
    memcpy(out + 4 * j, d.v, 32);
}
// 16-byte leaf halves -> 4-word scalars
__global__ void k_vk_widen16(const uint64_t* __restrict__ in, size_t n, uint64_t* __restrict__ out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    out[4 * j] = in[2 * j];
    out[4 * j + 1] = in[2 * j + 1];
    out[4 * j + 2] = 0;
    out[4 * j + 3] = 0;
}
// extension commitment rows [1, stem item, c1 item, c2 item] (node.rs:245-256), columns 0..3; the
// stem arrives as its raw 32 LE bytes and is reduced mod r here (from_le_bytes_mod_order of a value
// below 2^256 < 6 r: at most five subtractions)
__global__ void k_vk_ext_rows4(const uint64_t* __restrict__ stem, const uint64_t* __restrict__ it12, size_t E,
                               uint32_t* __restrict__ cols, uint64_t* __restrict__ vals) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // entry 4 k + c
    if (j >= 4 * E) return;
    const size_t k = j >> 2;
    const uint32_t c = (uint32_t)(j & 3);
    cols[j] = c;
    const uint64_t one[4] = {1, 0, 0, 0};
    const uint64_t* v = c == 0 ? one : c == 1 ? stem + 4 * k : it12 + 4 * (2 * k + (c - 2));
    uint64_t w[4] = {v[0], v[1], v[2], v[3]};
    if (c == 1) {
        constexpr uint64_t R[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL,
                                   0x30644e72e131a029ULL};  // BN254 r
        for (int it = 0; it < 5; it++) {
            uint64_t d[4], br = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint64_t a = w[i], b = R[i];
                d[i] = a - b - br;
                br = (a < b || (a == b && br)) ? 1 : 0;
            }
            if (br) break;  // w < r
#pragma unroll
            for (int i = 0; i < 4; i++) w[i] = d[i];
        }
    }
    uint64_t* o = vals + 4 * j;
    o[0] = w[0];
    o[1] = w[1];
    o[2] = w[2];
    o[3] = w[3];
}
// row pointers of E rows of 4: rp[k] = 4 k, k <= E
__global__ void k_vk_rp4(uint64_t* __restrict__ rp, size_t E) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= E) rp[k] = 4 * (uint64_t)k;
}
// rows' results -> the mirror at their node ids
__global__ void k_vk_scatter(const uint32_t* __restrict__ ids, size_t n, const uint64_t* __restrict__ xy,
                             const uint8_t* __restrict__ inf, const uint64_t* __restrict__ it,
                             uint64_t* __restrict__ m_cxy, uint8_t* __restrict__ m_inf, uint64_t* __restrict__ m_item) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const size_t id = ids[j];
#pragma unroll
    for (int k = 0; k < 8; k++) m_cxy[8 * id + k] = xy[8 * j + k];
#pragma unroll
    for (int k = 0; k < 4; k++) m_item[4 * id + k] = it[4 * j + k];
    m_inf[id] = inf[j];
}
// dense width-`width` rows of a small level: dense[b][col] = item[child] (zeroed before)
__global__ void k_vk_dense(const uint32_t* __restrict__ row, const uint32_t* __restrict__ cols,
                           const uint32_t* __restrict__ child, size_t nnz, const uint64_t* __restrict__ item,
                           uint32_t width, uint64_t* __restrict__ dense) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nnz) return;
    const uint64_t* s = item + 4 * (size_t)child[j];
    uint64_t* o = dense + 4 * ((size_t)row[j] * width + cols[j]);
    o[0] = s[0];
    o[1] = s[1];
    o[2] = s[2];
    o[3] = s[3];
}

namespace {

unsigned grid(size_t n) { return (unsigned)((n + 255) / 256); }

// the call's laps: VKZG_VERKLE_STAMPS = the host's time at each lap (no synchronising), printed in
// one line when the call ends; verbose = every lap's time with the stream synchronised
struct Laps {
    vc_ctx* ctx;
    const bool stamps = verkle_stamps();
    std::chrono::steady_clock::time_point tic = std::chrono::steady_clock::now();
    const std::chrono::steady_clock::time_point t_entry = tic;
    std::vector<std::pair<const char*, double>> marks;
    void operator()(const char* what) {
        if (stamps) {
            marks.emplace_back(what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_entry).count());
            return;
        }
        if (!verbose()) return;
        (void)hipStreamSynchronize(ctx->stream);
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[verkle-dev] %s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - tic).count());
        tic = now;
    }
    ~Laps() {
        if (marks.empty()) return;
        std::string line = "[verkle-stamps]";
        char buf[96];
        for (auto& x : marks) {
            snprintf(buf, sizeof buf, " %s@%.0f", x.first, x.second);
            line += buf;
        }
        fprintf(stderr, "%s\n", line.c_str());
    }
};

// one level's uploaded lists (LevelLists' layout, on the device)
struct LevelDev {
    const uint32_t *cols, *child, *ids;
    const int32_t* sidx;  // null without delta rows, as add
    const uint32_t* add;
};

// One commitment's state: the mirror, the stream, the table, and the internal levels' lists, built
// one level ahead of the level that runs
struct DevCommit {
    vc_ctx* ctx;
    Table* tab;
    vc_verkle* t;
    Laps& lap;
    const DeltaPlan& plan;
    uint64_t* m_item = static_cast<uint64_t*>(t->dev.item);
    uint64_t* m_cxy = static_cast<uint64_t*>(t->dev.cxy);
    uint8_t* m_inf = static_cast<uint8_t*>(t->dev.inf);
    hipStream_t st = ctx->stream;
    HostPool& pool = host_pool();
    const int dense_mode = verkle_dense_mode();
    // levels of at most this many (non-zero, window) pairs take the sparse commits' latency path
    // (a wave per 64 pairs, sparse_commit.hip k_fb_sparse_small) instead of the sort-based one: an update's
    // levels; VKZG_SPARSE_SMALL_MAX (pairs, read per call; 0 = never) is the A/B knob
    const size_t small_max = [] {
        const char* env = getenv("VKZG_SPARSE_SMALL_MAX");
        return env ? (size_t)atoll(env) : (size_t)1 << 18;
    }();
    bool small_ok(size_t nnz) const { return sparse_small_pairs(tab, nnz) <= small_max; }

    // the old items of the delta rows' changed slots (DeltaPlan::snap_ids order)
    DevBuf d_snap{ctx}, d_snap_ids{ctx};

    // internal nodes, deepest level first (width 256: the reference's hard-coded HACK). A level's
    // lists depend on the tree alone, so the next level's are built (into the other page-locked
    // buffer) while the current level's kernels run -- in the wait of its normalisation
    std::vector<int> order;
    LevelLists lists[2];
    size_t next_built = 0;  // levels of `order` whose lists are built
    // level cur's lists are in use: the other buffer takes order[cur + 1] (before the first level,
    // cur = 0 and both buffers are free: order[0] and order[1] may be built during the extension
    // commits' kernels)
    size_t cur = 0;
    void build_next() {
        if (next_built < order.size() && next_built <= cur + 1) {
            PinBuf& pinbuf = ctx->pin_verkle_lv[next_built & 1];
            level_lists(*t, order[next_built], plan, dense_mode, pool,
                        [&](size_t bytes) -> uint8_t* { return pinbuf.ensure(bytes) == VC_OK ? pinbuf.as<uint8_t>() : nullptr; },
                        lists[next_built & 1]);
            next_built++;
        }
    }
    const std::function<void()> build_next_fn = [this] { build_next(); };
    // the hook the commits call once their kernels are queued, while lists remain to be built
    const std::function<void()>* overlap() const { return next_built < order.size() ? &build_next_fn : nullptr; }

    // the dense (host-result) levels' staging stays alive until the one sync at the end, and the
    // root's point is taken from them when the root was on such a level (no read-back)
    std::vector<std::vector<uint64_t>> keep64;
    std::vector<std::vector<uint8_t>> keep8;
    std::vector<uvec<uint32_t>> keep32;
    uint64_t root_xy[8];
    uint8_t root_inf = 1;
    bool root_known = false;

    // results of one level's B rows (device) -> the mirror at the nodes' ids
    int scatter(const uint32_t* d_ids, size_t B, const void* d_xy, const uint8_t* d_inf, const void* d_it) {
        VK_LAUNCH(ctx, "verkle_scatter", k_vk_scatter, grid(B), 256, 0, d_ids, B, static_cast<const uint64_t*>(d_xy),
                  d_inf, static_cast<const uint64_t*>(d_it), m_cxy, m_inf, m_item);
        return VC_OK;
    }

    // the snapshot of the delta plan's old items, gathered before this call's scatters overwrite them
    int snapshot() {
        const size_t S = plan.snap_ids.size();
        if (!S) return VC_OK;
        VK_TRY(d_snap_ids.ensure(S * 4));
        VK_TRY(d_snap.ensure(S * 32));
        VK_CHECK_HIP(hipMemcpyAsync(d_snap_ids.p, plan.snap_ids.data(), S * 4, hipMemcpyHostToDevice, st));
        VK_LAUNCH(ctx, "verkle_gather", k_vk_gather, grid(S), 256, 0, m_item, d_snap_ids.as<uint32_t>(), S,
                  d_snap.as<uint64_t>());
        return VC_OK;
    }

    // extension nodes: c1 / c2 rows (host: the leaves), then the width-4 rows on the device
    int extension_level() {
        const std::vector<int>& exts = t->dirty_ext;
        const size_t E = exts.size();
        static thread_local std::vector<ExtRows16> parts_cache;  // storage kept between calls
        // (the rows built and uploaded in pieces, piece p built while piece p - 1 crosses PCIe,
        // measured slower at 65,536 keys: full commitment 2.17-2.23 ms in one piece, 2.33-2.40 in 2,
        // 2.49-2.53 in 4, profiles/r06/verkle/pieces/ -- every piece pays the host pool's fork / join
        // and merge, more than the ~0.05-0.08 ms of upload it hides. Removed: the level's one buffer
        // in one copy.)
        DevBuf d_up(ctx), d_vals(ctx), d_xy(ctx), d_inf(ctx), d_it(ctx);
        ExtStage X;
        VK_TRY(ext_stage(*t, exts, pool, parts_cache,
                         [&](size_t bytes) -> uint8_t* {
                             return ctx->pin_verkle.ensure(bytes) == VC_OK ? ctx->pin_verkle.as<uint8_t>() : nullptr;
                         },
                         &X));
        const size_t nnz = X.nnz;
        const uint32_t maxlen = X.maxlen;
        const uint64_t* rp = reinterpret_cast<const uint64_t*>(X.base);
        lap("ext rows (host)");
        // the row pointers travel in the same copy: the sort-based commit reads them there
        // instead of uploading them again (one 1-MB copy and its gap less, profiles/r06/verkle/)
        VK_TRY(d_up.ensure(X.o_end));
        VK_CHECK_HIP(hipMemcpyAsync(d_up.p, X.base, X.o_end, hipMemcpyHostToDevice, st));
        const uint8_t* du = d_up.as<uint8_t>();
        const uint64_t* d_rp_dev = reinterpret_cast<const uint64_t*>(du);
        const uint64_t* d_stem = reinterpret_cast<const uint64_t*>(du + X.o_stem);
        const uint64_t* d_v16 = reinterpret_cast<const uint64_t*>(du + X.o_vals);
        const uint32_t* d_ids = reinterpret_cast<const uint32_t*>(du + X.o_ids);
        const uint32_t* d_cols = reinterpret_cast<const uint32_t*>(du + X.o_cols);
        VK_TRY(d_xy.ensure(2 * E * 64));
        VK_TRY(d_inf.ensure(2 * E));
        VK_TRY(d_it.ensure(2 * E * 32));
        if (small_ok(nnz)) {  // the 16-byte values read as they are
            SmallRows in;
            in.batch = 2 * E;
            in.row_ptr = rp;
            in.mode = 1;
            in.d_cols = d_cols;
            in.d_vals = d_v16;
            in.d_out_xy = d_xy.as<uint64_t>();
            in.d_out_inf = d_inf.as<uint8_t>();
            in.d_out_item = d_it.as<uint64_t>();
            VK_TRY(sparse_small_items_dev(ctx, tab, in));
        } else {
            VK_TRY(d_vals.ensure(std::max<size_t>(nnz, 1) * 32));
            if (nnz)
                VK_LAUNCH(ctx, "verkle_widen", k_vk_widen16, grid(nnz), 256, 0, d_v16, nnz, d_vals.as<uint64_t>());
            // rows of <= 4 non-zeros (random keys: one leaf per extension) are the sparse commit's
            // chunks as they are (an empty row is an empty chunk: the identity), no chunk lists
            VK_TRY(sparse_commit_items_dev(ctx, tab, 2 * E, rp, maxlen <= 4, d_cols, d_vals.p, d_xy.p,
                                           d_inf.as<uint8_t>(), d_it.p, nullptr, nullptr, nullptr, nullptr,
                                           order.empty() ? nullptr : &build_next_fn, d_rp_dev));
        }
        lap("ext c1 / c2 commits");
        // the width-4 rows use bases 0..3 only: their own table with 20-bit windows (13 instead of
        // 16 window adds per scalar, 3.5 GB; VKZG_VERKLE_LEAD_C: the window bits, 0 = the SRS's table)
        Table* tab4 = tab;
        {
            const char* lc = getenv("VKZG_VERKLE_LEAD_C");
            const int c4 = lc ? atoi(lc) : 20;
            if (c4 > 0 && tab->n >= 4 && c4 > tab->fb_c) {
                Table* lt = nullptr;
                VK_TRY(lead_table(ctx, tab, 4, c4, &lt));
                if (lt) tab4 = lt;
            }
        }
        DevBuf d_c4(ctx), d_v4(ctx);
        VK_TRY(d_c4.ensure(4 * E * 4));
        VK_TRY(d_v4.ensure(4 * E * 32));
        VK_LAUNCH(ctx, "verkle_ext_rows4", k_vk_ext_rows4, grid(4 * E), 256, 0, d_stem, d_it.as<uint64_t>(), E,
                  d_c4.as<uint32_t>(), d_v4.as<uint64_t>());
        // rows of 4: row_ptr[k] = 4 k, kept between calls (a fresh 0.5 MB vector's page faults and
        // fill were ~30 us of idle GPU before the width-4 commits)
        static thread_local uvec<uint64_t> rp4;
        if (rp4.size() < E + 1) {
            rp4.resize(E + 1);
            for (size_t k = 0; k <= E; k++) rp4[k] = 4 * k;
        }
        if (small_ok(4 * E)) {  // results straight into the mirror
            SmallRows in;
            in.batch = E;
            in.row_ptr = rp4.data();
            in.mode = 0;
            in.d_cols = d_c4.as<uint32_t>();
            in.d_vals = d_v4.as<uint64_t>();
            in.d_dst = d_ids;
            in.d_out_xy = m_cxy;
            in.d_out_inf = m_inf;
            in.d_out_item = m_item;
            VK_TRY(sparse_small_items_dev(ctx, tab4, in, order.empty() ? nullptr : &build_next_fn));
        } else {  // results straight into the mirror as well; row_ptr[k] = 4 k made on the device
            DevBuf d_rp4(ctx);
            VK_TRY(d_rp4.ensure((E + 1) * 8));
            VK_LAUNCH(ctx, "verkle_rp4", k_vk_rp4, grid(E + 1), 256, 0, d_rp4.as<uint64_t>(), E);
            VK_TRY(sparse_commit_items_dev(ctx, tab4, E, rp4.data(), true, d_c4.as<uint32_t>(), d_v4.p, m_cxy, m_inf,
                                           m_item, nullptr, nullptr, nullptr, d_ids,
                                           order.empty() ? nullptr : &build_next_fn, d_rp4.as<uint64_t>()));
        }
        lap("ext commits");
        return VC_OK;
    }

    // a level of <= 64 rows (or VKZG_VERKLE_DENSE=1): dense rows gathered on the device, committed
    // on the latency path (host results), the <= 64 items on the host, results uploaded into the mirror
    int level_dense(const LevelLists& L, const LevelDev& d) {
        const size_t B = L.B, nnz = L.nnz, nz1 = std::max<size_t>(nnz, 1);
        uvec<uint32_t> row(nz1);
        for (size_t b = 0; b < B; b++)
            for (uint64_t j = L.ptr[b]; j < L.ptr[b + 1]; j++) row[j] = (uint32_t)b;
        DevBuf d_row(ctx), d_dense(ctx), d_xy(ctx), d_inf(ctx), d_it(ctx);
        VK_TRY(d_row.ensure(nz1 * 4));
        VK_TRY(d_dense.ensure(B * 256 * 32));
        VK_TRY(d_xy.ensure(B * 64));
        VK_TRY(d_inf.ensure(B));
        VK_TRY(d_it.ensure(B * 32));
        VK_CHECK_HIP(hipMemsetAsync(d_dense.p, 0, B * 256 * 32, st));
        if (nnz) {
            VK_CHECK_HIP(hipMemcpyAsync(d_row.p, row.data(), nnz * 4, hipMemcpyHostToDevice, st));
            VK_LAUNCH(ctx, "verkle_dense", k_vk_dense, grid(nnz), 256, 0, d_row.as<uint32_t>(), d.cols, d.child,
                      nnz, m_item, 256u, d_dense.as<uint64_t>());
        }
        std::vector<uint64_t> hxy(B * 8), hit(B * 4);
        std::vector<uint8_t> hinf(B);
        bool on_host = false;
        VK_TRY(msm_batch_run(ctx, tab, 256, d_dense.p, B, 0, d_xy.p, d_inf.as<uint8_t>(), hxy.data(), hinf.data(),
                             &on_host, nullptr, overlap()));
        if (!on_host) {
            VK_CHECK_HIP(hipMemcpyAsync(hxy.data(), d_xy.p, B * 64, hipMemcpyDeviceToHost, st));
            VK_CHECK_HIP(hipMemcpyAsync(hinf.data(), d_inf.p, B, hipMemcpyDeviceToHost, st));
            VK_CHECK_HIP(hipStreamSynchronize(st));
        }
        for (size_t b = 0; b < B; b++) mont_to_canon<BN254Fr>(to_data_item_host(&hxy[8 * b], hinf[b] != 0), &hit[4 * b]);
        VK_CHECK_HIP(hipMemcpyAsync(d_xy.p, hxy.data(), B * 64, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_inf.p, hinf.data(), B, hipMemcpyHostToDevice, st));
        VK_CHECK_HIP(hipMemcpyAsync(d_it.p, hit.data(), B * 32, hipMemcpyHostToDevice, st));
        VK_TRY(scatter(d.ids, B, d_xy.p, d_inf.as<uint8_t>(), d_it.p));
        const uint32_t* h_ids = reinterpret_cast<const uint32_t*>(L.pin + L.o_ids);
        for (size_t b = 0; b < B; b++)
            if (h_ids[b] == 0) {  // the root (node id 0)
                memcpy(root_xy, &hxy[8 * b], 64);
                root_inf = hinf[b];
                root_known = true;
            }
        // the uploads above read these host vectors: kept (not synchronised) until the end
        keep64.push_back(std::move(hxy));
        keep64.push_back(std::move(hit));
        keep8.push_back(std::move(hinf));
        keep32.push_back(std::move(row));
        lap("internal level (dense)");
        return VC_OK;
    }

    // a level within small_max: children's items gathered in the kernel; results into the mirror
    int level_small(const LevelLists& L, const LevelDev& d) {
        SmallRows in;
        in.batch = L.B;
        in.row_ptr = L.ptr.data();
        in.mode = 2;
        in.d_cols = d.cols;
        in.d_item = m_item;
        in.d_child = d.child;
        in.d_sidx = d.sidx;
        in.d_snap = d_snap.as<uint64_t>();
        in.d_add_ids = d.add;
        in.d_add_xy = m_cxy;
        in.d_add_inf = m_inf;
        in.d_dst = d.ids;
        in.d_out_xy = m_cxy;
        in.d_out_inf = m_inf;
        in.d_out_item = m_item;
        VK_TRY(sparse_small_items_dev(ctx, tab, in, overlap()));
        lap(L.any_delta ? "internal level (small, delta rows)" : "internal level (small)");
        return VC_OK;
    }

    // any other level: the row values gathered (minus the snapshot for delta rows), then the
    // sort-based sparse commit
    int level_sparse(const LevelLists& L, const LevelDev& d) {
        const size_t nnz = L.nnz;
        DevBuf d_vals(ctx);
        VK_TRY(d_vals.ensure(std::max<size_t>(nnz, 1) * 32));
        if (L.any_delta) {
            if (nnz)
                VK_LAUNCH(ctx, "verkle_delta", k_vk_delta, grid(nnz), 256, 0, m_item, d.child, d.sidx,
                          d_snap.as<uint64_t>(), nnz, d_vals.as<uint64_t>());
        } else if (nnz) {
            VK_LAUNCH(ctx, "verkle_gather", k_vk_gather, grid(nnz), 256, 0, m_item, d.child, nnz, d_vals.as<uint64_t>());
        }
        // results straight into the mirror (a delta row's old commitment is read there by the first
        // normalisation kernel, its new one written by the second); the next level's lists are built
        // once this level's kernels are queued
        VK_TRY(sparse_commit_items_dev(ctx, tab, L.B, L.ptr.data(), false, d.cols, d_vals.p, m_cxy, m_inf, m_item, d.add,
                                       m_cxy, m_inf, d.ids, overlap()));
        lap(L.any_delta ? "internal level (sparse, delta rows)" : "internal level (sparse)");
        return VC_OK;
    }

    // level order[oi]: its lists uploaded in one copy, then one of the three routes
    int internal_level(size_t oi) {
        cur = oi;
        if (next_built <= oi) build_next();
        const LevelLists& L = lists[oi & 1];
        if (L.status != VC_OK) return L.status;
        DevBuf d_up(ctx);
        VK_TRY(d_up.ensure(L.o_end));
        VK_CHECK_HIP(hipMemcpyAsync(d_up.p, L.pin, L.o_end, hipMemcpyHostToDevice, st));
        const uint8_t* du = d_up.as<uint8_t>();
        LevelDev d;
        d.cols = reinterpret_cast<const uint32_t*>(du);
        d.child = reinterpret_cast<const uint32_t*>(du + L.o_child);
        d.ids = reinterpret_cast<const uint32_t*>(du + L.o_ids);
        d.sidx = L.any_delta ? reinterpret_cast<const int32_t*>(du + L.o_sidx) : nullptr;
        d.add = L.any_delta ? reinterpret_cast<const uint32_t*>(du + L.o_add) : nullptr;
        if (L.dense) return level_dense(L, d);
        if (small_ok(L.nnz)) return level_small(L, d);
        return level_sparse(L, d);
    }

    // the root's commitment from the mirror (the rest stays there: host_valid = false)
    int root(uint64_t* out_xy, uint8_t* out_inf) {
        uint64_t rxy[8];
        uint8_t rinf = 1;
        if (root_known) {  // the root's level ran on the host-result path
            memcpy(rxy, root_xy, 64);
            rinf = root_inf;
        } else {
            VK_CHECK_HIP(hipMemcpyAsync(rxy, m_cxy, 64, hipMemcpyDeviceToHost, st));
            VK_CHECK_HIP(hipMemcpyAsync(&rinf, m_inf, 1, hipMemcpyDeviceToHost, st));
        }
        VK_CHECK_HIP(hipStreamSynchronize(st));  // also: every staging vector above may die now
        lap(root_known ? "final sync (root from the dense level)" : "root read-back");
        memcpy(out_xy, rxy, 64);
        *out_inf = rinf;
        return VC_OK;
    }
};

}  // namespace

int verkle_commitment_dev(vc_ctx* ctx, int table, vc_verkle* t, uint64_t* out_xy, uint8_t* out_inf) {
    if (!ctx || !t || !out_xy || !out_inf) return VC_E_INVALID;
    Guard guard(ctx);
    Table* tab = ctx->table(table);
    if (!tab) return VC_E_TABLE;
    if (tab->curve != VC_CURVE_BN254) return VC_E_INVALID;
    Laps lap{ctx};
    DeltaGuard delta_guard{t};
    VK_TRY(mirror_prepare(ctx, t));
    lap("mirror");
    // VKZG_VERKLE_DELTA=0 (read per call, A/B probe) recommits every row in full
    const char* delta_env = getenv("VKZG_VERKLE_DELTA");
    const DeltaPlan plan(*t, !(delta_env && atoi(delta_env) == 0));
    DevCommit C{ctx, tab, t, lap, plan};
    VK_TRY(C.snapshot());
    lap("delta plan");
    for (int level = (int)t->dirty_int.size() - 1; level >= 0; level--)
        if (!t->dirty_int[level].empty()) C.order.push_back(level);
    if (!t->dirty_ext.empty()) VK_TRY(C.extension_level());
    for (size_t oi = 0; oi < C.order.size(); oi++) VK_TRY(C.internal_level(oi));
    VK_TRY(C.root(out_xy, out_inf));
    t->clear_dirty();
    t->host_valid = false;
    delta_guard.ok = true;
    lap("dirty lists cleared");
    return VC_OK;
}

}  // namespace vk

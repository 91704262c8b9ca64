// Host check of IPA batch verification's shared text (verkle-kzg_amd/csrc/ipa_batch.hpp, what the
// kernels of ipa_batch.hip wrap). Reads the flat dump tests/test_ipa_verify_batch_host.py writes
// (argv[1]): the CRS, the fresh-transcript entries of tests/golden/ipa_verify_many.json with their
// recorded challenges, and batches (entry indices, rho, the oracle's fold S). Checks
//   * entry_challenges (SHA-256 from register words, expand_message_xmd, the reduction mod r,
//     compress_words) against the recorded w / x of every entry;
//   * the fold of every batch, entry by entry through fold_entry with those challenges and the
//     weights rho^j, plus N + 1 plain scalar multiplications over the CRS, against the oracle's S;
//   * pow_index against repeated multiplication.
// Prints one JSON line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../verkle-kzg_amd/csrc/ipa_batch.hpp"
#include "../../verkle-kzg_amd/csrc/host/fr.hpp"
using namespace vk;
using namespace vk::ipab;

struct Words {
    uint32_t w[8];
};
static bool read_words(FILE* f, Words& out) {  // one hex token, up to 64 digits
    char tok[80];
    if (fscanf(f, "%79s", tok) != 1) return false;
    memset(out.w, 0, sizeof out.w);
    const size_t len = strlen(tok);
    for (size_t i = 0; i < len; i++) {
        const char c = tok[len - 1 - i];
        const uint32_t d = c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10;
        out.w[i / 8] |= d << (4 * (i % 8));
    }
    return true;
}
struct Pt {
    int inf;
    uint32_t xy[16];
};
static bool read_pt(FILE* f, Pt& p) {
    Words x, y;
    if (fscanf(f, "%d", &p.inf) != 1 || !read_words(f, x) || !read_words(f, y)) return false;
    memcpy(p.xy, x.w, 32);
    memcpy(p.xy + 8, y.w, 32);
    return true;
}
static G1A scalar_mul(const G1P& P, const FrE& k_mont) {
    const FrE k = fe_from_mont<BN254Fr>(k_mont);
    G1A r = BN254G1::zero();
    for (int b = 255; b >= 0; b--) {
        r = BN254G1::dbl(r);
        if ((k.v[b >> 5] >> (b & 31)) & 1u) r = BN254G1::madd(r, P, false);
    }
    return r;
}

struct Entry {
    uint32_t N;
    int K, valid;
    Pt com;
    Words point, tip, y, w;
    std::vector<Words> x;
    std::vector<Pt> l, r;
};
// the ABI's flat arrays (as 32-bit words) of a list of entries of one N
struct Arrays {
    std::vector<uint32_t> com_xy, points, l_xy, r_xy, tip, y;
    std::vector<uint8_t> com_inf, l_inf, r_inf;
    void push(const Entry& e) {
        com_xy.insert(com_xy.end(), e.com.xy, e.com.xy + 16);
        com_inf.push_back((uint8_t)e.com.inf);
        points.insert(points.end(), e.point.w, e.point.w + 8);
        tip.insert(tip.end(), e.tip.w, e.tip.w + 8);
        y.insert(y.end(), e.y.w, e.y.w + 8);
        for (int k = 0; k < e.K; k++) {
            l_xy.insert(l_xy.end(), e.l[k].xy, e.l[k].xy + 16);
            l_inf.push_back((uint8_t)e.l[k].inf);
            r_xy.insert(r_xy.end(), e.r[k].xy, e.r[k].xy + 16);
            r_inf.push_back((uint8_t)e.r[k].inf);
        }
    }
};

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int ncrs = 0, nent = 0, nbatch = 0;
    if (fscanf(f, "%d", &ncrs) != 1) return 2;
    std::vector<G1P> crs(ncrs);
    for (int i = 0; i < ncrs; i++) {
        Pt p;
        if (!read_pt(f, p) || p.inf || !bn::g1_load(p.xy, crs[i])) return 2;
    }
    if (fscanf(f, "%d", &nent) != 1) return 2;
    std::vector<Entry> ents(nent);
    int chal_checked = 0, chal_bad = 0, identity_seen = 0;
    for (Entry& e : ents) {
        if (fscanf(f, "%u %d %d", &e.N, &e.K, &e.valid) != 3) return 2;
        if (!read_pt(f, e.com) || !read_words(f, e.point) || !read_words(f, e.tip) || !read_words(f, e.y) ||
            !read_words(f, e.w))
            return 2;
        e.x.resize(e.K), e.l.resize(e.K), e.r.resize(e.K);
        for (auto& x : e.x)
            if (!read_words(f, x)) return 2;
        for (auto& p : e.l)
            if (!read_pt(f, p)) return 2;
        for (auto& p : e.r)
            if (!read_pt(f, p)) return 2;
        Arrays a;
        a.push(e);
        std::vector<uint32_t> ch(8 * (size_t)(e.K + 1));
        entry_challenges(0, e.K, a.com_xy.data(), a.com_inf.data(), a.points.data(), a.y.data(), a.l_xy.data(),
                         a.l_inf.data(), a.r_xy.data(), a.r_inf.data(), ch.data());
        for (int k = 0; k <= e.K; k++) {
            const FrE got = fe_from_mont<BN254Fr>(fr_load(ch.data() + 8 * k));
            chal_checked++;
            if (memcmp(got.v, k == 0 ? e.w.w : e.x[k - 1].w, 32) != 0) {
                chal_bad++;
                fprintf(stderr, "MISMATCH: entry %d challenge %d\n", (int)(&e - ents.data()), k);
            }
        }
        for (auto& p : e.l) identity_seen += p.inf;
    }
    if (fscanf(f, "%d", &nbatch) != 1) return 2;
    int fold_bad = 0, fold_nonzero = 0;
    for (int b = 0; b < nbatch; b++) {
        uint32_t N;
        int cnt;
        Words rho_w;
        if (fscanf(f, "%u %d", &N, &cnt) != 2 || !read_words(f, rho_w)) return 2;
        int K = 0;
        while ((1u << K) < N) K++;
        Arrays a;
        std::vector<uint32_t> chal;
        for (int j = 0; j < cnt; j++) {
            int idx;
            if (fscanf(f, "%d", &idx) != 1 || idx < 0 || idx >= nent || ents[idx].N != N) return 2;
            a.push(ents[idx]);
        }
        Pt want;
        if (!read_pt(f, want) || (int)N + 1 > ncrs) return 2;
        chal.resize((size_t)cnt * 8 * (K + 1));
        for (int j = 0; j < cnt; j++)
            entry_challenges(j, K, a.com_xy.data(), a.com_inf.data(), a.points.data(), a.y.data(), a.l_xy.data(),
                             a.l_inf.data(), a.r_xy.data(), a.r_inf.data(), chal.data() + (size_t)j * 8 * (K + 1));
        const FrE rho = fe_to_mont<BN254Fr>(fr_load(rho_w.w));
        const FrE omega = bn254_group_gen(N), n_inv = fe_inv_bin<BN254Fr>(mont_from_u64<BN254Fr>(N));
        std::vector<FrE> pw(N), row(N + 1, fe_zero<BN254Fr>());
        FrE acc = fe_one<BN254Fr>();
        for (uint32_t i = 0; i < N; i++) pw[i] = acc, acc = fe_mul<BN254Fr>(acc, omega);
        G1A S = BN254G1::zero();
        FrE wt = fe_one<BN254Fr>();
        bool ok = true;
        for (int j = 0; j < cnt && ok; j++) {
            if (!fe_eq<BN254Fr>(wt, pow_index(rho, (uint64_t)j))) ok = false;  // the weights by index
            ok = ok && fold_entry(j, N, K, a.com_xy.data(), a.com_inf.data(), a.points.data(), a.l_xy.data(),
                                  a.l_inf.data(), a.r_xy.data(), a.r_inf.data(), a.tip.data(), a.y.data(),
                                  chal.data() + (size_t)j * 8 * (K + 1), pw.data(), n_inv, wt, row.data(), S, scalar_mul);
            wt = fe_mul<BN254Fr>(wt, rho);
        }
        for (uint32_t i = 0; i <= N; i++) S = BN254G1::add(S, scalar_mul(crs[i], row[i]));
        bn::Fq ax, ay;
        const bool inf = !BN254G1::to_aff<true>(S, ax, ay);
        bool same = ok && inf == (want.inf != 0);
        if (same && !inf) {
            ax = fe_from_mont<BN254Fq>(ax), ay = fe_from_mont<BN254Fq>(ay);
            same = memcmp(ax.v, want.xy, 32) == 0 && memcmp(ay.v, want.xy + 8, 32) == 0;
        }
        if (!same) {
            fold_bad++;
            fprintf(stderr, "MISMATCH: batch %d (N %u, %d entries)\n", b, N, cnt);
        }
        fold_nonzero += inf ? 0 : 1;
    }
    fclose(f);
    printf("{\"entries\": %d, \"challenges\": %d, \"challenges_bad\": %d, \"identity_points\": %d, \"batches\": %d, "
           "\"fold_bad\": %d, \"fold_nonzero\": %d}\n",
           nent, chal_checked, chal_bad, identity_seen, nbatch, fold_bad, fold_nonzero);
    return 0;
}

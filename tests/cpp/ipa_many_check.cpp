// Host check of IPA batch proving's shared text (verkle-kzg_amd/csrc/ipa_many.hpp, what the kernels
// of ipa_many.hip wrap). Reads the flat dump tests/test_ipa_prove_many_host.py writes (argv[1]):
// openings with their data row, commitment, point, the recorded L_k / R_k of their proof and the
// expected field side. Each opening runs as the kernels run it -- init, K rounds, finish -- with the
// 64 lanes of the wave in a loop and the xor butterflies as plain loops over the lanes' values:
//   * the barycentric row (in the domain and outside), y and w;
//   * every round's two rows of N + 1 scalars, entry by entry;
//   * every fold the device keeps: a, b and the coefficients after each round but the last, whose
//     fold of a is the tip (its b and coefficients are never needed);
//   * the tip.
// An opening marked `full` carries all of these (the Python oracle's values); the others only y and
// the tip (the N = 256 golden proofs). Prints one JSON line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../verkle-kzg_amd/csrc/ipa_many.hpp"
#include "../../verkle-kzg_amd/csrc/host/fr.hpp"
using namespace vk;
using namespace vk::ipam;

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
static bool read_vec(FILE* f, size_t n, std::vector<Words>& v) {
    v.resize(n);
    for (auto& w : v)
        if (!read_words(f, w)) return false;
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
static FrE mont(const Words& w) { return fe_to_mont<BN254Fr>(fr_load(w.w)); }

struct Tally {
    long weights = 0, weights_bad = 0, ys = 0, ys_bad = 0, ws = 0, ws_bad = 0, rows = 0, rows_bad = 0, folds = 0,
         folds_bad = 0, tips = 0, tips_bad = 0;
};
// got (Montgomery) against the expected canonical words
static void expect(const FrE& got, const Words& want, long& n, long& bad, const char* what, int cas, int k, size_t i) {
    n++;
    const FrE c = fe_from_mont<BN254Fr>(got);
    if (memcmp(c.v, want.w, 32) != 0) {
        bad++;
        if (bad < 8) fprintf(stderr, "MISMATCH: opening %d %s round %d entry %zu\n", cas, what, k, i);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int ncases = 0, inside = 0, outside = 0, seen_n = 0;
    if (fscanf(f, "%d", &ncases) != 1) return 2;
    Tally t;
    for (int cas = 0; cas < ncases; cas++) {
        uint32_t N;
        int K, full;
        if (fscanf(f, "%u %d %d", &N, &K, &full) != 3 || N < 2 || N > IM_N_MAX || (1u << K) != N) return 2;
        Pt com;
        Words zw, want_y, want_tip, want_w;
        std::vector<Words> data, want_b;
        if (!read_pt(f, com) || !read_words(f, zw) || !read_vec(f, N, data) || !read_words(f, want_y) ||
            !read_words(f, want_tip))
            return 2;
        if (full && (!read_words(f, want_w) || !read_vec(f, N, want_b))) return 2;
        struct Round {
            Pt l, r;
            Words x;
            std::vector<Words> sl, sr, a, b, coeff;
        };
        std::vector<Round> rounds(K);
        for (int k = 0; k < K; k++) {
            Round& rd = rounds[k];
            if (!read_pt(f, rd.l) || !read_pt(f, rd.r)) return 2;
            const size_t m2 = (size_t)(N >> (k + 1));
            if (full && (!read_words(f, rd.x) || !read_vec(f, N + 1, rd.sl) || !read_vec(f, N + 1, rd.sr) ||
                         !read_vec(f, m2, rd.a) || !read_vec(f, m2, rd.b) || !read_vec(f, N, rd.coeff)))
                return 2;
        }
        seen_n |= (int)N;

        // the device's buffers of one opening
        std::vector<FrE> row(N), pw(N), wa(N), wb(2 * (size_t)N), wc(N), rows(2 * ((size_t)N + 1));
        for (uint32_t i = 0; i < N; i++) row[i] = mont(data[i]);
        const FrE om = bn254_group_gen(N), n_inv = fe_inv_bin<BN254Fr>(mont_from_u64<BN254Fr>(N));
        FrE acc = fe_one<BN254Fr>();
        for (uint32_t i = 0; i < N; i++) pw[i] = acc, acc = fe_mul<BN254Fr>(acc, om);

        // ---- init
        uint64_t idx = 0;
        const bool in_dom = point_in_domain(zw.w, N, &idx);
        (in_dom ? inside : outside)++;
        const FrE z = mont(zw);
        FrE tot[64], oth[64];
        for (uint32_t l = 0; l < 64; l++) oth[l] = fe_one<BN254Fr>();
        if (!in_dom) {
            for (uint32_t l = 0; l < 64; l++) tot[l] = bary_lane_total(pw.data(), N, z, l);
            for (uint32_t s = 1; s < 64; s <<= 1) {
                FrE before[64];
                memcpy(before, tot, sizeof tot);
                for (uint32_t l = 0; l < 64; l++) kzgm::others_step<BN254Fr>(tot[l], oth[l], before[l ^ s]);
            }
        }
        FrE y = fe_zero<BN254Fr>();
        for (uint32_t l = 0; l < 64; l++)
            y = fe_add<BN254Fr>(y, init_lane(row.data(), pw.data(), N, z, in_dom, idx, oth[l], n_inv, l, wb.data()));
        uint32_t yc[8], prev[8];
        const FrE w = opening_w(com.xy, com.inf != 0, zw.w, y, yc);
        fr_store(fe_from_mont<BN254Fr>(w), prev);
        t.ys++;
        if (memcmp(yc, want_y.w, 32) != 0) {
            t.ys_bad++;
            fprintf(stderr, "MISMATCH: opening %d y\n", cas);
        }
        if (full) {
            expect(w, want_w, t.ws, t.ws_bad, "w", cas, -1, 0);
            for (uint32_t i = 0; i < N; i++) expect(wb[i], want_b[i], t.weights, t.weights_bad, "weight", cas, -1, i);
        }

        // ---- rounds, then the finish: r closes round r - 1
        for (int r = 0; r <= K; r++) {
            Level lv = level_first(row.data(), wb.data(), N);
            if (r > 0) {
                const Round& rd = rounds[r - 1];
                const FrE x = close_challenge(prev, r - 1, rd.l.xy, rd.l.inf != 0, rd.r.xy, rd.r.inf != 0);
                fr_store(fe_from_mont<BN254Fr>(x), prev);
                if (full) expect(x, rd.x, t.ws, t.ws_bad, "x", cas, r - 1, 0);
                lv = level_after(row.data(), wa.data(), wb.data(), N, r - 1, x);
            }
            if (r == K) {
                uint32_t tw[8];
                tip_words(lv, tw);
                t.tips++;
                if (memcmp(tw, want_tip.w, 32) != 0) {
                    t.tips_bad++;
                    fprintf(stderr, "MISMATCH: opening %d tip\n", cas);
                }
                break;
            }
            const uint32_t m = N >> r, half = m / 2;
            FrE* sL = rows.data();
            FrE* sR = sL + (N + 1);
            for (uint32_t l = 0; l < 64; l++) rows_lane(lv, wc.data(), N, r, l, sL, sR);
            FrE DL = fe_zero<BN254Fr>(), DR = fe_zero<BN254Fr>();
            for (uint32_t l = 0; l < 64; l++) {
                FrE dl, dr;
                halves_lane(lv, half, l, a_store(wa.data(), N, r), b_store(wb.data(), N, r), dl, dr);
                DL = fe_add<BN254Fr>(DL, dl), DR = fe_add<BN254Fr>(DR, dr);
            }
            sL[N] = q_term(w, DL), sR[N] = q_term(w, DR);
            if (!full) continue;
            for (uint32_t i = 0; i <= N; i++) {
                expect(sL[i], rounds[r].sl[i], t.rows, t.rows_bad, "L row", cas, r, i);
                expect(sR[i], rounds[r].sr[i], t.rows, t.rows_bad, "R row", cas, r, i);
            }
            if (r > 0) {  // the fold that closed round r - 1, as this round stored it
                const Round& rd = rounds[r - 1];
                const FrE* la = wa.data() + a_level(N, r);
                const FrE* lb = wb.data() + b_level(N, r);
                for (uint32_t j = 0; j < m; j++) {
                    expect(la[j], rd.a[j], t.folds, t.folds_bad, "a", cas, r - 1, j);
                    expect(lb[j], rd.b[j], t.folds, t.folds_bad, "b", cas, r - 1, j);
                }
                for (uint32_t i = 0; i < N; i++) expect(wc[i], rd.coeff[i], t.folds, t.folds_bad, "coeff", cas, r - 1, i);
            }
        }
    }
    fclose(f);
    printf("{\"openings\": %d, \"inside\": %d, \"outside\": %d, \"widths\": %d, \"weights\": %ld, \"weights_bad\": %ld, "
           "\"ys\": %ld, \"ys_bad\": %ld, \"challenges\": %ld, \"challenges_bad\": %ld, \"rows\": %ld, \"rows_bad\": %ld, "
           "\"folds\": %ld, \"folds_bad\": %ld, \"tips\": %ld, \"tips_bad\": %ld}\n",
           ncases, inside, outside, seen_n, t.weights, t.weights_bad, t.ys, t.ys_bad, t.ws, t.ws_bad, t.rows, t.rows_bad,
           t.folds, t.folds_bad, t.tips, t.tips_bad);
    return 0;
}

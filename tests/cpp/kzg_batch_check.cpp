// Host check of KZG batch verification's arithmetic (verkle-kzg_amd/csrc/kzg_batch.hpp, the text
// k_kzg_batch_prep and the host path of vc_kzg_batch_fold compile). Reads the flat dump that
// tests/test_kzg_verify_batch_host.py writes (argv[1]): the domain size, [s]_2, and batches of
// entries with their challenge, the oracle's P1 / P2 and the oracle's verdict. Per batch: the fold
// as one range and as three ranges added (the host pool's shape) must both give the oracle's two
// points, a malformed batch must be reported as such, and the final pairing entry over the key's
// line tables must give the oracle's verdict. Also rho^i by square-and-multiply on the index
// against the running product.
// Prints one JSON line: batches, wrong results, accepted / rejected / malformed batches seen.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../verkle-kzg_amd/csrc/kzg_batch.hpp"
#include "../../verkle-kzg_amd/csrc/host/fr.hpp"
using namespace vk;
using namespace vk::kzgb;

static bool read_words(FILE* f, uint32_t* w) {  // one hex token, up to 64 digits
    char tok[80];
    if (fscanf(f, "%79s", tok) != 1) return false;
    memset(w, 0, 32);
    const size_t len = strlen(tok);
    for (size_t i = 0; i < len; i++) {
        const char c = tok[len - 1 - i];
        const uint32_t d = c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10;
        w[i / 8] |= d << (4 * (i % 8));
    }
    return true;
}
static bool read_pt(FILE* f, uint8_t& inf, uint32_t* xy) {
    int flag;
    if (fscanf(f, "%d", &flag) != 1 || !read_words(f, xy) || !read_words(f, xy + 8)) return false;
    inf = (uint8_t)flag;
    return true;
}
// the accumulator as canonical affine words; true for the identity
static bool to_affine(const G1A& a, uint32_t* xy) {
    bn::Fq x, y;
    memset(xy, 0, 64);
    if (!BN254G1::to_aff<true>(a, x, y)) return true;
    x = fe_from_mont<BN254Fq>(x), y = fe_from_mont<BN254Fq>(y);
    memcpy(xy, x.v, 32);
    memcpy(xy + 8, y.v, 32);
    return false;
}
static bool same_point(const G1A& a, uint8_t want_inf, const uint32_t* want_xy) {
    uint32_t xy[16];
    const bool inf = to_affine(a, xy);
    if (inf || want_inf) return inf == (want_inf != 0);
    return memcmp(xy, want_xy, 64) == 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned long long size = 0;
    int nbatch = 0;
    if (fscanf(f, "%llu", &size) != 1) return 2;
    bn::G2Aff s2{bn::fq2_zero(), bn::fq2_zero(), false};
    bn::Fq* dst[4] = {&s2.x.c0, &s2.x.c1, &s2.y.c0, &s2.y.c1};
    for (int k = 0; k < 4; k++) {
        uint32_t w[8];
        if (!read_words(f, w)) return 2;
        bn::Fq c;
        memcpy(c.v, w, 32);
        *dst[k] = fe_to_mont<BN254Fq>(c);
    }
    if (!bn::g2_on_twist(s2)) return 2;
    std::vector<bn::LineCoef> lines(2 * bn::PC::ATE_LINES);
    bn::ate_line_table(s2, lines.data());
    bn::ate_line_table(bn::g2_generator(), lines.data() + bn::PC::ATE_LINES);
    const FrE omega = bn254_group_gen(size);
    if (fscanf(f, "%d", &nbatch) != 1) return 2;
    int wrong = 0, accepted = 0, rejected = 0, malformed = 0, pow_checks = 0;
    for (int bi = 0; bi < nbatch; bi++) {
        int n, want_malformed, want_valid;
        uint32_t rho_w[8];
        if (fscanf(f, "%d %d %d", &n, &want_malformed, &want_valid) != 3 || !read_words(f, rho_w)) return 2;
        std::vector<uint32_t> com(16 * (size_t)n), proof(16 * (size_t)n), pts(8 * (size_t)n), ys(8 * (size_t)n);
        std::vector<uint8_t> cinf(n), pinf(n);
        for (int i = 0; i < n; i++)
            if (!read_pt(f, cinf[i], &com[16 * (size_t)i]) || !read_words(f, &pts[8 * (size_t)i]) ||
                !read_pt(f, pinf[i], &proof[16 * (size_t)i]) || !read_words(f, &ys[8 * (size_t)i]))
                return 2;
        uint8_t w1inf, w2inf;
        uint32_t w1[16], w2[16];
        if (!read_pt(f, w1inf, w1) || !read_pt(f, w2inf, w2)) return 2;
        const FrE rho = fe_to_mont<BN254Fr>(fr_words(rho_w));
        // rho^i on the index (the kernel's way) against the running product (fold_range's way)
        FrE run = fe_one<BN254Fr>();
        for (int i = 0; i < n && i < 40; i++) {
            pow_checks++;
            if (!fe_eq<BN254Fr>(pow_index(rho, (uint64_t)i), run)) wrong++;
            run = bn::fr_mul(run, rho);
        }
        auto fold = [&](int parts, Sums& total) {
            total = sums_zero();
            bool ok = true;
            for (int k = 0; k < parts; k++) {
                Sums s;
                if (!fold_range((size_t)n * k / parts, (size_t)n * (k + 1) / parts, com.data(), cinf.data(), pts.data(),
                                proof.data(), pinf.data(), ys.data(), rho, omega, size, s))
                    ok = false;
                else
                    total = sums_add(total, s);
            }
            return ok;
        };
        Sums one, three;
        const bool ok1 = fold(1, one), ok3 = fold(3, three);
        bool bad = ok1 != ok3 || ok1 == (want_malformed != 0);
        bool verdict = false;
        if (ok1 && ok3) {
            G1A P1, P2, Q1, Q2;
            fold_finish(one, P1, P2);
            fold_finish(three, Q1, Q2);
            bad |= !same_point(P1, w1inf, w1) || !same_point(P2, w2inf, w2);
            bad |= !same_point(Q1, w1inf, w1) || !same_point(Q2, w2inf, w2);
            verdict = pair_check(P1, P2, lines.data(), lines.data() + bn::PC::ATE_LINES);
            (verdict ? accepted : rejected)++;
        } else {
            malformed++;
        }
        bad |= verdict != (want_valid != 0);
        if (bad) {
            wrong++;
            fprintf(stderr, "MISMATCH: batch %d (n = %d): folds ok %d / %d, verdict %d, want malformed %d valid %d\n", bi,
                    n, (int)ok1, (int)ok3, (int)verdict, want_malformed, want_valid);
        }
    }
    fclose(f);
    printf("{\"batches\": %d, \"wrong\": %d, \"accepted\": %d, \"rejected\": %d, \"malformed\": %d, \"pow_checks\": %d}\n",
           nbatch, wrong, accepted, rejected, malformed, pow_checks);
    return 0;
}

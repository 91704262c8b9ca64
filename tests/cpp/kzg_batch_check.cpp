// Host check of KZG batch verification's arithmetic (verkle-kzg_amd/csrc/kzg_batch.hpp, the text
// k_kzg_batch_prep and the host path of vc_kzg_batch_fold compile) for the curve named by argv[2]
// (bn254 when absent, or bls12_381). Reads the flat dump that tests/test_kzg_verify_batch_host.py
// or tests/test_kzg_verify_bls_host.py writes (argv[1]): the domain size, [s]_2, and batches of
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

static bool read_words(FILE* f, uint32_t* w, int words = 8) {  // one hex token, up to 8 digits per word
    char tok[112];
    if (fscanf(f, "%111s", tok) != 1) return false;
    memset(w, 0, 4 * words);
    const size_t len = strlen(tok);
    if (len > 8 * (size_t)words) return false;
    for (size_t i = 0; i < len; i++) {
        const char c = tok[len - 1 - i];
        const uint32_t d = c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10;
        w[i / 8] |= d << (4 * (i % 8));
    }
    return true;
}
template <class C>
static bool read_pt(FILE* f, uint8_t& inf, uint32_t* xy) {
    constexpr int NL = C::Fq::N;
    int flag;
    if (fscanf(f, "%d", &flag) != 1 || !read_words(f, xy, NL) || !read_words(f, xy + NL, NL)) return false;
    inf = (uint8_t)flag;
    return true;
}
// the accumulator as canonical affine words; true for the identity
template <class C>
static bool to_affine(const G1AOf<C>& a, uint32_t* xy) {
    using Fq = typename C::Fq;
    fe<Fq> x, y;
    memset(xy, 0, 4 * C::PW);
    if (!C::G1::template to_aff<true>(a, x, y)) return true;
    x = fe_from_mont<Fq>(x), y = fe_from_mont<Fq>(y);
    memcpy(xy, x.v, 4 * Fq::N);
    memcpy(xy + Fq::N, y.v, 4 * Fq::N);
    return false;
}
template <class C>
static bool same_point(const G1AOf<C>& a, uint8_t want_inf, const uint32_t* want_xy) {
    uint32_t xy[C::PW];
    const bool inf = to_affine<C>(a, xy);
    if (inf || want_inf) return inf == (want_inf != 0);
    return memcmp(xy, want_xy, 4 * C::PW) == 0;
}

template <class C>
static int run(FILE* f) {
    using Fq = typename C::Fq;
    using Fr = typename C::Fr;
    using FrE = fe<Fr>;
    using G1A = G1AOf<C>;
    constexpr int NL = Fq::N, PW = C::PW;
    unsigned long long size = 0;
    int nbatch = 0;
    if (fscanf(f, "%llu", &size) != 1) return 2;
    ate::G2AffT<Fq> s2{ate::fq2_zero<Fq>(), ate::fq2_zero<Fq>(), false};
    fe<Fq>* dst[4] = {&s2.x.c0, &s2.x.c1, &s2.y.c0, &s2.y.c1};
    for (int k = 0; k < 4; k++) {
        uint32_t w[NL];
        if (!read_words(f, w, NL)) return 2;
        fe<Fq> c;
        memcpy(c.v, w, 4 * NL);
        *dst[k] = fe_to_mont<Fq>(c);
    }
    if (!ate::g2_on_twist(s2)) return 2;
    std::vector<ate::LineCoefT<Fq>> lines(2 * C::PC::ATE_LINES);
    ate::ate_line_table(s2, lines.data());
    ate::ate_line_table(ate::g2_generator<Fq>(), lines.data() + C::PC::ATE_LINES);
    const FrE omega = group_gen_t<Fr>(size, fr_generator<Fr>());
    if (fscanf(f, "%d", &nbatch) != 1) return 2;
    int wrong = 0, accepted = 0, rejected = 0, malformed = 0, pow_checks = 0;
    for (int bi = 0; bi < nbatch; bi++) {
        int n, want_malformed, want_valid;
        uint32_t rho_w[8];
        if (fscanf(f, "%d %d %d", &n, &want_malformed, &want_valid) != 3 || !read_words(f, rho_w)) return 2;
        std::vector<uint32_t> com(PW * (size_t)n), proof(PW * (size_t)n), pts(8 * (size_t)n), ys(8 * (size_t)n);
        std::vector<uint8_t> cinf(n), pinf(n);
        for (int i = 0; i < n; i++)
            if (!read_pt<C>(f, cinf[i], &com[PW * (size_t)i]) || !read_words(f, &pts[8 * (size_t)i]) ||
                !read_pt<C>(f, pinf[i], &proof[PW * (size_t)i]) || !read_words(f, &ys[8 * (size_t)i]))
                return 2;
        uint8_t w1inf, w2inf;
        uint32_t w1[PW], w2[PW];
        if (!read_pt<C>(f, w1inf, w1) || !read_pt<C>(f, w2inf, w2)) return 2;
        const FrE rho = fe_to_mont<Fr>(fr_words<Fr>(rho_w));
        // rho^i on the index (the kernel's way) against the running product (fold_range's way)
        FrE run = fe_one<Fr>();
        for (int i = 0; i < n && i < 40; i++) {
            pow_checks++;
            if (!fe_eq<Fr>(pow_index(rho, (uint64_t)i), run)) wrong++;
            run = ate::fr_mul(run, rho);
        }
        auto fold = [&](int parts, Sums<C>& total) {
            total = sums_zero<C>();
            bool ok = true;
            for (int k = 0; k < parts; k++) {
                Sums<C> s;
                if (!fold_range<C>((size_t)n * k / parts, (size_t)n * (k + 1) / parts, com.data(), cinf.data(), pts.data(),
                                   proof.data(), pinf.data(), ys.data(), rho, omega, size, s))
                    ok = false;
                else
                    total = sums_add(total, s);
            }
            return ok;
        };
        Sums<C> one, three;
        const bool ok1 = fold(1, one), ok3 = fold(3, three);
        bool bad = ok1 != ok3 || ok1 == (want_malformed != 0);
        bool verdict = false;
        if (ok1 && ok3) {
            G1A P1, P2, Q1, Q2;
            fold_finish(one, P1, P2);
            fold_finish(three, Q1, Q2);
            bad |= !same_point<C>(P1, w1inf, w1) || !same_point<C>(P2, w2inf, w2);
            bad |= !same_point<C>(Q1, w1inf, w1) || !same_point<C>(Q2, w2inf, w2);
            verdict = pair_check(P1, P2, lines.data(), lines.data() + C::PC::ATE_LINES);
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
    printf("{\"batches\": %d, \"wrong\": %d, \"accepted\": %d, \"rejected\": %d, \"malformed\": %d, \"pow_checks\": %d}\n",
           nbatch, wrong, accepted, rejected, malformed, pow_checks);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const bool bls = argc > 2 && !strcmp(argv[2], "bls12_381");
    if (argc > 2 && !bls && strcmp(argv[2], "bn254")) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    const int st = bls ? run<BLS381Kzg>(f) : run<BN254Kzg>(f);
    fclose(f);
    return st;
}

// Host check of KZG subvector batch verification's shared text (verkle-kzg_amd/csrc/kzg_subv.hpp, the
// text k_kzg_subv_fold compiles) and of miller_loop_tabn (pairing_common.hpp). argv[1]: the flat dump
// tests/test_kzg_subv_batch_host.py writes, argv[2]: "bn254" or "bls12_381". Per case N, k, the k
// indices, the k values y, a weight, and from Python integers the k + 1 coefficients of Z_S and the
// k of weight * I. Each case runs as the wave kernel runs it: 64 lanes in a loop over the same lane
// functions, a step's reads all made before its writes (the fence), the xor shuffles as array reads
// of the partner lane's value, the LDS rows as arrays of exactly k values, so the sanitizer sees any
// index past them; then as the host path runs it (coeffs_serial), with the weights from the tables.
// The pairing part: miller_loop_tabn at m = 2 against miller_loop_tab2 value for value, and its
// final exponentiation at m = 3 against the general product with lines made on the fly, for a product
// that is one and one that is not.
// Prints one JSON line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../verkle-kzg_amd/csrc/kzg_subv.hpp"
#include "../../verkle-kzg_amd/csrc/host/fr.hpp"
using namespace vk;
using namespace vk::kzgv;

template <class F>
static bool read_canon(FILE* f, uint32_t* w) {  // one hex token, up to 64 digits, below r
    char tok[80];
    if (fscanf(f, "%79s", tok) != 1) return false;
    memset(w, 0, 32);
    const size_t len = strlen(tok);
    if (len > 64) return false;
    for (size_t i = 0; i < len; i++) {
        const char c = tok[len - 1 - i];
        const uint32_t d = c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10;
        w[i / 8] |= d << (4 * (i % 8));
    }
    return ate::words_below_modulus<F>(w);
}
template <class F>
static bool read_mont(FILE* f, fe<F>& out) {
    uint32_t w[8];
    if (!read_canon<F>(f, w)) return false;
    out = fe_to_mont<F>(fr_words<F>(w));
    return true;
}

template <class C>
static int pairing_part(int& wrong) {
    using Fq = typename C::Fq;
    using Fr = typename C::Fr;
    using Line = ate::LineCoefT<Fq>;
    constexpr int L = C::PC::ATE_LINES;
    const uint32_t s_w[8] = {100, 0, 0, 0, 0, 0, 0, 0}, s2_w[8] = {10000, 0, 0, 0, 0, 0, 0, 0};
    const ate::G2AffT<Fq> Q[3] = {ate::g2_generator<Fq>(), ate::g2_mul(ate::g2_generator<Fq>(), s_w, 8),
                                  ate::g2_mul(ate::g2_generator<Fq>(), s2_w, 8)};
    std::vector<Line> lines(3 * L);
    const Line* tab[3];
    for (int t = 0; t < 3; t++) {
        ate::ate_line_table(Q[t], lines.data() + t * L);
        tab[t] = lines.data() + t * L;
    }
    int checks = 0;
    const fe<Fr> s = fe_to_mont<Fr>(fr_words<Fr>(s_w)), ss = fe_mul<Fr>(s, s);
    for (int round = 0; round < 2; round++) {
        // a + b s + c s^2 = 0 (round 0) or 1 (round 1); c = 0 in the second variant: an identity skipped
        for (int variant = 0; variant < 2; variant++) {
            const uint32_t b_w[8] = {0x1234567u + round, 77, 0, 5, 0, 0, 0, 0}, c_w[8] = {99u, 3, 0, 0, 8, 0, 0, 1};
            const fe<Fr> b = fe_to_mont<Fr>(fr_words<Fr>(b_w));
            const fe<Fr> c = variant ? fe_zero<Fr>() : fe_to_mont<Fr>(fr_words<Fr>(c_w));
            fe<Fr> a = fe_neg<Fr>(fe_add<Fr>(fe_mul<Fr>(b, s), fe_mul<Fr>(c, ss)));
            if (round) a = fe_add<Fr>(a, fe_one<Fr>());
            const fe<Fr> k[3] = {a, b, c};
            ate::G1EvalT<Fq> P[3];
            for (int t = 0; t < 3; t++) P[t] = ate::g1_eval_acc(kzgb::scalar_mul<C>(C::g1_generator(), k[t]));
            if (P[2].skip != (variant == 1)) wrong++;
            const ate::Fq12T<Fq> f2 = ate::miller_loop_tab2(P[0], tab[0], P[1], tab[1]);
            const ate::Fq12T<Fq> g2 = ate::miller_loop_tabn<Fq>(2, P, tab);
            if (memcmp(&f2, &g2, sizeof f2) != 0) wrong++;
            const bool one = ate::fq12_is_one(ate::final_exp(ate::miller_loop_tabn<Fq>(3, P, tab)));
            if (one != ate::pairing_product_is_one(3, P, Q) || one != (round == 0)) wrong++;
            // the product of two calls is the call over all tables
            const ate::Fq12T<Fq> split = ate::fq12_mul(ate::miller_loop_tabn<Fq>(1, P, tab),
                                                       ate::miller_loop_tabn<Fq>(2, P + 1, tab + 1));
            if (ate::fq12_is_one(ate::final_exp(split)) != one) wrong++;
            checks += 4;
        }
    }
    return checks;
}

template <class C>
static int run(FILE* f) {
    using F = typename C::Fr;
    using FrE = fe<F>;
    int ncases = 0;
    if (fscanf(f, "%d", &ncases) != 1) return 2;
    int wrong = 0;
    long coeffs_checked = 0, sums_checked = 0;
    for (int ci = 0; ci < ncases; ci++) {
        unsigned N, k;
        if (fscanf(f, "%u %u", &N, &k) != 2) return 2;
        if (N < 2 || N > kzgm::KM_MAX_N || (N & (N - 1)) || k < 1 || k > N) return 2;
        std::vector<uint32_t> S(k), y(8 * (size_t)k);
        for (unsigned t = 0; t < k; t++)
            if (fscanf(f, "%u", &S[t]) != 1 || S[t] >= N) return 2;
        for (unsigned t = 0; t < k; t++)
            if (!read_canon<F>(f, &y[8 * (size_t)t])) return 2;
        FrE wgt;
        if (!read_mont<F>(f, wgt)) return 2;
        std::vector<FrE> wantZ(k + 1), wantA(k);
        for (auto& v : wantZ)
            if (!read_mont<F>(f, v)) return 2;
        for (auto& v : wantA)
            if (!read_mont<F>(f, v)) return 2;
        // the domain's tables, as poly.hip caches them (inv1[0] = 0)
        const FrE omega = group_gen_t<F>(N, fr_generator<F>());
        std::vector<FrE> pw(N), inv1(N, fe_zero<F>());
        pw[0] = fe_one<F>();
        for (unsigned i = 1; i < N; i++) pw[i] = fe_mul<F>(pw[i - 1], omega);
        for (unsigned i = 1; i < N; i++) inv1[i] = fe_inv_bin<F>(fe_sub<F>(pw[i], fe_one<F>()));

        bool bad = false;
        std::vector<FrE> z(k), a(k, fe_zero<F>());  // the LDS rows
        // ---- Z, lanes over t, 64 at a time from the top
        for (uint32_t i = 0; i < k; i++) {
            const FrE x = pw[S[i]];
            for (uint32_t c = i >> 6;; c--) {
                FrE v[64];
                for (uint32_t lane = 0; lane < 64; lane++)
                    if (64 * c + lane <= i) v[lane] = z_step<F>(z.data(), i, 64 * c + lane, x);
                for (uint32_t lane = 0; lane < 64; lane++)  // (after the fence)
                    if (64 * c + lane <= i) z[64 * c + lane] = v[lane];
                if (!c) break;
            }
        }
        // ---- the rows' scalars, two rows above the degree as well
        for (uint32_t t = 0; t <= k + 2; t++, coeffs_checked++) {
            const FrE got = row_scalar<F>(z.data(), k, t, wgt);
            bad |= !fe_eq<F>(got, t <= k ? fe_mul<F>(wgt, wantZ[t]) : fe_zero<F>());
        }
        bad |= !fe_eq<F>(wantZ[k], fe_one<F>());
        // ---- the division, lanes over the set, a wave sum per t
        uint32_t sum = 0;
        for (uint32_t t = 0; t < k; t++) sum += S[t];
        const FrE wsum = kzgs::sub_wsum<F>(pw.data(), N, sum);
        for (uint32_t ib = 0; ib < k; ib += 64) {
            FrE x[64], u[64], b[64];
            for (uint32_t lane = 0; lane < 64; lane++) {
                x[lane] = u[lane] = b[lane] = fe_zero<F>();
                if (ib + lane < k)
                    lane_weight<F>(S.data(), k, pw.data(), inv1.data(), N, ib + lane, wsum, &y[8 * (size_t)(ib + lane)],
                                   wgt, x[lane], u[lane]);
            }
            for (uint32_t t = k; t-- > 0;) {
                FrE s[64];
                for (uint32_t lane = 0; lane < 64; lane++) {
                    b[lane] = div_step<F>(z.data(), k, t, x[lane], b[lane]);
                    s[lane] = fe_mul<F>(u[lane], b[lane]);
                }
                for (uint32_t m = 1; m < 64; m <<= 1) {
                    FrE nx[64];
                    for (uint32_t lane = 0; lane < 64; lane++) nx[lane] = fe_add<F>(s[lane], s[lane ^ m]);
                    memcpy(s, nx, sizeof s);
                }
                for (uint32_t lane = 1; lane < 64; lane++) bad |= !fe_eq<F>(s[lane], s[0]);
                a[t] = fe_add<F>(a[t], s[0]);
            }
        }
        for (uint32_t t = 0; t < k; t++, sums_checked++) bad |= !fe_eq<F>(a[t], wantA[t]);
        // ---- one thread, the host path's text (the weights from the tables here)
        {
            std::vector<FrE> x(k), c(k), z2(k), b(k), a2(k, fe_zero<F>());
            for (uint32_t t = 0; t < k; t++) {
                x[t] = pw[S[t]];
                c[t] = kzgs::sub_weight_full<F>(kzgs::sub_weight<F>(S.data(), k, inv1.data(), N, t, wsum), pw.data(), S[t]);
            }
            coeffs_serial<F>(x.data(), c.data(), y.data(), k, wgt, z2.data(), b.data(), a2.data());
            for (uint32_t t = 0; t < k; t++) bad |= !fe_eq<F>(z2[t], wantZ[t]) || !fe_eq<F>(a2[t], wantA[t]);
        }
        if (bad) {
            wrong++;
            fprintf(stderr, "MISMATCH: case %d (N = %u, k = %u)\n", ci, N, k);
        }
    }
    int pwrong = 0;
    const int pairing_checks = pairing_part<C>(pwrong);
    printf("{\"cases\": %d, \"wrong\": %d, \"coeffs\": %ld, \"sums\": %ld, \"pairing_checks\": %d, \"pairing_wrong\": %d}\n",
           ncases, wrong, coeffs_checked, sums_checked, pairing_checks, pwrong);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    const int rc = strcmp(argv[2], "bls12_381") == 0 ? run<BLS381Kzg>(f) : run<BN254Kzg>(f);
    fclose(f);
    return rc;
}

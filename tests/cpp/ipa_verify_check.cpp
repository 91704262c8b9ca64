// Host check of the batched IPA verifier's per-proof arithmetic (verkle-kzg_amd/csrc/
// ipa_verify.hpp, the text the kernels of ipa_verify.hip wrap). Reads the flat dump of
// tests/golden/ipa_verify_many.json that tests/test_ipa_verify_many_host.py writes (argv[1]) and,
// for every entry, evaluates the whole identity with the recorded challenges, laid out as the
// kernels lay it out: the field phase over 64 lanes with the xor-butterfly of fractions, the curve
// phase over 8 lanes per proof with the xor-butterfly of partial sums (and over 1 lane, which must
// agree). The fixed part is N + 1 plain double-and-add scalar multiplications over the CRS.
// Also: the barycentric dot product carried as one fraction (and its single inversion) against
// per-element inverses.
// Prints one JSON line: entries, verdicts that differ from `valid`, true / false verdicts seen,
// barycentric comparisons and mismatches.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../verkle-kzg_amd/csrc/ipa_verify.hpp"
#include "../../verkle-kzg_amd/csrc/host/fr.hpp"
using namespace vk;
using namespace vk::ipav;

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

// the verdict of one entry; lp = lanes per proof of the curve phase
static bool verdict(const Entry& e, const std::vector<G1P>& crs, int lp) {
    const uint32_t N = e.N;
    const int K = e.K, T = 1 + 2 * K;
    if (!bn::words_below_modulus<BN254Fr>(e.tip.w) || !bn::words_below_modulus<BN254Fr>(e.y.w) ||
        !bn::words_below_modulus<BN254Fr>(e.point.w))
        return false;
    std::vector<FrE> xs(K);
    for (int k = 0; k < K; k++) xs[k] = fe_to_mont<BN254Fr>(fr_load(e.x[k].w));
    const FrE w = fe_to_mont<BN254Fr>(fr_load(e.w.w)), tip = fe_to_mont<BN254Fr>(fr_load(e.tip.w));
    const FrE z = fe_to_mont<BN254Fr>(fr_load(e.point.w)), y = fe_to_mont<BN254Fr>(fr_load(e.y.w));
    const FrE omega = bn254_group_gen(N);
    std::vector<FrE> pw(N);
    FrE acc = fe_one<BN254Fr>();
    for (uint32_t i = 0; i < N; i++) pw[i] = acc, acc = fe_mul<BN254Fr>(acc, omega);
    const FrE n_inv = fe_inv_bin<BN254Fr>(mont_from_u64<BN254Fr>(N));
    // field phase, 64 lanes
    uint64_t idx = 0;
    const bool in_dom = point_in_domain(e.point.w, N, &idx);
    std::vector<FrE> row(N + 1);
    Frac f[64];
    for (uint32_t lane = 0; lane < 64; lane++) {
        f[lane] = frac_zero();
        for (uint32_t i = lane; i < N; i += 64) {
            const FrE s = s_coeff(xs.data(), K, i);
            row[i] = row_entry(tip, s);
            if (!in_dom) f[lane] = frac_add_term(f[lane], s, pw[i], z);
        }
    }
    for (uint32_t m = 1; m < 64; m <<= 1) {
        Frac g[64];
        for (uint32_t lane = 0; lane < 64; lane++) g[lane] = frac_add(f[lane], f[lane ^ m]);
        memcpy(f, g, sizeof f);
    }
    FrE scale = fe_one<BN254Fr>();
    if (!in_dom) {
        scale = f[0].den;
        for (uint32_t i = 0; i < N; i++) row[i] = fr_mul(row[i], scale);
    }
    const FrE cb = in_dom ? s_coeff(xs.data(), K, (uint32_t)idx) : bary_dot_scaled(f[0], z, K, n_inv);
    std::vector<uint32_t> vs(8 * (size_t)T);
    const FrE prodx = var_scalars(xs.data(), K, scale, vs.data());
    row[N] = row_tail(prodx, w, y, tip, cb, scale);
    if (fe_is_zero<BN254Fr>(scale)) return false;
    // fixed part: plain scalar multiplications over the CRS, then canonical affine
    G1A fixed = BN254G1::zero();
    for (uint32_t i = 0; i <= N; i++) fixed = BN254G1::add(fixed, scalar_mul(crs[i], row[i]));
    uint32_t fxy[16] = {0};
    bn::Fq ax, ay;
    const bool finf = !BN254G1::to_aff<true>(fixed, ax, ay);
    if (!finf) {
        ax = fe_from_mont<BN254Fq>(ax), ay = fe_from_mont<BN254Fq>(ay);
        memcpy(fxy, ax.v, 32);
        memcpy(fxy + 8, ay.v, 32);
    }
    // curve phase, lp lanes
    std::vector<G1P> mont(T);
    std::vector<int> inf(T);
    for (int t = 0; t < T; t++) {
        const Pt& p = t == 0 ? e.com : ((t - 1) & 1) ? e.r[(t - 1) >> 1] : e.l[(t - 1) >> 1];
        inf[t] = p.inf;
        if (!p.inf && !bn::g1_load(p.xy, mont[t])) return false;
    }
    std::vector<G1A> part(lp);
    for (int sub = 0; sub < lp; sub++) {
        const int count = sub < T ? (T - sub + lp - 1) / lp : 0;
        part[sub] = var_partial_sum(
            count,
            [&](int j, G1P& P) {
                const int t = sub + j * lp;
                if (inf[t]) return false;
                P = mont[t];
                return true;
            },
            [&](int j, int b) { return ((vs[8 * (size_t)(sub + j * lp) + (b >> 5)] >> (b & 31)) & 1u) != 0; });
    }
    for (int m = 1; m < lp; m <<= 1) {
        std::vector<G1A> g(lp);
        for (int sub = 0; sub < lp; sub++) g[sub] = BN254G1::add(part[sub], part[sub ^ m]);
        part = g;
    }
    return sum_is_identity(part[0], fxy, finf);
}

static uint64_t rs = 0x243F6A8885A308D3ull;
static uint64_t rnd64() {
    rs ^= rs << 13;
    rs ^= rs >> 7;
    rs ^= rs << 17;
    return rs;
}
static FrE rnd_fr() {
    FrE r;
    for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)rnd64();
    r.v[7] &= 0x0fffffffu;  // below r
    return r;
}

// sum_i s_i t w^i / (z - w^i) as one fraction against N inversions, and the one-hot branch
static void bary_checks(int& checks, int& bad) {
    for (uint32_t N : {4u, 32u}) {
        int K = 0;
        while ((1u << K) < N) K++;
        std::vector<FrE> xs(K);
        for (auto& x : xs) x = rnd_fr();
        const FrE omega = bn254_group_gen(N), n_inv = fe_inv_bin<BN254Fr>(mont_from_u64<BN254Fr>(N));
        FrE big = rnd_fr();
        big.v[7] |= 0x20000000u;  // a 254-bit value below r = 0x30644e72..
        const FrE zs[5] = {mont_from_u64<BN254Fr>(5), mont_from_u64<BN254Fr>(N - 1), mont_from_u64<BN254Fr>(N),
                           mont_from_u64<BN254Fr>(1000), fe_to_mont<BN254Fr>(big)};
        for (const FrE& z : zs) {
            const FrE t = fe_mul<BN254Fr>(fe_sub<BN254Fr>(fe_pow_u64<BN254Fr>(z, N), fe_one<BN254Fr>()), n_inv);
            FrE direct = fe_zero<BN254Fr>(), w = fe_one<BN254Fr>();
            Frac f = frac_zero();
            bool pole = false;
            for (uint32_t i = 0; i < N; i++) {
                const FrE s = s_coeff(xs.data(), K, i), den = fe_sub<BN254Fr>(z, w);
                pole |= fe_is_zero<BN254Fr>(den);
                const FrE b = fe_mul<BN254Fr>(fe_mul<BN254Fr>(t, w), fe_inv_bin<BN254Fr>(den));
                direct = fe_add<BN254Fr>(direct, fe_mul<BN254Fr>(b, s));
                f = frac_add_term(f, s, w, z);
                w = fe_mul<BN254Fr>(w, omega);
            }
            if (pole) continue;  // (z a domain element: the call rejects it before any arithmetic)
            checks++;
            // the scaled form the kernel uses, den <b, s>, and the one inversion that undoes the scale
            const FrE scaled = bary_dot_scaled(f, z, K, n_inv);
            if (!fe_eq<BN254Fr>(fe_mul<BN254Fr>(direct, f.den), scaled)) bad++;
            checks++;
            if (!fe_eq<BN254Fr>(direct, fe_mul<BN254Fr>(scaled, fe_inv_bin<BN254Fr>(f.den)))) bad++;
        }
        // the one-hot branch: <b, s> = s_point for a point below N
        for (uint64_t pt : {(uint64_t)0, (uint64_t)5 % N, (uint64_t)N - 1}) {
            uint32_t pw[8] = {(uint32_t)pt};
            uint64_t idx = 99;
            checks++;
            if (!point_in_domain(pw, N, &idx) || idx != pt) bad++;
        }
        uint32_t at_n[8] = {N};
        uint64_t idx;
        checks++;
        if (point_in_domain(at_n, N, &idx)) bad++;
    }
    // points_coeffs' order at N = 4: [x0 x1, x0, x1, 1]
    FrE xs[2] = {rnd_fr(), rnd_fr()};
    const FrE want[4] = {fe_mul<BN254Fr>(xs[0], xs[1]), xs[0], xs[1], fe_one<BN254Fr>()};
    for (uint32_t i = 0; i < 4; i++) {
        checks++;
        if (!fe_eq<BN254Fr>(s_coeff(xs, 2, i), want[i])) bad++;
    }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int ncrs = 0, nent = 0;
    if (fscanf(f, "%d", &ncrs) != 1) return 2;
    std::vector<G1P> crs(ncrs);
    for (int i = 0; i < ncrs; i++) {
        Pt p;
        if (!read_pt(f, p) || p.inf || !bn::g1_load(p.xy, crs[i])) return 2;
    }
    if (fscanf(f, "%d", &nent) != 1) return 2;
    int wrong = 0, seen_true = 0, seen_false = 0;
    for (int n = 0; n < nent; n++) {
        Entry e;
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
        if ((int)e.N + 1 > ncrs) return 2;
        const bool v8 = verdict(e, crs, 8), v1 = verdict(e, crs, 1);
        if (v8 != (e.valid != 0) || v1 != v8) {
            wrong++;
            fprintf(stderr, "MISMATCH: entry %d: valid %d, 8 lanes %d, 1 lane %d\n", n, e.valid, (int)v8, (int)v1);
        }
        (v8 ? seen_true : seen_false)++;
    }
    fclose(f);
    int bchecks = 0, bbad = 0;
    bary_checks(bchecks, bbad);
    printf("{\"entries\": %d, \"wrong\": %d, \"true\": %d, \"false\": %d, \"bary_checks\": %d, \"bary_bad\": %d}\n", nent,
           wrong, seen_true, seen_false, bchecks, bbad);
    return 0;
}

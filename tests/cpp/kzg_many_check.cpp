// Host check of KZG batch proving's arithmetic (verkle-kzg_amd/csrc/kzg_many.hpp, the text the
// kernels of kzg_many.hip compile). Reads the flat dump tests/test_kzg_prove_many_host.py writes
// (argv[1]): per case N, width, the oracle's class of the point (0 in the domain, 1 outside, 2 the
// reference panics), the point, the row, z^N - 1 and -- unless the reference panics -- y and the
// whole quotient row. Each case runs as the wave kernel runs it: 64 lanes in a loop over the same
// per-lane functions, the xor shuffles as array reads of the partner lane's value, 1 / D by the host
// inverse (the kernel gets it from the batch inversion).
// Prints one JSON line: cases, wrong results, and how many cases of each class were seen.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../verkle-kzg_amd/csrc/kzg_many.hpp"
#include "../../verkle-kzg_amd/csrc/host/fr.hpp"
using namespace vk;
using namespace vk::kzgm;
using F = BN254Fr;
using FrE = fe<F>;

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
static bool read_mont(FILE* f, FrE& out) {
    uint32_t w[8];
    if (!read_words(f, w) || !words_canonical<F>(w)) return false;
    out = fe_to_mont<F>(words_load<F>(w));
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int ncases = 0;
    if (fscanf(f, "%d", &ncases) != 1) return 2;
    int wrong = 0, seen[3] = {0, 0, 0}, rows_checked = 0;
    for (int ci = 0; ci < ncases; ci++) {
        unsigned N, width;
        int want_cls;
        uint32_t zw[8];
        if (fscanf(f, "%u %u %d", &N, &width, &want_cls) != 3 || !read_words(f, zw)) return 2;
        if (N < 2 || N > KM_MAX_N || (N & (N - 1)) || width > N || want_cls < 0 || want_cls > 2) return 2;
        std::vector<FrE> row(width);
        for (unsigned i = 0; i < width; i++)
            if (!read_mont(f, row[i])) return 2;
        FrE wantD;
        if (!read_mont(f, wantD)) return 2;
        FrE wantY = fe_zero<F>();
        std::vector<FrE> wantQ(N);
        if (want_cls != 2) {
            if (!read_mont(f, wantY)) return 2;
            for (unsigned i = 0; i < N; i++)
                if (!read_mont(f, wantQ[i])) return 2;
        }
        seen[want_cls]++;
        int lgN = 0;
        while ((1u << lgN) < N) lgN++;
        // the domain's tables, as poly.hip caches them
        const FrE omega = bn254_group_gen(N);
        std::vector<FrE> pw(N), inv1(N, fe_zero<F>());
        pw[0] = fe_one<F>();
        for (unsigned i = 1; i < N; i++) pw[i] = fe_mul<F>(pw[i - 1], omega);
        for (unsigned k = 1; k < N; k++) inv1[k] = fe_inv_bin<F>(fe_sub<F>(pw[k], fe_one<F>()));
        const FrE n_inv = fe_inv_bin<F>(mont_from_u64<F>(N));

        bool bad = !words_canonical<F>(zw);
        const uint32_t c = classify<F>(zw, N);
        const FrE z = fe_to_mont<F>(words_load<F>(zw));
        const FrE D = vanishing<F>(z, lgN);
        bad |= !fe_eq<F>(D, wantD);
        const int cls = c == KM_AT_N || (c == KM_OUTSIDE && fe_is_zero<F>(D)) ? 2 : c == KM_OUTSIDE ? 1 : 0;
        bad |= cls != want_cls;
        if (cls == want_cls && cls != 2) {
            // the row's buffers at their exact sizes: the sanitizer sees any index past them
            std::vector<FrE> q(N, fe_zero<F>());
            const FrE* fr = row.data();
            FrE y;
            if (cls == 0) {
                const uint32_t m = c;
                const FrE fm = row_at<F>(fr, width, m), wminv = pw[(N - m) & (N - 1)];
                FrE acc[64];
                for (uint32_t lane = 0; lane < 64; lane++)
                    acc[lane] = in_pass<F>(fr, width, pw.data(), inv1.data(), N, m, fm, wminv, lane, q.data());
                for (uint32_t s = 1; s < 64; s <<= 1) {
                    FrE nx[64];
                    for (uint32_t lane = 0; lane < 64; lane++) nx[lane] = fe_add<F>(acc[lane], acc[lane ^ s]);
                    memcpy(acc, nx, sizeof acc);
                }
                for (uint32_t lane = 1; lane < 64; lane++) bad |= !fe_eq<F>(acc[lane], acc[0]);
                q[m] = in_qm<F>(wminv, acc[m & 63u]);
                y = fm;
            } else {
                const FrE dinv = fe_inv_bin<F>(D);
                FrE tot[64], oth[64], acc[64];
                for (uint32_t lane = 0; lane < 64; lane++) {
                    tot[lane] = out_prefix_pass<F>(pw.data(), N, z, lane, q.data());
                    oth[lane] = fe_one<F>();
                }
                for (uint32_t s = 1; s < 64; s <<= 1) {
                    FrE pt[64];
                    for (uint32_t lane = 0; lane < 64; lane++) pt[lane] = tot[lane ^ s];
                    for (uint32_t lane = 0; lane < 64; lane++) others_step<F>(tot[lane], oth[lane], pt[lane]);
                }
                for (uint32_t lane = 0; lane < 64; lane++) bad |= !fe_eq<F>(tot[lane], D);  // prod (w^j - z) = z^N - 1
                for (uint32_t lane = 0; lane < 64; lane++)
                    acc[lane] = out_inverse_pass<F>(fr, width, pw.data(), N, z, fe_mul<F>(oth[lane], dinv), lane, q.data());
                for (unsigned i = 0; i < N; i++)  // the row holds 1 / (w^i - z) now
                    bad |= !fe_eq<F>(fe_mul<F>(q[i], fe_sub<F>(pw[i], z)), fe_one<F>());
                for (uint32_t s = 1; s < 64; s <<= 1) {
                    FrE nx[64];
                    for (uint32_t lane = 0; lane < 64; lane++) nx[lane] = fe_add<F>(acc[lane], acc[lane ^ s]);
                    memcpy(acc, nx, sizeof acc);
                }
                y = out_y<F>(tot[0], n_inv, acc[0]);
                for (uint32_t lane = 0; lane < 64; lane++) out_quotient_pass<F>(fr, width, N, y, lane, q.data());
            }
            bad |= !fe_eq<F>(y, wantY);
            for (unsigned i = 0; i < N; i++) bad |= !fe_eq<F>(q[i], wantQ[i]);
            rows_checked++;
        }
        if (bad) {
            wrong++;
            fprintf(stderr, "MISMATCH: case %d (N = %u, width = %u, class %d)\n", ci, N, width, want_cls);
        }
    }
    fclose(f);
    printf("{\"cases\": %d, \"wrong\": %d, \"in_domain\": %d, \"outside\": %d, \"domain_error\": %d, \"rows\": %d}\n",
           ncases, wrong, seen[0], seen[1], seen[2], rows_checked);
    return 0;
}

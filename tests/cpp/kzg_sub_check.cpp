// Host check of KZG subvector proving's arithmetic (verkle-kzg_amd/csrc/kzg_sub.hpp, the text the
// kernel of kzg_sub.hip compiles). Reads the flat dump tests/test_kzg_sub_host.py writes (argv[1]):
// per case N, width, k, the k indices, the row, the k weights c_i and the whole quotient row of
// (f - I) / Z_S. Each case runs as the wave kernel runs it: 64 lanes in a loop over the same per-lane
// functions, the xor shuffles as array reads of the partner lane's value, the scratch row of weights
// as an array of exactly k values. Every buffer has its exact size: the sanitizer sees any index
// past it.
// Prints one JSON line: cases, wrong results, weights and row entries compared.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../verkle-kzg_amd/csrc/kzg_sub.hpp"
#include "../../verkle-kzg_amd/csrc/host/fr.hpp"
using namespace vk;
using namespace vk::kzgs;
using F = BN254Fr;
using FrE = fe<F>;

static bool read_mont(FILE* f, FrE& out) {  // one hex token, up to 64 digits, below r
    char tok[80];
    if (fscanf(f, "%79s", tok) != 1) return false;
    uint32_t w[8];
    memset(w, 0, sizeof w);
    const size_t len = strlen(tok);
    if (len > 64) return false;
    for (size_t i = 0; i < len; i++) {
        const char c = tok[len - 1 - i];
        const uint32_t d = c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10;
        w[i / 8] |= d << (4 * (i % 8));
    }
    if (!kzgm::words_canonical<F>(w)) return false;
    out = fe_to_mont<F>(kzgm::words_load<F>(w));
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int ncases = 0;
    if (fscanf(f, "%d", &ncases) != 1) return 2;
    int wrong = 0;
    long weights_checked = 0, entries_checked = 0;
    for (int ci = 0; ci < ncases; ci++) {
        unsigned N, width, k;
        if (fscanf(f, "%u %u %u", &N, &width, &k) != 3) return 2;
        if (N < 2 || N > kzgm::KM_MAX_N || (N & (N - 1)) || width > N || k < 1 || k > N) return 2;
        std::vector<uint32_t> S(k);
        for (unsigned t = 0; t < k; t++)
            if (fscanf(f, "%u", &S[t]) != 1 || S[t] >= N) return 2;
        std::vector<FrE> row(width), wantC(k), wantQ(N);
        for (auto& v : row)
            if (!read_mont(f, v)) return 2;
        for (auto& v : wantC)
            if (!read_mont(f, v)) return 2;
        for (auto& v : wantQ)
            if (!read_mont(f, v)) return 2;
        // the domain's tables, as poly.hip caches them (inv1[0] = 0: the batch inversion keeps zeros)
        const FrE omega = bn254_group_gen(N);
        std::vector<FrE> pw(N), inv1(N, fe_zero<F>());
        pw[0] = fe_one<F>();
        for (unsigned i = 1; i < N; i++) pw[i] = fe_mul<F>(pw[i - 1], omega);
        for (unsigned i = 1; i < N; i++) inv1[i] = fe_inv_bin<F>(fe_sub<F>(pw[i], fe_one<F>()));

        bool bad = false;
        const FrE* fr = row.data();
        std::vector<FrE> cw(k), q(N, fe_zero<F>());
        // ---- the weights, lanes over the subset
        uint32_t part[64], sum = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            part[lane] = 0;
            for (uint32_t t = lane; t < k; t += 64) part[lane] += S[t];
        }
        for (uint32_t s = 1; s < 64; s <<= 1) {
            uint32_t nx[64];
            for (uint32_t lane = 0; lane < 64; lane++) nx[lane] = part[lane] + part[lane ^ s];
            memcpy(part, nx, sizeof part);
        }
        sum = part[0];
        for (uint32_t lane = 1; lane < 64; lane++) bad |= part[lane] != sum;
        const FrE wsum = sub_wsum<F>(pw.data(), N, sum);
        for (uint32_t lane = 0; lane < 64; lane++)
            for (uint32_t t = lane; t < k; t += 64) cw[t] = sub_weight<F>(S.data(), k, inv1.data(), N, t, wsum);
        for (unsigned t = 0; t < k; t++, weights_checked++)
            bad |= !fe_eq<F>(sub_weight_full<F>(cw[t], pw.data(), S[t]), wantC[t]);
        // ---- the row, lanes over its entries
        for (uint32_t lane = 0; lane < 64; lane++)
            for (uint32_t j = lane; j < N; j += 64)
                q[j] = sub_row_entry<F>(fr, width, S.data(), k, cw.data(), inv1.data(), N, j);
        // ---- the diagonal terms
        for (uint32_t t = 0; t < k; t++) {
            const uint32_t m = S[t];
            FrE acc[64];
            for (uint32_t lane = 0; lane < 64; lane++)
                acc[lane] = sub_diag_pass<F>(fr, width, inv1.data(), N, m, row_at<F>(fr, width, m), lane);
            for (uint32_t s = 1; s < 64; s <<= 1) {
                FrE nx[64];
                for (uint32_t lane = 0; lane < 64; lane++) nx[lane] = fe_add<F>(acc[lane], acc[lane ^ s]);
                memcpy(acc, nx, sizeof acc);
            }
            for (uint32_t lane = 1; lane < 64; lane++) bad |= !fe_eq<F>(acc[lane], acc[0]);
            q[m] = sub_diag<F>(q[m], cw[t], acc[m & 63u]);
        }
        for (unsigned j = 0; j < N; j++, entries_checked++) bad |= !fe_eq<F>(q[j], wantQ[j]);
        if (bad) {
            wrong++;
            fprintf(stderr, "MISMATCH: case %d (N = %u, width = %u, k = %u)\n", ci, N, width, k);
        }
    }
    fclose(f);
    printf("{\"cases\": %d, \"wrong\": %d, \"weights\": %ld, \"entries\": %ld}\n", ncases, wrong, weights_checked,
           entries_checked);
    return 0;
}

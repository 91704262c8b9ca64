// Host check of the IPA rounds' field arithmetic (verkle-kzg_amd/csrc/ipa_rounds.hpp, the text
// ipa.hip's provers and verifiers call), built with the sanitizers and run directly by
// tests/test_ipa_rounds_host.py. Fixed pseudo-random a, b, w and challenges; for K = 0 .. 4
// (N = 2^K), once with a dense b and once with a one-hot b (the in-domain weights):
//   * every round's rows against the definition, entry by entry, with and without the q terms
//     (the row buffers are exactly N + 1 and N long), round 0's shortcut against multiplying by one;
//   * every round's fold against a second, plain loop, and the inner product it must preserve:
//     <a', b'> = <a_L, b_R> + x (<a_L, b_L> + <a_R, b_R>) + x^2 <a_R, b_L>;
//   * the coefficients after R rounds against prod_{r < R, bit (K-1-r) of i clear} x_r, and after K
//     rounds against points_coeffs;
//   * the verifier's scalars against the batched verifier's closed forms (ipa_verify.hpp s_coeff,
//     var_scalars with scale one, as canonical words) and prod x against its return value.
// Prints one JSON line of counts.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../verkle-kzg_amd/csrc/ipa_rounds.hpp"
#include "../../verkle-kzg_amd/csrc/ipa_verify.hpp"
#include "../../verkle-kzg_amd/csrc/host/fr.hpp"
using namespace vk;
using ipar::FrE;
using Fr_ = BN254Fr;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {  // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static FrE rnd() {  // a product of four 64-bit values plus a fifth: all 254 bits in play
    FrE r = mont_from_u64<Fr_>(rng());
    for (int i = 0; i < 3; i++) r = fe_mul<Fr_>(r, mont_from_u64<Fr_>(rng()));
    return fe_add<Fr_>(r, mont_from_u64<Fr_>(rng()));
}
static FrE mul(const FrE& a, const FrE& b) { return fe_mul<Fr_>(a, b); }
static FrE add(const FrE& a, const FrE& b) { return fe_add<Fr_>(a, b); }
static FrE dot(const FrE* a, const FrE* b, size_t n) {  // plain: no entry skipped
    FrE s = fe_zero<Fr_>();
    for (size_t i = 0; i < n; i++) s = add(s, mul(a[i], b[i]));
    return s;
}

static long rows_checked = 0, rows_bad = 0, folds_checked = 0, folds_bad = 0, coeff_checked = 0, coeff_bad = 0,
            scalars_checked = 0, scalars_bad = 0, inner_checked = 0, inner_bad = 0;
static void eq(const FrE& a, const FrE& b, long& n, long& bad) {
    n++;
    if (memcmp(a.v, b.v, sizeof a.v) != 0) bad++;
}

static void run(int K, bool one_hot) {
    const size_t N = (size_t)1 << K;
    const FrE one = fe_one<Fr_>(), zero = fe_zero<Fr_>();
    std::vector<FrE> a(N), b(N, zero), xs(K), coeff(N, one);
    for (auto& v : a) v = rnd();
    if (one_hot) b[rng() % N] = one;
    else
        for (auto& v : b) v = rnd();
    const FrE w = rnd();
    for (auto& x : xs) x = rnd();

    // inner (skips b's zeros) against the plain dot: the whole vectors, and b with every other entry zero
    std::vector<FrE> bz(b);
    for (size_t i = 0; i < N; i += 2) bz[i] = zero;
    eq(ipar::inner(a.data(), b.data(), N), dot(a.data(), b.data(), N), inner_checked, inner_bad);
    eq(ipar::inner(a.data(), bz.data(), N), dot(a.data(), bz.data(), N), inner_checked, inner_bad);
    for (int r = 0; r < K; r++) {
        const size_t m = N >> r, half = m / 2;
        // rows with the q terms, and without (buffers of exactly N)
        std::vector<FrE> sL(N + 1), sR(N + 1), tL(N), tR(N);
        ipar::round_rows(a.data(), r == 0 ? nullptr : coeff.data(), N, m, half, sL.data(), sR.data(), b.data(), &w);
        ipar::round_rows(a.data(), r == 0 ? nullptr : coeff.data(), N, m, half, tL.data(), tR.data());
        for (size_t i = 0; i < N; i++) {
            const size_t j = i % m;
            // (in round 0 coeff is all one: the shortcut must give the words of the multiply)
            const FrE eL = j >= half ? mul(a[j - half], coeff[i]) : zero;
            const FrE eR = j < half ? mul(a[j + half], coeff[i]) : zero;
            eq(sL[i], eL, rows_checked, rows_bad);
            eq(sR[i], eR, rows_checked, rows_bad);
            eq(tL[i], eL, rows_checked, rows_bad);
            eq(tR[i], eR, rows_checked, rows_bad);
        }
        eq(sL[N], mul(w, dot(&a[0], &b[half], half)), rows_checked, rows_bad);
        eq(sR[N], mul(w, dot(&a[half], &b[0], half)), rows_checked, rows_bad);
        if (r == 0) {  // the shortcut against the general path given the ones
            std::vector<FrE> uL(N + 1), uR(N + 1);
            ipar::round_rows(a.data(), coeff.data(), N, m, half, uL.data(), uR.data(), b.data(), &w);
            for (size_t i = 0; i <= N; i++) {
                eq(uL[i], sL[i], rows_checked, rows_bad);
                eq(uR[i], sR[i], rows_checked, rows_bad);
            }
        }
        // the fold against a plain loop
        const FrE x = xs[r];
        std::vector<FrE> ea(half), eb(half), ec(coeff);
        for (size_t j = 0; j < half; j++) {
            ea[j] = add(a[j], mul(x, a[j + half]));
            eb[j] = add(b[j + half], mul(x, b[j]));
        }
        for (size_t i = 0; i < N; i++)
            if (i % m < half) ec[i] = mul(ec[i], x);
        const FrE want = add(add(dot(&a[0], &b[half], half), mul(x, add(dot(&a[0], &b[0], half), dot(&a[half], &b[half], half)))),
                             mul(mul(x, x), dot(&a[half], &b[0], half)));
        std::vector<FrE> a_only(a);  // the commitment proof's fold: no b
        ipar::round_fold(x, N, m, half, a_only, nullptr, nullptr);
        ipar::round_fold(x, N, m, half, a, &b, coeff.data());
        folds_checked++;
        if (a.size() != half || b.size() != half || a_only.size() != half) {
            folds_bad++;
            return;
        }
        for (size_t j = 0; j < half; j++) {
            eq(a[j], ea[j], folds_checked, folds_bad);
            eq(b[j], eb[j], folds_checked, folds_bad);
            eq(a_only[j], ea[j], folds_checked, folds_bad);
        }
        eq(dot(a.data(), b.data(), half), want, folds_checked, folds_bad);
        // the coefficients after r + 1 rounds, closed form
        for (size_t i = 0; i < N; i++) {
            eq(coeff[i], ec[i], coeff_checked, coeff_bad);
            FrE c = one;
            for (int q = 0; q <= r; q++)
                if (!((i >> (K - 1 - q)) & 1u)) c = mul(c, xs[q]);
            eq(coeff[i], c, coeff_checked, coeff_bad);
        }
    }
    // the verifier's scalars
    std::vector<FrE> s, vs;
    const FrE prodx = ipar::verifier_scalars(xs.data(), K, s, vs);
    scalars_checked++;
    if (s.size() != N || vs.size() != (size_t)(1 + 2 * K)) {
        scalars_bad++;
        return;
    }
    for (size_t i = 0; i < N; i++) {
        eq(s[i], coeff[i], coeff_checked, coeff_bad);  // K rounds of folds give points_coeffs
        eq(s[i], ipav::s_coeff(xs.data(), K, (uint32_t)i), scalars_checked, scalars_bad);
    }
    std::vector<uint32_t> words(8 * (1 + 2 * K));
    const FrE p2 = ipav::var_scalars(xs.data(), K, one, words.data());
    for (int k = 0; k < 1 + 2 * K; k++)
        eq(fe_from_mont<Fr_>(vs[k]), ipav::fr_load(&words[8 * k]), scalars_checked, scalars_bad);
    FrE p3 = one;
    for (int k = 0; k < K; k++) p3 = mul(p3, xs[k]);
    eq(prodx, p2, scalars_checked, scalars_bad);
    eq(prodx, p3, scalars_checked, scalars_bad);
    eq(prodx, vs[0], scalars_checked, scalars_bad);
}

int main() {
    int seen = 0;
    for (int K = 0; K <= 4; K++) {
        run(K, false);
        run(K, true);
        seen |= 1 << K;
    }
    printf("{\"k_seen\": %d, \"rows\": %ld, \"rows_bad\": %ld, \"folds\": %ld, \"folds_bad\": %ld, \"coeffs\": %ld, "
           "\"coeffs_bad\": %ld, \"scalars\": %ld, \"scalars_bad\": %ld, \"inner\": %ld, \"inner_bad\": %ld}\n",
           seen, rows_checked, rows_bad, folds_checked, folds_bad, coeff_checked, coeff_bad, scalars_checked,
           scalars_bad, inner_checked, inner_bad);
    return 0;
}

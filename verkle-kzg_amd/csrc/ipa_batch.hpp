// Shared text of IPA batch verification (vc_ipa_verify_batch), host + gfx950 device from one source:
// the kernels of ipa_batch.hip wrap it, the host paths of vc_ipa_challenges_many / vc_ipa_batch_fold
// run it over the host pool, and tests/cpp/ipa_batch_check.cpp runs it under the sanitizers.
//
// n openings fold with the weights rho^j sigma_j into one point. With E_j the left side of the
// identity of ipa_verify.hpp and sigma_j = 1 for a point below N, z_j^N - 1 (the product of all
// z_j - w^i, ipa_verify.hpp's un-inverted denominator) otherwise,
//   S = sum_j rho^j sigma_j E_j        accept  <=>  S is the identity.
// Grouped by base S is one fixed row of N + 1 scalars over (g, q), summed over the entries, and one
// variable-base MSM over the entries' own points (C_j, L_j0, R_j0, ..) with rho^j sigma_j times
// var_scalars' values.
//
// The per-proof Fiat-Shamir transcript of a fresh "ipa" transcript has messages of fixed length and
// layout, so it is hashed here from register words, every word position a compile-time constant:
//   w    zpad(48) "C" C(32) "input point" z(32) "output point" y(32) "w" | 00 30 00 "ipa" 03   176 B
//   x_k  zpad(48) prev(32) label "L" L_k(32) "R" R_k(32) "x"            | 00 30 00 "ipa" 03   155 B
// (prev / label: the previous canonical challenge and its label, "w" before x_0 and "x" after),
// three blocks each, then expand_message_xmd's two one-block follow-ups: b1 = H(b0 | 01 | dst'),
// b2 = H(b0 ^ b1 | 02 | dst'), the challenge b1 | b2[0..16) read big-endian and reduced mod r.
#pragma once
#include "ipa_verify.hpp"

namespace vk {
namespace ipab {

using namespace ipav;

// ---------------------------------------------------------------- SHA-256
VK_HD uint32_t rotr32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
VK_HD uint32_t sha_k(int i) {
    constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
        0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
        0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
        0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
        0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
        0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
        0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    return K[i];
}
VK_HD void sha_init(uint32_t st[8]) {
    st[0] = 0x6a09e667u, st[1] = 0xbb67ae85u, st[2] = 0x3c6ef372u, st[3] = 0xa54ff53au;
    st[4] = 0x510e527fu, st[5] = 0x9b05688cu, st[6] = 0x1f83d9abu, st[7] = 0x5be0cd19u;
}
// one block of 16 big-endian words (used up: the schedule rolls through them in place). Fully
// unrolled, so every index is a constant and the words stay in registers.
VK_HD void sha_compress(uint32_t st[8], uint32_t w[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        if (i >= 16) {
            const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            w[i & 15] += (rotr32(w15, 7) ^ rotr32(w15, 18) ^ (w15 >> 3)) + w[(i + 9) & 15] +
                         (rotr32(w2, 17) ^ rotr32(w2, 19) ^ (w2 >> 10));
        }
        const uint32_t t1 = h + (rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25)) + ((e & f) ^ (~e & g)) + sha_k(i) + w[i & 15];
        const uint32_t t2 = (rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    st[0] += a, st[1] += b, st[2] += c, st[3] += d, st[4] += e, st[5] += f, st[6] += g, st[7] += h;
}

// ---------------------------------------------------------------- message words
// A message is an array of big-endian words, zeroed by its maker; the pieces are or-ed in at constant
// byte offsets (the callers' loops unroll, so each word is a handful of shifts of register words).
VK_HD void put_byte(uint32_t* m, int off, uint32_t b) { m[off >> 2] |= b << (8 * (3 - (off & 3))); }
// 32 bytes: eight little-endian words, least significant first (a canonical field element or a
// compressed point as the transcript appends it)
VK_HD void put_le256(uint32_t* m, int off, const uint32_t* v) {
#pragma unroll
    for (int i = 0; i < 32; i++) put_byte(m, off + i, (v[i >> 2] >> (8 * (i & 3))) & 0xffu);
}
template <int L>
VK_HD void put_str(uint32_t* m, int off, const char (&s)[L]) {
#pragma unroll
    for (int i = 0; i < L - 1; i++) put_byte(m, off + i, (uint32_t)(uint8_t)s[i]);
}
// the tail of every expand_message_xmd input here: l_i_b_str = 00 30 (48 bytes out), 00, then
// dst' = "ipa" 03; then SHA-256's padding for a message of `len` bytes in `blocks` blocks
VK_HD void put_tail(uint32_t* m, int off, int len, int blocks) {
    put_byte(m, off + 1, 0x30);
    put_str(m, off + 3, "ipa");
    put_byte(m, off + 6, 3);
    put_byte(m, len, 0x80);
    m[16 * blocks - 1] = (uint32_t)len * 8;
}

// the 48 output bytes b1 | b2[0..16) of expand_message_xmd, big-endian, mod r (Montgomery): lo +
// hi 2^256, lo the low 32 bytes, hi the top 16 (shared with mp_verify.hpp's "multiproof" DST)
VK_HD FrE xmd_reduce(const uint32_t b1[8], const uint32_t b2[8]) {
    // big-endian bytes b1[0..8) b2[0..4): the least significant word is b2[3]
    FrE lo, hi = fe_zero<BN254Fr>();
    for (int i = 0; i < 4; i++) lo.v[i] = b2[3 - i];
    for (int i = 0; i < 4; i++) lo.v[4 + i] = b1[7 - i];
    for (int i = 0; i < 4; i++) hi.v[i] = b1[3 - i];
    for (int it = 0; it < 6; it++) lo = fe_reduce_once<BN254Fr>(lo);  // < 2^256 < 6r
    // hi 2^256 in Montgomery form is hi R^2: two conversions
    return fe_add<BN254Fr>(fe_to_mont<BN254Fr>(lo), fe_to_mont<BN254Fr>(fe_to_mont<BN254Fr>(hi)));
}

// expand_message_xmd's end from b0 = st (the hash of the padded message) to the field element
// (Montgomery)
VK_HD FrE xmd_finish(const uint32_t b0[8]) {
    uint32_t b1[8], b2[8], m[16];
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) m[i] = b0[i];
    put_byte(m, 32, 1);
    put_str(m, 33, "ipa");
    put_byte(m, 36, 3);
    put_byte(m, 37, 0x80);
    m[15] = 37 * 8;
    sha_init(b1);
    sha_compress(b1, m);
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) m[i] = b0[i] ^ b1[i];
    put_byte(m, 32, 2);
    put_str(m, 33, "ipa");
    put_byte(m, 36, 3);
    put_byte(m, 37, 0x80);
    m[15] = 37 * 8;
    sha_init(b2);
    sha_compress(b2, m);
    return xmd_reduce(b1, b2);
}

// compress_g1 (arkworks SWFlags) as eight little-endian words: x with bit 255 set when y > p - y;
// the identity is zero bytes with bit 254 (0x40 in byte 31). Canonical coordinates in; anything else
// gives some words and no fault.
VK_HD void compress_words(const uint32_t* xy, bool inf, uint32_t out[8]) {
    if (inf) {
        for (int i = 0; i < 8; i++) out[i] = 0;
        out[7] = 0x40000000u;
        return;
    }
    const fe<BN254Fq> y = words_load<BN254Fq>(xy + 8), ny = fe_sub<BN254Fq>(fe_zero<BN254Fq>(), y);
    bool neg = false;
    for (int k = 7; k >= 0; k--)
        if (y.v[k] != ny.v[k]) {
            neg = y.v[k] > ny.v[k];
            break;
        }
    for (int i = 0; i < 8; i++) out[i] = xy[i];
    if (neg) out[7] |= 0x80000000u;
}

// w of a fresh "ipa" transcript after C, the input point z and the output point y (compressed /
// canonical words); Montgomery
VK_HD FrE challenge_w(const uint32_t* c, const uint32_t* z, const uint32_t* y) {
    uint32_t m[48];
#pragma unroll
    for (int i = 0; i < 48; i++) m[i] = 0;
    put_str(m, 48, "C");
    put_le256(m, 49, c);
    put_str(m, 81, "input point");
    put_le256(m, 92, z);
    put_str(m, 124, "output point");
    put_le256(m, 136, y);
    put_str(m, 168, "w");
    put_tail(m, 169, 176, 3);
    uint32_t st[8];
    sha_init(st);
    sha_compress(st, m);
    sha_compress(st, m + 16);
    sha_compress(st, m + 32);
    return xmd_finish(st);
}
// x_k after the previous challenge (canonical words; its label 'w' or 'x'), L_k and R_k
VK_HD FrE challenge_x(const uint32_t* prev, uint32_t prev_label, const uint32_t* l, const uint32_t* r) {
    uint32_t m[48];
#pragma unroll
    for (int i = 0; i < 48; i++) m[i] = 0;
    put_le256(m, 48, prev);
    put_byte(m, 80, prev_label);
    put_str(m, 81, "L");
    put_le256(m, 82, l);
    put_str(m, 114, "R");
    put_le256(m, 115, r);
    put_str(m, 147, "x");
    put_tail(m, 148, 155, 3);
    uint32_t st[8];
    sha_init(st);
    sha_compress(st, m);
    sha_compress(st, m + 16);
    sha_compress(st, m + 32);
    return xmd_finish(st);
}

// [w, x_0 .. x_{K-1}] of entry p of the ABI's arrays (as 32-bit words: com_xy / l_xy / r_xy 16 per
// point, points / y 8 per entry), Montgomery, 8 (1 + K) words at `out`. Reads no more than the
// entry's own words whatever they hold.
VK_HD void entry_challenges(size_t p, int K, const uint32_t* com_xy, const uint8_t* com_inf, const uint32_t* points,
                            const uint32_t* y, const uint32_t* l_xy, const uint8_t* l_inf, const uint32_t* r_xy,
                            const uint8_t* r_inf, uint32_t* out) {
    uint32_t c[8], zw[8], yw[8];
    compress_words(com_xy + 16 * p, com_inf[p] != 0, c);
    for (int i = 0; i < 8; i++) zw[i] = points[8 * p + i], yw[i] = y[8 * p + i];
    FrE ch = challenge_w(c, zw, yw);
    fr_store(ch, out);
    for (int k = 0; k < K; k++) {
        const size_t at = p * (size_t)K + (size_t)k;
        uint32_t lw[8], rw[8];
        compress_words(l_xy + 16 * at, l_inf[at] != 0, lw);
        compress_words(r_xy + 16 * at, r_inf[at] != 0, rw);
        const FrE prev = fe_from_mont<BN254Fr>(ch);
        ch = challenge_x(prev.v, k == 0 ? 'w' : 'x', lw, rw);
        fr_store(ch, out + 8 * (1 + k));
    }
}

// ---------------------------------------------------------------- the fold
// rho^e by square-and-multiply on the index (Montgomery in and out): entry j of a chunk that starts
// at entry `first` of the call weighs rho^(first + j), so the weights continue across chunks
VK_HD FrE pow_index(const FrE& rho, uint64_t e) {
    FrE acc = fe_one<BN254Fr>(), b = rho;
    while (e) {
        if (e & 1) acc = fr_mul(acc, b);
        e >>= 1;
        if (e) b = fr_mul(b, b);
    }
    return acc;
}
// tip, y and the point canonical below r (vc_ipa_verify_many's field kernel calls the rest bad)
VK_HD bool entry_fr_ok(const uint32_t* tip, const uint32_t* y, const uint32_t* point) {
    return ate::words_below_modulus<BN254Fr>(tip) && ate::words_below_modulus<BN254Fr>(y) &&
           ate::words_below_modulus<BN254Fr>(point);
}
// a point of an entry (canonical words, identity flag) in Montgomery form; false: malformed
VK_HD bool point_load(const uint32_t* xy, bool inf, G1P& out) {
    out = G1P{fe_zero<BN254Fq>(), fe_zero<BN254Fq>()};
    return inf || ate::g1_load(xy, out);
}

// One entry's share of the fold on one thread (the host path and the check program): row[0..N] +=
// wt sigma (fixed row of E), var += the variable part; pw: the domain's powers; chal: the entry's
// Montgomery challenges. false: the entry is malformed (row and var unspecified).
template <class ScalarMul>
VK_HD bool fold_entry(size_t p, uint32_t N, int K, const uint32_t* com_xy, const uint8_t* com_inf,
                      const uint32_t* points, const uint32_t* l_xy, const uint8_t* l_inf, const uint32_t* r_xy,
                      const uint8_t* r_inf, const uint32_t* tip_w, const uint32_t* y_w, const uint32_t* chal,
                      const FrE* pw, const FrE& n_inv, const FrE& wt, FrE* row, G1A& var, ScalarMul smul) {
    const uint32_t *tw = tip_w + 8 * p, *yw = y_w + 8 * p, *zw = points + 8 * p;
    if (!entry_fr_ok(tw, yw, zw)) return false;
    FrE xs[32];
    for (int k = 0; k < K; k++) xs[k] = fr_load(chal + 8 * (1 + k));
    const FrE tip = fe_to_mont<BN254Fr>(fr_load(tw)), z = fe_to_mont<BN254Fr>(fr_load(zw));
    uint64_t idx = 0;
    const bool in_dom = point_in_domain(zw, N, &idx);
    Frac f = frac_zero();
    if (!in_dom)
        for (uint32_t i = 0; i < N; i++) f = frac_add_term(f, s_coeff(xs, K, i), pw[i], z);
    const FrE scale = in_dom ? fe_one<BN254Fr>() : f.den, sw = fr_mul(scale, wt);
    if (fe_is_zero<BN254Fr>(scale)) return false;
    const FrE mt = fr_mul(tip, sw);
    for (uint32_t i = 0; i < N; i++) row[i] = fe_add<BN254Fr>(row[i], row_entry(mt, s_coeff(xs, K, i)));
    const FrE cb = in_dom ? s_coeff(xs, K, (uint32_t)idx) : bary_dot_scaled(f, z, K, n_inv);
    uint32_t vs[8 * 65];
    const FrE prodx = var_scalars(xs, K, sw, vs);
    row[N] = fe_add<BN254Fr>(
        row[N], fr_mul(wt, row_tail(prodx, fr_load(chal), fe_to_mont<BN254Fr>(fr_load(yw)), tip, cb, scale)));
    for (int t = 0; t < 1 + 2 * K; t++) {
        const size_t at = p * (size_t)K + (size_t)((t - 1) >> 1);
        const uint32_t* xy = t == 0 ? com_xy + 16 * p : ((t - 1) & 1) ? r_xy + 16 * at : l_xy + 16 * at;
        const bool inf = (t == 0 ? com_inf[p] : ((t - 1) & 1) ? r_inf[at] : l_inf[at]) != 0;
        G1P P;
        if (!point_load(xy, inf, P)) return false;
        if (!inf) var = BN254G1::add(var, smul(P, fe_to_mont<BN254Fr>(fr_load(vs + 8 * t))));
    }
    return true;
}

}  // namespace ipab
}  // namespace vk

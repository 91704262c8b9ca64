// Shared text of multiproof batch verification (vc_multiproof_verify_many_ipa / _kzg,
// vc_multiproof_claims_many), host + gfx950 device from one source: the kernels of mp_verify.hip
// wrap it and tests/cpp/mp_verify_check.cpp runs it under the sanitizers against the library's
// host transcript.
//
// verify_multiproof (multiproof.rs:178-215) of one proof with queries (C_i, z_i, y_i), i < q, the
// point D and an inner proof:
//   r     = digest of the "multiproof" transcript over the queries           (label "r")
//   t     = digest after D                                                   (label "t")
//   E     = sum_i r^i / (t - z_i) C_i      (z_i the integer: utils.rs:57-62, mp_claim's coefficients)
//   inner = the scheme's verify of (E - D, t), for IPA over the transcript continued after E.
//
// Messages (every digest is expand_message_xmd with z_pad of 48 zero bytes -- ark-ff 0.4 passes
// len_per_elem as the block size, scheme_host.cpp -- and the tail 00 30 00 "multiproof" 0a):
//   r    zpad(48) { "C" C_i(32) "z" le64(z_i) "y" y_i(32) } x q "r" | tail        48 + 75 q + 15 B
//   t    zpad(48) r(32) "r" "D" D(32) "t" | tail                                  129 B, 3 blocks
//   w    zpad(48) t(32) "t" "E" E(32) "C" (E - D)(32) "input point" t(32)
//        "output point" y(32) "w" | tail                                          249 B, 5 blocks
//   x_k  zpad(48) prev(32) label "L" L_k(32) "R" R_k(32) "x" | tail               162 B, 3 blocks
// (points compressed, field elements canonical little-endian; prev / label: the previous canonical
// challenge and its label, "w" before x_0 and "x" after). The r message has no fixed length and its
// 75-byte records fall anywhere against the 64-byte blocks, so it goes through a byte-stream feeder
// over a 16-word block buffer the caller owns (a lane's column of LDS on the device: dynamic
// indexing of a register array would put it in scratch); the other three are fixed layouts built
// in registers like ipa_batch.hpp's challenge_w / challenge_x. Each digest ends with
// expand_message_xmd's two one-block follow-ups over dst' = "multiproof" 0a.
#pragma once
#include "ipa_batch.hpp"

namespace vk {
namespace mpv {

using namespace ipab;

// ---------------------------------------------------------------- the "multiproof" DST
VK_HD void put_dst(uint32_t* m, int off) {  // dst' = "multiproof" 0a, 11 bytes
    put_str(m, off, "multiproof");
    put_byte(m, off + 10, 10);
}
// l_i_b_str = 00 30, 00, dst', then SHA-256's padding for `len` bytes in `blocks` blocks
VK_HD void put_tail_mp(uint32_t* m, int off, int len, int blocks) {
    put_byte(m, off + 1, 0x30);
    put_dst(m, off + 3);
    put_byte(m, len, 0x80);
    m[16 * blocks - 1] = (uint32_t)len * 8;
}
// expand_message_xmd's end from b0 to the field element (Montgomery), as ipab::xmd_finish
VK_HD FrE xmd_finish_mp(const uint32_t b0[8]) {
    uint32_t b1[8], b2[8], m[16];
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) m[i] = b0[i];
    put_byte(m, 32, 1);
    put_dst(m, 33);
    put_byte(m, 44, 0x80);
    m[15] = 44 * 8;
    sha_init(b1);
    sha_compress(b1, m);
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) m[i] = b0[i] ^ b1[i];
    put_byte(m, 32, 2);
    put_dst(m, 33);
    put_byte(m, 44, 0x80);
    m[15] = 44 * 8;
    sha_init(b2);
    sha_compress(b2, m);
    return xmd_reduce(b1, b2);
}

// ---------------------------------------------------------------- byte-stream feeder
// SHA-256 over a stream of bytes. The block under construction is 16 big-endian words at
// w[0], w[stride], .. (zero where no byte has come yet); a full block is compressed at once.
struct Feed {
    uint32_t st[8];
    uint32_t* w;
    uint32_t stride;
    uint32_t n;  // bytes fed
};
VK_HD void feed_begin(Feed& f, uint32_t* w, uint32_t stride) {
    sha_init(f.st);
    f.w = w;
    f.stride = stride;
    f.n = 0;
    for (int i = 0; i < 16; i++) w[i * stride] = 0;
}
VK_HD void feed_flush(Feed& f) {
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        m[i] = f.w[i * f.stride];
        f.w[i * f.stride] = 0;
    }
    sha_compress(f.st, m);
}
VK_HD void feed_byte(Feed& f, uint32_t b) {
    const uint32_t at = f.n & 63u;
    f.w[(at >> 2) * f.stride] |= b << (8 * (3 - (at & 3u)));
    f.n++;
    if ((f.n & 63u) == 0) feed_flush(f);
}
// four bytes, the most significant byte of `be` first, at any alignment
VK_HD void feed_be32(Feed& f, uint32_t be) {
    const uint32_t at = f.n & 63u, i = at >> 2, sh = 8 * (at & 3u);
    f.w[i * f.stride] |= be >> sh;
    f.n += 4;
    if (i == 15) feed_flush(f);  // (the block's last word: full, or full once the bytes below are in)
    if (sh) f.w[((i + 1) & 15u) * f.stride] |= be << (32 - sh);
}
VK_HD uint32_t bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }
// 32 bytes: eight little-endian words, least significant first
VK_HD void feed_le256(Feed& f, const uint32_t* v) {
    for (int i = 0; i < 8; i++) feed_be32(f, bswap32(v[i]));
}
// the tail and SHA-256's padding; afterwards f.st is b0
VK_HD void feed_finish(Feed& f) {
    feed_byte(f, 0);
    feed_byte(f, 0x30);
    feed_byte(f, 0);
    const char dst[] = "multiproof";
#pragma unroll
    for (int i = 0; i < 10; i++) feed_byte(f, (uint32_t)(uint8_t)dst[i]);
    feed_byte(f, 10);
    const uint32_t len = f.n;
    feed_byte(f, 0x80);
    if ((f.n & 63u) > 56) feed_flush(f);  // no room for the length: it goes into a block of its own
    f.w[15 * f.stride] = len * 8;         // (len < 2^29: the length's high word stays zero)
    feed_flush(f);
}

// ---------------------------------------------------------------- r and t
// r (Montgomery) of a proof's q queries. com_xy 16 words per point, z two words per query (a u64),
// y 8 words per query, all canonical. y_ok: every y_i below the modulus. Reads only the proof's own
// words whatever they hold.
VK_HD FrE challenge_r(uint32_t* w, uint32_t stride, uint32_t q, const uint32_t* com_xy, const uint8_t* com_inf,
                      const uint32_t* z, const uint32_t* y, bool& y_ok) {
    Feed f;
    feed_begin(f, w, stride);
    for (int i = 0; i < 12; i++) feed_be32(f, 0);  // z_pad
    y_ok = true;
    for (uint32_t i = 0; i < q; i++) {
        uint32_t c[8], yw[8];
        compress_words(com_xy + 16 * (size_t)i, com_inf[i] != 0, c);
        for (int k = 0; k < 8; k++) yw[k] = y[8 * (size_t)i + k];
        y_ok = y_ok && ate::words_below_modulus<BN254Fr>(yw);
        feed_byte(f, 'C');
        feed_le256(f, c);
        feed_byte(f, 'z');
        feed_be32(f, bswap32(z[2 * (size_t)i]));
        feed_be32(f, bswap32(z[2 * (size_t)i + 1]));
        feed_byte(f, 'y');
        feed_le256(f, yw);
    }
    feed_byte(f, 'r');
    feed_finish(f);
    return xmd_finish_mp(f.st);
}
// t (Montgomery) after r (canonical words) and D (compressed)
VK_HD FrE challenge_t(const uint32_t* r, const uint32_t* d) {
    uint32_t m[48];
#pragma unroll
    for (int i = 0; i < 48; i++) m[i] = 0;
    put_le256(m, 48, r);
    put_str(m, 80, "r");
    put_str(m, 81, "D");
    put_le256(m, 82, d);
    put_str(m, 114, "t");
    put_tail_mp(m, 115, 129, 3);
    uint32_t st[8];
    sha_init(st);
    sha_compress(st, m);
    sha_compress(st, m + 16);
    sha_compress(st, m + 32);
    return xmd_finish_mp(st);
}

// ---------------------------------------------------------------- the inner IPA's challenges
// w from the state t "t" "E" E: t, y canonical words; e, c = E and E - D compressed
VK_HD FrE inner_w(const uint32_t* t, const uint32_t* e, const uint32_t* c, const uint32_t* y) {
    uint32_t m[80];
#pragma unroll
    for (int i = 0; i < 80; i++) m[i] = 0;
    put_le256(m, 48, t);
    put_str(m, 80, "t");
    put_str(m, 81, "E");
    put_le256(m, 82, e);
    put_str(m, 114, "C");
    put_le256(m, 115, c);
    put_str(m, 147, "input point");
    put_le256(m, 158, t);
    put_str(m, 190, "output point");
    put_le256(m, 202, y);
    put_str(m, 234, "w");
    put_tail_mp(m, 235, 249, 5);
    uint32_t st[8];
    sha_init(st);
#pragma unroll
    for (int b = 0; b < 5; b++) sha_compress(st, m + 16 * b);
    return xmd_finish_mp(st);
}
// x_k after the previous challenge (canonical words; its label 'w' or 'x'), L_k and R_k compressed
VK_HD FrE inner_x(const uint32_t* prev, uint32_t prev_label, const uint32_t* l, const uint32_t* r) {
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
    put_tail_mp(m, 148, 162, 3);
    uint32_t st[8];
    sha_init(st);
    sha_compress(st, m);
    sha_compress(st, m + 16);
    sha_compress(st, m + 32);
    return xmd_finish_mp(st);
}
// [w, x_0 .. x_{K-1}] (Montgomery, 8 (1 + K) words at out) of one proof: l_xy / r_xy its K points
// (16 canonical words each), l_inf / r_inf their flags
VK_HD void inner_challenges(int K, const uint32_t* t, const uint32_t* e, const uint32_t* c, const uint32_t* y,
                            const uint32_t* l_xy, const uint8_t* l_inf, const uint32_t* r_xy, const uint8_t* r_inf,
                            uint32_t* out) {
    FrE ch = inner_w(t, e, c, y);
    fr_store(ch, out);
    for (int k = 0; k < K; k++) {
        uint32_t lw[8], rw[8];
        compress_words(l_xy + 16 * (size_t)k, l_inf[k] != 0, lw);
        compress_words(r_xy + 16 * (size_t)k, r_inf[k] != 0, rw);
        const FrE prev = fe_from_mont<BN254Fr>(ch);
        ch = inner_x(prev.v, k == 0 ? 'w' : 'x', lw, rw);
        fr_store(ch, out + 8 * (1 + k));
    }
}

// ---------------------------------------------------------------- coefficients
// coef_i = r^i / (t - z_i) over a proof's q queries on 64 lanes: lane l owns i = l, l + 64, ..
// One inversion per proof: every lane multiplies its own denominators from the back (pass 1, the
// suffix products parked in coef), the lanes' totals are multiplied together with each lane keeping
// the product of the others (kzgm::others_step over xor shuffles on the device), the one total is
// inverted, and pass 2 walks forward: 1 / d_i = inv * suffix_i, inv *= d_i, with r^i stepping by
// r^64 from r^l. A zero denominator (t equal to a z_i) counts as 1 and sets `bad`.
VK_HD FrE coef_denom(const FrE& t, const uint32_t* z, uint32_t i, bool& bad) {
    FrE zi = fe_zero<BN254Fr>();
    zi.v[0] = z[2 * (size_t)i];
    zi.v[1] = z[2 * (size_t)i + 1];
    const FrE d = fe_sub<BN254Fr>(t, fe_to_mont<BN254Fr>(zi));
    if (fe_is_zero<BN254Fr>(d)) {
        bad = true;
        return fe_one<BN254Fr>();
    }
    return d;
}
// pass 1: the lane's total (1 for a lane with no query); coef[i] <- prod of the lane's d_j, j > i
VK_HD FrE coef_suffix_pass(uint32_t q, uint32_t lane, const FrE& t, const uint32_t* z, uint32_t* coef, bool& bad) {
    FrE suf = fe_one<BN254Fr>();
    if (lane >= q) return suf;
    for (uint32_t i = lane + ((q - 1 - lane) / 64) * 64;; i -= 64) {
        fr_store(suf, coef + 8 * (size_t)i);
        suf = fr_mul(suf, coef_denom(t, z, i, bad));
        if (i == lane) break;
    }
    return suf;
}
// pass 2: inv = 1 / (the lane's total); coef[i] <- r^i / d_i as canonical words
VK_HD void coef_finish_pass(uint32_t q, uint32_t lane, const FrE& t, const uint32_t* z, const FrE& r, const FrE& r64,
                            FrE inv, uint32_t* coef) {
    FrE rp = pow_index(r, lane);
    bool bad = false;
    for (uint32_t i = lane; i < q; i += 64) {
        const FrE c = fr_mul(inv, fr_load(coef + 8 * (size_t)i));
        inv = fr_mul(inv, coef_denom(t, z, i, bad));
        fr_store(fe_from_mont<BN254Fr>(fr_mul(c, rp)), coef + 8 * (size_t)i);
        rp = fr_mul(rp, r64);
    }
}

// ---------------------------------------------------------------- claims
// E (an accumulator) and D (Montgomery affine or the identity) to what the inner verifier reads: E
// compressed (e), E - D as canonical affine words (c_xy zero for the identity) with its flag, and
// E - D compressed (c). Two inversions, the binary one (a lane's own: nothing crosses lanes).
VK_HD void fq_store(const fe<BN254Fq>& a, uint32_t* w) {
    for (int i = 0; i < 8; i++) w[i] = a.v[i];
}
VK_HD void claim_of(const G1A& E, const G1P& D, bool d_inf, uint32_t e[8], uint32_t c_xy[16], bool& c_inf,
                    uint32_t c[8]) {
    uint32_t exy[16];
    fe<BN254Fq> x, y;
    const bool e_inf = !BN254G1::to_aff<true>(E, x, y);
    for (int k = 0; k < 16; k++) exy[k] = 0;
    if (!e_inf) {
        fq_store(fe_from_mont<BN254Fq>(x), exy);
        fq_store(fe_from_mont<BN254Fq>(y), exy + 8);
    }
    compress_words(exy, e_inf, e);
    const G1A Cl = d_inf ? E : BN254G1::madd(E, D, true);
    c_inf = !BN254G1::to_aff<true>(Cl, x, y);
    for (int k = 0; k < 16; k++) c_xy[k] = 0;
    if (!c_inf) {
        fq_store(fe_from_mont<BN254Fq>(x), c_xy);
        fq_store(fe_from_mont<BN254Fq>(y), c_xy + 8);
    }
    compress_words(c_xy, c_inf, c);
}

}  // namespace mpv
}  // namespace vk

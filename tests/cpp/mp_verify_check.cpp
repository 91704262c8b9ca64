// Host check of multiproof batch verification's shared text (verkle-kzg_amd/csrc/mp_verify.hpp,
// what the kernels of mp_verify.hip wrap), linked with the library's host transcript
// (csrc/scheme_host.cpp). Checks
//   * the byte-stream feeder: r and t of Q = 1 .. 130 queries (every residue of the message length
//     mod 64, the paddings that need an extra block among them; points with the sign bit and with the
//     identity flag) against vc_transcript_* over the same triples;
//   * the inner IPA's challenge layouts for K = 1 .. 8 against a vc_transcript advanced from the same
//     prior state;
//   * the coefficients r^i / (t - z_i) of the 64-lane passes against a plain loop, Q in
//     {1, 63, 64, 65, 130}.
// Prints one JSON line of counts.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vc_scheme.h"
#include "../../verkle-kzg_amd/csrc/mp_verify.hpp"
using namespace vk;
using namespace vk::mpv;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static void rnd_words(uint32_t* w) {  // below 2^252: canonical in Fq and Fr
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)rnd();
    w[7] &= 0x0fffffffu;
}
struct Queries {
    std::vector<uint32_t> com, z, y;
    std::vector<uint8_t> inf;
    uint32_t d[16];
    uint8_t d_inf;
    int signs = 0, idents = 0;
    explicit Queries(uint32_t q, uint32_t N) : com(16 * q), z(2 * q), y(8 * q), inf(q) {
        for (uint32_t i = 0; i < q; i++) {
            rnd_words(&com[16 * i]);
            rnd_words(&com[16 * i + 8]);
            if (rnd() & 1) com[16 * i + 15] |= 0x20000000u;  // y above p / 2 (still below p): the sign bit
            rnd_words(&y[8 * i]);
            inf[i] = (rnd() % 7) == 0;
            z[2 * i] = (uint32_t)(rnd() % N);
            z[2 * i + 1] = 0;
            if (i > 0 && rnd() % 5 == 0) z[2 * i] = z[2 * (i - 1)];  // a repeated point
            uint32_t c[8];
            compress_words(&com[16 * i], inf[i] != 0, c);
            signs += (c[7] >> 31) & 1;
            idents += inf[i];
        }
        rnd_words(d);
        rnd_words(d + 8);
        d_inf = (rnd() % 9) == 0;
    }
};
static const uint64_t* u64p(const uint32_t* w) { return reinterpret_cast<const uint64_t*>(w); }

// the library's transcript up to r (and, with D, t); canonical words out; the handle positioned after "t"
static vc_transcript* host_rt(const Queries& qs, uint32_t q, uint32_t r_out[8], uint32_t t_out[8]) {
    vc_transcript* tr = vc_transcript_new("multiproof");
    for (uint32_t i = 0; i < q; i++) {
        vc_transcript_append_point(tr, u64p(&qs.com[16 * i]), qs.inf[i], "C");
        vc_transcript_append_u64(tr, (uint64_t)qs.z[2 * i] | ((uint64_t)qs.z[2 * i + 1] << 32), "z");
        vc_transcript_append_fr(tr, u64p(&qs.y[8 * i]), "y");
    }
    uint64_t out[4];
    vc_transcript_digest(tr, "r", out);
    memcpy(r_out, out, 32);
    vc_transcript_append_point(tr, u64p(qs.d), qs.d_inf, "D");
    vc_transcript_digest(tr, "t", out);
    memcpy(t_out, out, 32);
    return tr;
}

int main() {
    int feeder = 0, feeder_bad = 0, residues = 0, signs = 0, idents = 0;
    int inner = 0, inner_bad = 0, coefs = 0, coefs_bad = 0, zero_denoms = 0;
    bool seen[64] = {false};
    // ---- feeder
    for (uint32_t q = 1; q <= 130; q++) {
        Queries qs(q, 256);
        uint32_t r_want[8], t_want[8];
        vc_transcript_free(host_rt(qs, q, r_want, t_want));
        uint32_t blk[16];
        bool y_ok = false;
        const FrE r = fe_from_mont<BN254Fr>(challenge_r(blk, 1, q, qs.com.data(), qs.inf.data(), qs.z.data(), qs.y.data(), y_ok));
        uint32_t dc[8];
        compress_words(qs.d, qs.d_inf != 0, dc);
        const FrE t = fe_from_mont<BN254Fr>(challenge_t(r.v, dc));
        feeder += 2;
        feeder_bad += memcmp(r.v, r_want, 32) != 0;
        feeder_bad += memcmp(t.v, t_want, 32) != 0;
        feeder_bad += !y_ok;
        const uint32_t len = 48 + 75 * q + 15;
        if (!seen[len & 63]) seen[len & 63] = true, residues++;
        signs += qs.signs, idents += qs.idents;
    }
    {  // a y_i >= r is reported
        Queries qs(3, 8);
        for (int k = 0; k < 8; k++) qs.y[8 + k] = 0xffffffffu;
        uint32_t blk[16];
        bool y_ok = true;
        (void)challenge_r(blk, 1, 3, qs.com.data(), qs.inf.data(), qs.z.data(), qs.y.data(), y_ok);
        feeder_bad += y_ok;
    }
    // ---- the inner IPA's challenges
    for (int K = 1; K <= 8; K++) {
        const uint32_t q = 3 + (uint32_t)K;
        Queries qs(q, 1u << K);
        uint32_t r_w[8], t_w[8];
        vc_transcript* tr = host_rt(qs, q, r_w, t_w);
        uint32_t E[16], Cl[16], y[8];
        std::vector<uint32_t> l(16 * K), r(16 * K);
        std::vector<uint8_t> li(K), ri(K);
        rnd_words(E), rnd_words(E + 8), rnd_words(Cl), rnd_words(Cl + 8), rnd_words(y);
        const uint8_t e_inf = K == 3, c_inf = K == 5;
        for (int k = 0; k < K; k++) {
            rnd_words(&l[16 * k]), rnd_words(&l[16 * k + 8]), rnd_words(&r[16 * k]), rnd_words(&r[16 * k + 8]);
            li[k] = (k == 2), ri[k] = (k == 4);
        }
        std::vector<uint32_t> want(8 * (1 + K)), got(8 * (1 + K));
        uint64_t out[4];
        vc_transcript_append_point(tr, u64p(E), e_inf, "E");
        vc_transcript_append_point(tr, u64p(Cl), c_inf, "C");
        vc_transcript_append_fr(tr, u64p(t_w), "input point");
        vc_transcript_append_fr(tr, u64p(y), "output point");
        vc_transcript_digest(tr, "w", out);
        memcpy(&want[0], out, 32);
        for (int k = 0; k < K; k++) {
            vc_transcript_append_point(tr, u64p(&l[16 * k]), li[k], "L");
            vc_transcript_append_point(tr, u64p(&r[16 * k]), ri[k], "R");
            vc_transcript_digest(tr, "x", out);
            memcpy(&want[8 * (1 + k)], out, 32);
        }
        vc_transcript_free(tr);
        uint32_t ec[8], cc[8];
        compress_words(E, e_inf != 0, ec);
        compress_words(Cl, c_inf != 0, cc);
        inner_challenges(K, t_w, ec, cc, y, l.data(), li.data(), r.data(), ri.data(), got.data());
        for (int k = 0; k <= K; k++) {
            const FrE c = fe_from_mont<BN254Fr>(fr_load(&got[8 * k]));
            inner++;
            inner_bad += memcmp(c.v, &want[8 * k], 32) != 0;
        }
    }
    // ---- coefficients
    const uint32_t qlist[5] = {1, 63, 64, 65, 130};
    for (uint32_t q : qlist) {
        Queries qs(q, 256);
        FrE r, t;
        rnd_words(r.v), rnd_words(t.v);
        r = fe_to_mont<BN254Fr>(r), t = fe_to_mont<BN254Fr>(t);
        std::vector<uint32_t> coef(8 * q);
        FrE tot[64];
        bool bad = false;
        for (uint32_t lane = 0; lane < 64; lane++) tot[lane] = coef_suffix_pass(q, lane, t, qs.z.data(), coef.data(), bad);
        FrE all = fe_one<BN254Fr>();
        for (uint32_t lane = 0; lane < 64; lane++) all = fr_mul(all, tot[lane]);
        const FrE inv_all = fe_inv_bin<BN254Fr>(all), r64 = pow_index(r, 64);
        for (uint32_t lane = 0; lane < 64; lane++) {
            FrE oth = fe_one<BN254Fr>();
            for (uint32_t o = 0; o < 64; o++)
                if (o != lane) oth = fr_mul(oth, tot[o]);
            coef_finish_pass(q, lane, t, qs.z.data(), r, r64, fr_mul(inv_all, oth), coef.data());
        }
        FrE rp = fe_one<BN254Fr>();
        for (uint32_t i = 0; i < q; i++) {
            FrE zi = fe_zero<BN254Fr>();
            zi.v[0] = qs.z[2 * i];
            const FrE want =
                fe_from_mont<BN254Fr>(fr_mul(rp, fe_inv_bin<BN254Fr>(fe_sub<BN254Fr>(t, fe_to_mont<BN254Fr>(zi)))));
            coefs++;
            coefs_bad += memcmp(want.v, &coef[8 * i], 32) != 0;
            rp = fr_mul(rp, r);
        }
        coefs_bad += bad;
    }
    {  // t equal to a query point: reported, nothing divides by zero
        Queries qs(5, 8);
        FrE t = fe_zero<BN254Fr>();
        t.v[0] = qs.z[2 * 3];
        t = fe_to_mont<BN254Fr>(t);
        std::vector<uint32_t> coef(8 * 5);
        bool bad = false;
        for (uint32_t lane = 0; lane < 64; lane++) (void)coef_suffix_pass(5, lane, t, qs.z.data(), coef.data(), bad);
        zero_denoms += bad;
    }
    printf("{\"feeder\": %d, \"feeder_bad\": %d, \"residues\": %d, \"signs\": %d, \"idents\": %d, \"inner\": %d, "
           "\"inner_bad\": %d, \"coefs\": %d, \"coefs_bad\": %d, \"zero_denoms\": %d}\n",
           feeder, feeder_bad, residues, signs, idents, inner, inner_bad, coefs, coefs_bad, zero_denoms);
    return 0;
}

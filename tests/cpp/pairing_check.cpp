// Host check of the BN254 pairing tower (verkle-kzg_amd/csrc/pairing.hpp): Fq2 / Fq6 / Fq12
// products against schoolbook products over the basis 1, w, .., w^5 (w^6 = xi), squares against
// products, inverses, the Frobenius maps against a^p, the cyclotomic squaring against the plain
// one, the sparse line product against the plain one, and the pairing itself: e(G, H) != 1,
// e(G, H)^r == 1, e(aG, bH) == e(G, H)^(ab) for seeded a, b, the precomputed-line Miller loop
// against the on-the-fly one (affine and projective G1 operands), and the identity operands.
// Prints one JSON line: comparisons made and mismatches.
#include <cstdint>
#include <cstdio>

#include "../../verkle-kzg_amd/csrc/pairing.hpp"
using namespace vk;
using namespace vk::bn;

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {
    rs ^= rs << 13;
    rs ^= rs >> 7;
    rs ^= rs << 17;
    return rs;
}
template <class F>
static fe<F> rnd_fe() {  // a random residue (Montgomery form of something)
    fe<F> r;
    for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)rnd64();
    r.v[7] &= 0x0fffffffu;  // below p
    return r;
}
static Fq2 rnd2() { return Fq2{rnd_fe<BN254Fq>(), rnd_fe<BN254Fq>()}; }
static Fq6 rnd6() { return Fq6{rnd2(), rnd2(), rnd2()}; }
static Fq12 rnd12() { return Fq12{rnd6(), rnd6()}; }

static int checks = 0, bad = 0;
static void expect(bool ok, const char* what) {
    checks++;
    if (!ok) {
        bad++;
        fprintf(stderr, "MISMATCH: %s\n", what);
    }
}

// ---- schoolbook
static Fq2 sb2(const Fq2& a, const Fq2& b) {
    return Fq2{fq_sub(fq_mul(a.c0, b.c0), fq_mul(a.c1, b.c1)), fq_add(fq_mul(a.c0, b.c1), fq_mul(a.c1, b.c0))};
}
static Fq2 xi() {
    Fq2 r = fq2_zero();
    r.c0.v[0] = 9;
    r.c1.v[0] = 1;
    return Fq2{fe_to_mont<BN254Fq>(r.c0), fe_to_mont<BN254Fq>(r.c1)};
}
static Fq6 sb6(const Fq6& a, const Fq6& b) {
    const Fq2 A[3] = {a.c0, a.c1, a.c2}, B[3] = {b.c0, b.c1, b.c2};
    Fq2 c[3] = {fq2_zero(), fq2_zero(), fq2_zero()};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            Fq2 t = sb2(A[i], B[j]);
            if (i + j >= 3) t = sb2(t, xi());
            c[(i + j) % 3] = fq2_add(c[(i + j) % 3], t);
        }
    return Fq6{c[0], c[1], c[2]};
}
static Fq12 sb12(const Fq12& a, const Fq12& b) {
    Fq12 r{fq6_zero(), fq6_zero()};
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            Fq2 t = sb2(fq12_coef(a, i), fq12_coef(b, j));
            if (i + j >= 6) t = sb2(t, xi());
            Fq2& dst = fq12_coef(r, (i + j) % 6);
            dst = fq2_add(dst, t);
        }
    return r;
}
static bool eq6(const Fq6& a, const Fq6& b) { return fq2_eq(a.c0, b.c0) && fq2_eq(a.c1, b.c1) && fq2_eq(a.c2, b.c2); }

static Fq12 pow12(const Fq12& a, const uint32_t* e, int words) {
    Fq12 r = fq12_one();
    for (int i = words - 1; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            r = fq12_sqr(r);
            if ((e[i] >> b) & 1) r = fq12_mul(r, a);
        }
    return r;
}

using G1 = BN254G1;
static G1::Aff g1_gen() {
    fe<BN254Fq> x = fe_zero<BN254Fq>(), y = fe_zero<BN254Fq>();
    x.v[0] = 1;
    y.v[0] = 2;
    return G1::Aff{fe_to_mont<BN254Fq>(x), fe_to_mont<BN254Fq>(y)};
}
static G1::Acc g1_mul(const G1::Aff& p, const uint32_t* k) {
    G1::Acc r = G1::zero();
    for (int i = 7; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            r = G1::dbl(r);
            if ((k[i] >> b) & 1) r = G1::madd(r, p, false);
        }
    return r;
}
static G1Eval eval_affine_of(const G1::Acc& a) {
    fe<BN254Fq> x, y;
    const bool ok = G1::to_aff<true>(a, x, y);
    return ok ? g1_eval_aff(x, y, false) : g1_eval_aff(fe_zero<BN254Fq>(), fe_zero<BN254Fq>(), true);
}
static Fq12 pairing(const G1Eval& P, const G2Aff& Q) { return final_exp(miller_loop(P, Q)); }

int main() {
    for (int it = 0; it < 20; it++) {
        const Fq2 a = rnd2(), b = rnd2();
        expect(fq2_eq(fq2_mul(a, b), sb2(a, b)), "fq2 mul");
        expect(fq2_eq(fq2_sqr(a), fq2_mul(a, a)), "fq2 sqr");
        expect(fq2_eq(fq2_mul(a, fq2_inv(a)), fq2_one()), "fq2 inv");
        expect(fq2_eq(fq2_mul_xi(a), sb2(a, xi())), "fq2 mul xi");
        const Fq6 c = rnd6(), d = rnd6();
        expect(eq6(fq6_mul(c, d), sb6(c, d)), "fq6 mul");
        expect(eq6(fq6_sqr(c), fq6_mul(c, c)), "fq6 sqr");
        expect(eq6(fq6_mul(c, fq6_inv(c)), fq6_one()), "fq6 inv");
        expect(eq6(fq6_mul_01(c, a, b), sb6(c, Fq6{a, b, fq2_zero()})), "fq6 mul_01");
        expect(eq6(fq6_mul_v(c), sb6(c, Fq6{fq2_zero(), fq2_one(), fq2_zero()})), "fq6 mul v");
        const Fq12 e = rnd12(), f = rnd12();
        expect(fq12_eq(fq12_mul(e, f), sb12(e, f)), "fq12 mul");
        expect(fq12_eq(fq12_sqr(e), fq12_mul(e, e)), "fq12 sqr");
        expect(fq12_is_one(fq12_mul(e, fq12_inv(e))), "fq12 inv");
        // the sparse line product
        const LineCoef l{a, b};
        const G1Eval P{rnd_fe<BN254Fq>(), rnd_fe<BN254Fq>(), rnd_fe<BN254Fq>(), false};
        expect(fq12_eq(fq12_mul_line(e, l, P), sb12(e, line_as_fq12(l, P))), "line product");
    }
    {  // Frobenius: a^p, composition, order 12
        uint32_t p[8];
        for (int i = 0; i < 8; i++) p[i] = BN254Fq::p(i);
        for (int it = 0; it < 2; it++) {
            const Fq12 a = rnd12();
            const Fq12 f1 = fq12_frob(a, 1);
            expect(fq12_eq(f1, pow12(a, p, 8)), "frob1 == a^p");
            expect(fq12_eq(fq12_frob(a, 2), fq12_frob(f1, 1)), "frob2 == frob1^2");
            expect(fq12_eq(fq12_frob(a, 3), fq12_frob(fq12_frob(a, 2), 1)), "frob3 == frob1^3");
            Fq12 t = a;
            for (int k = 0; k < 12; k++) t = fq12_frob(t, 1);
            expect(fq12_eq(t, a), "frob^12 == id");
            t = a;
            for (int k = 0; k < 6; k++) t = fq12_frob(t, 2);
            expect(fq12_eq(t, a), "frob2^6 == id");
            t = a;
            for (int k = 0; k < 4; k++) t = fq12_frob(t, 3);
            expect(fq12_eq(t, a), "frob3^4 == id");
        }
    }
    for (int it = 0; it < 4; it++) {  // the cyclotomic squaring, on elements the easy part produces
        Fq12 u = final_exp_easy(rnd12());
        for (int k = 0; k < 3; k++) {
            expect(fq12_eq(fq12_cyc_sqr(u), fq12_sqr(u)), "cyclotomic square == square");
            expect(fq12_is_one(fq12_mul(u, fq12_conj(u))), "unitary after the easy part");
            u = fq12_cyc_sqr(u);
        }
    }
    const G2Aff H = g2_generator();
    expect(g2_on_twist(H), "H on the twist");
    expect(g2_in_subgroup(H), "r H == O");
    {
        G2Aff off = H;
        off.y = fq2_add(off.y, fq2_one());
        expect(!g2_on_twist(off), "H + (0, 1) off the twist");
    }
    const G1::Aff G = g1_gen();
    const G1Eval Ge = g1_eval_aff(G.x, G.y, false);
    const Fq12 eGH = pairing(Ge, H);
    uint32_t r[8];
    for (int i = 0; i < 8; i++) r[i] = BN254Fr::p(i);
    expect(!fq12_is_one(eGH), "e(G, H) != 1");
    expect(fq12_is_one(pow12(eGH, r, 8)), "e(G, H)^r == 1");
    expect(fq12_is_one(pairing(g1_eval_aff(G.x, G.y, true), H)), "e(O, H) == 1");
    expect(fq12_is_one(pairing(Ge, G2Aff{fq2_zero(), fq2_zero(), true})), "e(G, O) == 1");
    for (int it = 0; it < 8; it++) {
        const fe<BN254Fr> a = fe_from_mont<BN254Fr>(rnd_fe<BN254Fr>()), b = fe_from_mont<BN254Fr>(rnd_fe<BN254Fr>());
        const fe<BN254Fr> ab = fe_from_mont<BN254Fr>(fe_mul<BN254Fr>(fe_to_mont<BN254Fr>(a), fe_to_mont<BN254Fr>(b)));
        const G1::Acc aG = g1_mul(G, a.v);
        const G2Aff bH = g2_mul(H, b.v, 8);
        expect(g2_on_twist(bH) && !bH.inf, "b H on the twist");
        const Fq12 lhs = pairing(eval_affine_of(aG), bH);
        expect(fq12_eq(lhs, pow12(eGH, ab.v, 8)), "e(aG, bH) == e(G, H)^(ab)");
        // projective G1 operand: the same value after the final exponentiation
        expect(fq12_eq(pairing(g1_eval_acc(aG), bH), lhs), "projective operand");
        // precomputed lines, two pairings on one accumulator
        LineCoef tab0[PC::ATE_LINES], tab1[PC::ATE_LINES];
        ate_line_table(bH, tab0);
        ate_line_table(H, tab1);
        const G1Eval P0 = eval_affine_of(aG), P1 = g1_eval_acc(g1_mul(G, b.v));
        const Fq12 m = miller_loop_tab2(P0, tab0, P1, tab1);
        expect(fq12_eq(m, fq12_mul(miller_loop(P0, bH), miller_loop(P1, H))), "table Miller loop == on the fly");
        // e(aG, bH) e(-(ab) G, H) == 1, and not with ab + 1
        fe<BN254Fr> ab1 = ab;
        ab1.v[0] ^= 1;
        const G1Eval N0 = g1_eval_acc(G1::neg(g1_mul(G, ab.v))), N1 = g1_eval_acc(G1::neg(g1_mul(G, ab1.v)));
        expect(fq12_is_one(final_exp(miller_loop_tab2(P0, tab0, N0, tab1))), "product check accepts");
        expect(!fq12_is_one(final_exp(miller_loop_tab2(P0, tab0, N1, tab1))), "product check rejects");
        const G1Eval Ps[2] = {P0, N0};
        const G2Aff Qs[2] = {bH, H};
        expect(pairing_product_is_one(2, Ps, Qs), "pairing_product_is_one");
    }
    printf("{\"checks\": %d, \"mismatches\": %d}\n", checks, bad);
    return bad ? 1 : 0;
}

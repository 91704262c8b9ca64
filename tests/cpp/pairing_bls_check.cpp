// Host check of the BLS12-381 pairing tower (verkle-kzg_amd/csrc/pairing_bls.hpp): Fq2 / Fq6 /
// Fq12 products against schoolbook products over the basis 1, w, .., w^5 (w^6 = xi = 1 + u),
// squares against products, inverses, the Frobenius maps against a^p, the cyclotomic squaring
// against the plain one, the sparse line product (the M-type twist's shape) against the plain one,
// the pairing itself: e(G, H) != 1, e(G, H)^r == 1, e(aG, bH) == e(G, H)^(ab) for seeded a, b, the
// precomputed-line Miller loop against the on-the-fly one, the G1 subgroup test against a raw
// [r] P on 8 points inside and 8 outside G1, and kzg_check on a valid and a tampered opening of a
// polynomial committed with a known secret, with the cofactor attack (pi + T, T of small order).
// Built with -DVK_BLS_NO_SUBGROUP_TEST the last case reports "accepted": the number the Python test
// reads to show that the subgroup test is what rejects it.
// Prints one JSON line: comparisons made, mismatches, and the cofactor case's verdict.
#include <cstdint>
#include <cstdio>

#include "../../verkle-kzg_amd/csrc/pairing_bls.hpp"
using namespace vk;
using namespace vk::bls;

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
    for (int i = 0; i < F::N; i++) r.v[i] = (uint32_t)rnd64();
    r.v[F::N - 1] &= 0x0fffffffu;  // below p (both moduli have a top limb above 2^28)
    return r;
}
static Fq rndq() { return rnd_fe<BLS381Fq>(); }
static Fq2 rnd2() { return Fq2{rndq(), rndq()}; }
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
static Fq small(uint32_t k) {
    Fq r = fe_zero<BLS381Fq>();
    r.v[0] = k;
    return fe_to_mont<BLS381Fq>(r);
}
static Fq2 sb2(const Fq2& a, const Fq2& b) {
    return Fq2{fq_sub(fq_mul(a.c0, b.c0), fq_mul(a.c1, b.c1)), fq_add(fq_mul(a.c0, b.c1), fq_mul(a.c1, b.c0))};
}
static Fq2 xi() { return Fq2{small(1), small(1)}; }
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

using G1 = BLS381G1;
static G1::Aff g1_gen() { return G1::Aff{g1_const(0), g1_const(1)}; }
// k P by a raw ladder over ec.hpp's group law: no reduction of k, so it does cofactor work
static G1::Acc g1_mul(const G1::Aff& p, const uint32_t* k, int words = 8) {
    G1::Acc r = G1::zero();
    for (int i = words - 1; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            r = G1::dbl(r);
            if ((k[i] >> b) & 1) r = G1::madd(r, p, false);
        }
    return r;
}
static bool aff_of(const G1::Acc& a, G1::Aff& out) { return G1::to_aff<true>(a, out.x, out.y); }
static G1Eval eval_affine_of(const G1::Acc& a) {
    G1::Aff p;
    return aff_of(a, p) ? g1_eval_aff(p.x, p.y, false) : g1_eval_aff(fe_zero<BLS381Fq>(), fe_zero<BLS381Fq>(), true);
}
static Fq12 pairing(const G1Eval& P, const G2Aff& Q) { return final_exp(miller_loop(P, Q)); }
// canonical words of an affine point, g1_load's input
static void canon_xy(const G1::Aff& p, uint32_t* xy) {
    const Fq x = fe_from_mont<BLS381Fq>(p.x), y = fe_from_mont<BLS381Fq>(p.y);
    for (int i = 0; i < NL; i++) {
        xy[i] = x.v[i];
        xy[NL + i] = y.v[i];
    }
}
// a point of E(Fq) with the given x, if x^3 + 4 is a square (p = 3 mod 4: the root is a^((p + 1) / 4))
static bool lift_x(uint32_t x0, G1::Aff& out) {
    const Fq x = small(x0), rhs = fq_add(fq_mul(fq_mul(x, x), x), small(4));
    uint32_t e[NL];  // (p + 1) / 4
    uint64_t c = 1;
    for (int i = 0; i < NL; i++) {
        c += BLS381Fq::p(i);
        e[i] = (uint32_t)c;
        c >>= 32;
    }
    for (int i = 0; i < NL; i++) e[i] = (e[i] >> 2) | (i + 1 < NL ? e[i + 1] << 30 : 0);
    Fq y = fe_one<BLS381Fq>();
    for (int i = NL - 1; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            y = fq_mul(y, y);
            if ((e[i] >> b) & 1) y = fq_mul(y, rhs);
        }
    out = G1::Aff{x, y};
    return fe_eq<BLS381Fq>(fq_mul(y, y), rhs);
}

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
        const G1Eval P{rndq(), rndq(), rndq(), false};
        expect(fq12_eq(fq12_mul_line(e, l, P), sb12(e, line_as_fq12(l, P))), "line product");
    }
    {  // Frobenius: a^p, composition, order 12
        uint32_t p[NL];
        for (int i = 0; i < NL; i++) p[i] = BLS381Fq::p(i);
        for (int it = 0; it < 2; it++) {
            const Fq12 a = rnd12();
            const Fq12 f1 = fq12_frob(a, 1);
            expect(fq12_eq(f1, pow12(a, p, NL)), "frob1 == a^p");
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
    for (int i = 0; i < 8; i++) r[i] = BLS381Fr::p(i);
    expect(!fq12_is_one(eGH), "e(G, H) != 1");
    expect(fq12_is_one(pow12(eGH, r, 8)), "e(G, H)^r == 1");
    expect(fq12_is_one(pairing(g1_eval_aff(G.x, G.y, true), H)), "e(O, H) == 1");
    expect(fq12_is_one(pairing(Ge, G2Aff{fq2_zero(), fq2_zero(), true})), "e(G, O) == 1");
    for (int it = 0; it < 8; it++) {
        const FrE a = fe_from_mont<BLS381Fr>(rnd_fe<BLS381Fr>()), b = fe_from_mont<BLS381Fr>(rnd_fe<BLS381Fr>());
        const FrE ab = fe_from_mont<BLS381Fr>(fr_mul(fe_to_mont<BLS381Fr>(a), fe_to_mont<BLS381Fr>(b)));
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
        FrE ab1 = ab;
        ab1.v[0] ^= 1;
        const G1Eval N0 = g1_eval_acc(G1::neg(g1_mul(G, ab.v))), N1 = g1_eval_acc(G1::neg(g1_mul(G, ab1.v)));
        expect(fq12_is_one(final_exp(miller_loop_tab2(P0, tab0, N0, tab1))), "product check accepts");
        expect(!fq12_is_one(final_exp(miller_loop_tab2(P0, tab0, N1, tab1))), "product check rejects");
        const G1Eval Ps[2] = {P0, N0};
        const G2Aff Qs[2] = {bH, H};
        expect(pairing_product_is_one(2, Ps, Qs), "pairing_product_is_one");
    }
    // the subgroup test against [r] P: 8 points in G1, 8 points of E(Fq) outside it
    G1::Aff T{};  // a non-identity point of small order: [r] R for R outside G1
    bool have_T = false;
    {
        int inside = 0, outside = 0;
        for (int it = 0; it < 8; it++) {
            const FrE a = fe_from_mont<BLS381Fr>(rnd_fe<BLS381Fr>());
            G1::Aff P;
            if (!aff_of(g1_mul(G, a.v), P)) continue;
            expect(G1::is_zero(g1_mul(P, r)), "[r] (aG) == O");
            expect(g1_in_subgroup(P), "aG passes the subgroup test");
            inside++;
        }
        for (uint32_t x0 = 5; outside < 8 && x0 < 200; x0++) {
            G1::Aff R;
            if (!lift_x(x0, R)) continue;
            const G1::Acc rR = g1_mul(R, r);
            if (G1::is_zero(rR)) continue;  // (would be in G1: does not happen for small x)
            expect(!g1_in_subgroup(R), "a point outside G1 fails the subgroup test");
            if (!have_T) {
                expect(x0 == 5, "x = 5 lifts to a point outside G1");
                have_T = aff_of(rR, T);
            }
            outside++;
        }
        expect(inside == 8 && outside == 8 && have_T, "8 points inside and 8 outside");
        expect(!g1_in_subgroup(T), "T = [r] R fails the subgroup test");
    }
    // kzg_check: f(X) = c0 + c1 X committed with the secret s, opened at z >= size (p = z):
    // C = f(s) G, y = f(z), pi = c1 G ((f(X) - y) / (X - z) = c1)
    int cofactor_verdict = -1;
    {
        const FrE s = rnd_fe<BLS381Fr>(), c0 = rnd_fe<BLS381Fr>(), c1 = rnd_fe<BLS381Fr>();  // Montgomery
        FrE zc = fe_zero<BLS381Fr>();
        zc.v[0] = 1000;  // canonical, >= size
        const FrE z = fe_to_mont<BLS381Fr>(zc);
        const FrE fs = fe_from_mont<BLS381Fr>(fe_add<BLS381Fr>(c0, fr_mul(c1, s)));
        const FrE y = fe_from_mont<BLS381Fr>(fe_add<BLS381Fr>(c0, fr_mul(c1, z)));
        const FrE sc = fe_from_mont<BLS381Fr>(s), c1c = fe_from_mont<BLS381Fr>(c1);
        G1::Aff C, pi;
        expect(aff_of(g1_mul(G, fs.v), C) && aff_of(g1_mul(G, c1c.v), pi), "C, pi not the identity");
        static LineCoef tab_s[PC::ATE_LINES], tab_h[PC::ATE_LINES];
        ate_line_table(g2_mul(H, sc.v, 8), tab_s);
        ate_line_table(H, tab_h);
        const FrE omega = fe_one<BLS381Fr>();
        uint32_t pw[8];
        kzg_eval_point(omega, 16, zc.v, pw);
        expect(kzg_check(C, false, pi, false, y.v, pw, tab_s, tab_h), "kzg_check accepts a valid opening");
        FrE y2 = y;
        y2.v[0] ^= 1;
        expect(!kzg_check(C, false, pi, false, y2.v, pw, tab_s, tab_h), "kzg_check rejects a changed y");
        expect(!kzg_check(pi, false, C, false, y.v, pw, tab_s, tab_h), "kzg_check rejects swapped points");
        // the inputs through g1_load, as the verifiers take them
        uint32_t w[2 * NL];
        G1::Aff L;
        canon_xy(pi, w);
        expect(g1_load(w, L) && fe_eq<BLS381Fq>(L.x, pi.x) && fe_eq<BLS381Fq>(L.y, pi.y), "g1_load(pi)");
        w[NL] ^= 1;
        expect(!g1_load(w, L), "g1_load rejects a point off the curve");
        for (int i = 0; i < NL; i++) w[i] = BLS381Fq::p(i);
        expect(!g1_load(w, L), "g1_load rejects x == p");
        // the cofactor attack: pi + T is on the curve and pairs as pi does
        G1::Aff piT;
        expect(have_T && aff_of(G1::madd(G1::from_aff(pi, false), T, false), piT), "pi + T");
        expect(kzg_check(C, false, piT, false, y.v, pw, tab_s, tab_h),
               "without the subgroup test pi + T verifies (kzg_check takes validated points)");
        canon_xy(piT, w);
        const bool loaded = g1_load(w, L);
        cofactor_verdict = loaded && kzg_check(C, false, L, false, y.v, pw, tab_s, tab_h) ? 1 : 0;
#ifdef VK_BLS_NO_SUBGROUP_TEST
        expect(cofactor_verdict == 1, "the subgroup test compiled out: pi + T is accepted");
#else
        expect(cofactor_verdict == 0, "g1_load rejects pi + T");
#endif
    }
    printf("{\"checks\": %d, \"mismatches\": %d, \"cofactor_verdict\": %d}\n", checks, bad, cofactor_verdict);
    return bad ? 1 : 0;
}

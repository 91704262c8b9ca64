// Per-lane arithmetic of IPA batch proving (vc_ipa_prove_many), host + gfx950 device from one
// source: the kernels of ipa_many.hip are wrappers that add the cross-lane steps (xor shuffles), and
// tests/cpp/ipa_many_check.cpp runs the same text on the host, 64 lanes in a loop.
//
// One opening is IPA::prove_point (ipa/mod.rs:137-154 -> low_level_ipa :268-319) of a row a of N
// values at a point z over a fresh "ipa" transcript, in ipa.hip's representation: the folded
// generators are coefficients over the original CRS, so a round's L and R are two rows of N + 1
// scalars (ipa_rounds.hpp) for the fixed-base commit. A wave takes one opening; lane l holds the
// entries i = l, l + 64, .. < N, at most IM_EPL of them (for N < 64 the upper lanes hold nothing).
// The transcript is hashed from register words by ipa_batch.hpp's challenge_w / challenge_x, every
// lane of the wave computing the same value.
//
// The barycentric weights outside the domain, b_i = (z^N - 1) / N * w^i / (z - w^i) (precompute.rs:
// 72-90): Montgomery's trick over the N denominators d_i = z - w^i gives 1 / d_i = E_i / D with
// E_i = prod_{j != i} d_j and D = prod_j d_j -- and D = z^N - 1 is the very factor b_i carries, so
// b_i = (1 / N) w^i E_i and the trick's one inversion is never taken. E_i is (the product of the
// other lanes' totals, one xor butterfly: kzg_many.hpp's others_step) x (the lane's own other
// entries).
//
// The levels: a and b of round r have m = N >> r entries. Level 0 of a is the data row itself and
// level 0 of b the weights; a round r > 0 first closes round r - 1 (its challenge x from L, R) and
// reads level r as level r - 1 folded by x (ipar::fold_a_at / fold_b_at), entry by entry wherever
// it needs one, and stores it beside the earlier levels for the next round. No lane ever reads what
// another lane of the same launch wrote. The coefficients are folded in place, each by its own lane.
#pragma once
#include "ipa_batch.hpp"
#include "ipa_rounds.hpp"
#include "kzg_many.hpp"

namespace vk {
namespace ipam {

using namespace ipab;

constexpr int IM_EPL = 4;                     // entries of a, b and the coefficients per lane
constexpr uint32_t IM_N_MAX = 64 * IM_EPL;
constexpr uint32_t IM_STATE_WORDS = 16;       // per opening: w (Montgomery), the previous challenge (canonical)

// where level r of an opening's a (r >= 1: N - 1 entries in all) and b (r >= 0: 2 N - 1) starts
VK_HD size_t a_level(uint32_t N, int r) { return (size_t)N - 2 * (size_t)(N >> r); }
VK_HD size_t b_level(uint32_t N, int r) { return 2 * (size_t)N - 2 * (size_t)(N >> r); }

// ---------------------------------------------------------------- init
// the lane's product of z - w^i (one for a lane without entries)
VK_HD FrE bary_lane_total(const FrE* pw, uint32_t N, const FrE& z, uint32_t lane) {
    FrE run = fe_one<BN254Fr>();
    for (uint32_t i = lane; i < N; i += 64) run = fr_mul(run, fe_sub<BN254Fr>(z, pw[i]));
    return run;
}
// the lane's weights b_i (written to b) and its part of <a, b>. In the domain at idx the weights are
// one-hot (precompute.rs:75-79); outside, oth is the product of the other lanes' totals.
VK_HD FrE init_lane(const FrE* a, const FrE* pw, uint32_t N, const FrE& z, bool in_dom, uint64_t idx, const FrE& oth,
                    const FrE& n_inv, uint32_t lane, FrE* b) {
    FrE acc = fe_zero<BN254Fr>();
    if (in_dom) {
        for (uint32_t i = lane; i < N; i += 64) {
            b[i] = i == idx ? fe_one<BN254Fr>() : fe_zero<BN254Fr>();
            if (i == idx) acc = fr_mul(a[i], b[i]);
        }
        return acc;
    }
    FrE d[IM_EPL];
#pragma unroll
    for (int c = 0; c < IM_EPL; c++) {
        const uint32_t i = lane + 64 * c;
        d[c] = i < N ? fe_sub<BN254Fr>(z, pw[i]) : fe_one<BN254Fr>();
    }
#pragma unroll
    for (int c = 0; c < IM_EPL; c++) {
        const uint32_t i = lane + 64 * c;
        if (i >= N) continue;
        FrE e = oth;
#pragma unroll
        for (int c2 = 0; c2 < IM_EPL; c2++)
            if (c2 != c) e = fr_mul(e, d[c2]);
        const FrE bi = fr_mul(fr_mul(n_inv, pw[i]), e);
        b[i] = bi;
        acc = fe_add<BN254Fr>(acc, fr_mul(a[i], bi));
    }
    return acc;
}
// w of the opening's transcript after C (canonical affine words, identity flag), z and y = <a, b>
// (Montgomery; its canonical words go to y_canon, the proof's y)
VK_HD FrE opening_w(const uint32_t* com_xy, bool com_inf, const uint32_t* zw, const FrE& y, uint32_t* y_canon) {
    uint32_t c[8];
    compress_words(com_xy, com_inf, c);
    fr_store(fe_from_mont<BN254Fr>(y), y_canon);
    return challenge_w(c, zw, y_canon);
}

// ---------------------------------------------------------------- rounds
// the challenge that closes round k: prev is the previous challenge (canonical words), w before x_0
VK_HD FrE close_challenge(const uint32_t* prev, int k, const uint32_t* l_xy, bool l_inf, const uint32_t* r_xy,
                          bool r_inf) {
    uint32_t lw[8], rw[8];
    compress_words(l_xy, l_inf, lw);
    compress_words(r_xy, r_inf, rw);
    return challenge_x(prev, k == 0 ? 'w' : 'x', lw, rw);
}

// a and b of the round being built: stored entries as they are (round 0), or the previous level's
// (2 m entries) folded by x into m
struct Level {
    const FrE *a, *b;
    FrE x;
    uint32_t m;
    bool fold;
    VK_HD FrE a_at(uint32_t j) const { return fold ? ipar::fold_a_at(x, a[j], a[j + m]) : a[j]; }
    VK_HD FrE b_at(uint32_t j) const { return fold ? ipar::fold_b_at(x, b[j], b[j + m]) : b[j]; }
};
// round 0's level of an opening: the data row and the weights as init left them at wb (the
// opening's 2 N entries of b's levels)
VK_HD Level level_first(const FrE* row, const FrE* wb, uint32_t N) {
    return Level{row, wb, fe_one<BN254Fr>(), N, false};
}
// the level after round k is closed by x: level k (the data row for k = 0, else in wa, the opening's
// N entries of a's levels) folded into N >> (k + 1) entries
VK_HD Level level_after(const FrE* row, const FrE* wa, const FrE* wb, uint32_t N, int k, const FrE& x) {
    return Level{k == 0 ? row : wa + a_level(N, k), wb + b_level(N, k), x, N >> (k + 1), true};
}
// where round r >= 1 stores its level for the next round
VK_HD FrE* a_store(FrE* wa, uint32_t N, int r) { return r ? wa + a_level(N, r) : wa; }
VK_HD FrE* b_store(FrE* wb, uint32_t N, int r) { return wb + b_level(N, r); }

// The lane's entries of round r's rows sL, sR (index < N; ipar::round_rows' rule) and, for r > 0, of
// the coefficients' fold by the challenge that closed round r - 1 (ipar::round_fold's rule; the
// coefficients are all one before the first fold and are not read then).
VK_HD void rows_lane(const Level& lv, FrE* coeff, uint32_t N, int r, uint32_t lane, FrE* sL, FrE* sR) {
    const uint32_t m = N >> r, half = m / 2;
    for (uint32_t i = lane; i < N; i += 64) {
        FrE v = lv.a_at((uint32_t)ipar::row_source(i, m, half));
        if (r > 0) {
            FrE co = r == 1 ? fe_one<BN254Fr>() : coeff[i];
            if (ipar::coeff_folds(i, 2 * m, m)) co = fr_mul(co, lv.x);
            coeff[i] = co;
            v = fr_mul(v, co);
        }
        const bool left = ipar::row_is_left(i, m, half);
        sL[i] = left ? v : fe_zero<BN254Fr>();
        sR[i] = left ? fe_zero<BN254Fr>() : v;
    }
}
// The lane's part of <a_L, b_R> (dl) and <a_R, b_L> (dr) over the level's halves (zero b entries
// skipped, as ipar::inner skips them); a folded level is stored to a_out, b_out for the next round.
VK_HD void halves_lane(const Level& lv, uint32_t half, uint32_t lane, FrE* a_out, FrE* b_out, FrE& dl, FrE& dr) {
    dl = fe_zero<BN254Fr>(), dr = fe_zero<BN254Fr>();
    for (uint32_t j = lane; j < half; j += 64) {
        const FrE al = lv.a_at(j), ar = lv.a_at(j + half), bl = lv.b_at(j), br = lv.b_at(j + half);
        if (lv.fold) {
            a_out[j] = al, a_out[j + half] = ar;
            b_out[j] = bl, b_out[j + half] = br;
        }
        if (!fe_is_zero<BN254Fr>(br)) dl = fe_add<BN254Fr>(dl, fr_mul(al, br));
        if (!fe_is_zero<BN254Fr>(bl)) dr = fe_add<BN254Fr>(dr, fr_mul(ar, bl));
    }
}
// the scalar of q in a row from the wave's dot product (ipar::q_terms)
VK_HD FrE q_term(const FrE& w, const FrE& dot) { return fr_mul(w, dot); }
// the proof's tip: the one entry of the last level (lv.m == 1), canonical words
VK_HD void tip_words(const Level& lv, uint32_t* out) { fr_store(fe_from_mont<BN254Fr>(lv.a_at(0)), out); }

}  // namespace ipam
}  // namespace vk

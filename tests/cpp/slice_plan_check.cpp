// Host check of the slice geometry chosen by msm_slice_plan (verkle-kzg_amd/csrc/msm_plan.hpp):
// prints one JSON line per named shape (the slices the MSM paths enqueue, msm.hip msm_run_t /
// msm_run_many_t / msm_run_host_chunks_t) for tests/test_slice_plan.py.
#include <cstdio>
#include "../../verkle-kzg_amd/csrc/msm_plan.hpp"
using namespace vk;

static void show(const char* name, const SliceShape& s) {
    const SlicePlan p = msm_slice_plan(s);  // (sort_chunk: the default, SORT_CHUNK as built)
    printf("{\"name\": \"%s\", \"nv\": %zu, \"c\": %d, \"W\": %d, \"wb\": %d, \"we\": %d, \"shared\": %d, \"sets\": %d, "
           "\"m\": %u, \"top_f\": %d, \"m_override\": %u, ",
           name, s.nv, s.c, s.W, s.wb, s.we, s.shared ? 1 : 0, s.sets, s.m, s.top_f, s.m_override);
    printf("\"M\": %u, \"Lseg\": %u, \"S\": %u, \"J\": %u, \"nU\": %u, \"Tmax\": %u, \"NB\": %u, \"NBtot\": %u, "
           "\"FB\": %u, \"chunk\": %u, \"cstage\": %d, \"NBC\": %u, \"nblk\": %u, \"ncnt\": %zu, \"guard\": %u}\n",
           p.M, p.Lseg, p.S, p.J, p.nU, p.Tmax, p.NB, p.NBtot, p.FB, p.chunk, p.cstage ? 1 : 0, p.NBC, p.nblk, p.ncnt,
           p.guard);
}

// windows [part, part + 1) of `parts` of a per-window MSM of nv terms whose digits cover `total`
// bits in c-bit windows (msm_run_t: the top window's shortfall counts when it is in the slice)
static SliceShape per_window(size_t nv, int c, int total, int part = 0, int parts = 1, uint32_t m_override = 0) {
    const int Wfull = (total + c - 1) / c;
    SliceShape s;
    s.nv = nv, s.c = c, s.wb = part * Wfull / parts, s.we = (part + 1) * Wfull / parts, s.W = s.we - s.wb;
    if (s.we == Wfull) s.top_f = top_shortfall(c, total);
    s.m_override = m_override;
    return s;
}
// `sets` MSMs of nv terms on the shared-window copies: radix m 2^c digits, W windows per set
static SliceShape shared(size_t nv, int c, int W, uint32_t m, int sets = 1) {
    SliceShape s;
    s.nv = nv, s.c = c, s.W = W * sets, s.wb = 0, s.we = W * sets, s.shared = true, s.sets = sets, s.m = m;
    return s;
}

int main() {
    const int BN = 254 + 1, BAND = 253 + 1, GLV = 128;  // digit bits: the scalar's and the recoding's spare one
    show("bn254_2e20", per_window(1u << 20, choose_window(1u << 20, BN), BN));
    show("band_2e20", per_window(1u << 20, choose_window(1u << 20, BAND), BAND));
    show("radix_2e20", shared(1u << 21, 16, 7, 5));  // BLS12-381 2^20: GLV halves, radix 5 x 2^16
    show("radix_2sets", shared(1u << 21, 16, 7, 5, 2));
    show("radix_8sets", shared(1u << 21, 16, 7, 5, 8));
    show("glv_perwin", per_window(1u << 21, glv_window(1u << 21), GLV));
    show("glv_slice8", per_window(1u << 21, glv_window(1u << 21), GLV, 0, 8));
    show("glv_slice2", per_window(1u << 21, glv_window(1u << 21), GLV, 0, 2));
    show("shared_pow2", shared(1u << 21, glv_window(1u << 21), (GLV + 15) / glv_window(1u << 21), 1));  // c = 16
    show("radix_range_2e17", shared(1u << 17, 16, 7, 5));  // a 2^16-point range of a larger table
    show("n1", per_window(1, choose_window(1, BN), BN));
    show("n1000", per_window(1000, choose_window(1000, BN), BN));
    show("n20000", per_window(20000, choose_window(20000, BN), BN));
    show("m_override1", per_window(1u << 14, choose_window(1u << 14, BN), BN, 0, 1, 1));
    show("m_override2", per_window(1u << 14, choose_window(1u << 14, BN), BN, 0, 1, 2));
    return 0;
}

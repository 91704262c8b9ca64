// Host check of Montgomery's trick over block products (verkle-kzg_amd/csrc/batch_inv.hpp
// BlockInverses: the host step of the split normalisations and of batch_inverse) on BN254 Fq,
// BLS12-381 Fq, Bandersnatch's base field (BLS12-381 Fr) and BN254 Fr: nblk = 1, 2, 3 and 127 random
// non-zero products with ones among them, driven in one take(nblk), in uneven pieces with empty
// take calls between them, and one block at a time. Every inv[b] must equal fe_inv_host(prod[b])
// and inv[b] * prod[b] must be one. Prints one JSON line per field: checks, mismatches.
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../verkle-kzg_amd/csrc/batch_inv.hpp"
using namespace vk;

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {
    rs ^= rs << 13;
    rs ^= rs >> 7;
    rs ^= rs << 17;
    return rs;
}

template <class F>
static fe<F> random_nonzero() {  // a Montgomery value in [1, p)
    for (;;) {
        fe<F> a, p;
        for (int i = 0; i < F::N; i += 2) {
            const uint64_t r = rnd64();
            a.v[i] = (uint32_t)r;
            a.v[i + 1] = (uint32_t)(r >> 32);
        }
        a.v[F::N - 1] &= 0x7fffffffu;
        for (int i = 0; i < F::N; i++) p.v[i] = F::p(i);
        for (int k = 0; k < 64 && fe_geq_raw<F>(a, p); k++) fe_sub_raw<F>(a, p);
        if (!fe_is_zero<F>(a)) return a;
    }
}

// the sizes of the take() calls of one drive: 0 = everything at once, 1 = uneven pieces (1, 0, 2,
// 0, 3, ... with empty calls), 2 = one block at a time
template <class F>
static void drive(BlockInverses<F>& bi, int how) {
    if (how == 0) {
        bi.take(bi.nblk);
    } else if (how == 1) {
        bi.take(0);
        for (size_t step = 1, upto = 0; upto < bi.nblk; step++) {
            upto = upto + step < bi.nblk ? upto + step : bi.nblk;
            bi.take(upto);
            bi.take(upto);  // (nothing new)
        }
    } else {
        for (size_t b = 1; b <= bi.nblk; b++) bi.take(b);
    }
    bi.finish();
}

template <class F>
static void run(const char* name) {
    const fe<F> one = fe_one<F>();
    size_t checks = 0;
    int mism = 0;
    for (size_t nblk : {(size_t)1, (size_t)2, (size_t)3, (size_t)127}) {
        for (int ones = 0; ones < 3; ones++) {  // no ones / every third a one / all ones
            std::vector<fe<F>> prod(nblk), want(nblk);
            for (size_t b = 0; b < nblk; b++) {
                prod[b] = (ones == 2 || (ones == 1 && b % 3 == 0)) ? one : random_nonzero<F>();
                want[b] = fe_inv_host<F>(prod[b]);
            }
            for (int how = 0; how < 3; how++) {
                std::vector<fe<F>> inv(nblk, fe_zero<F>());
                BlockInverses<F> bi{prod.data(), inv.data(), nblk};
                drive(bi, how);
                for (size_t b = 0; b < nblk; b++, checks++)
                    if (!fe_eq<F>(inv[b], want[b]) || !fe_eq<F>(fe_mul<F>(inv[b], prod[b]), one)) mism++;
            }
        }
    }
    printf("{\"field\": \"%s\", \"checks\": %zu, \"mismatches\": %d}\n", name, checks, mism);
}

int main() {
    run<BN254Fq>("bn254_fq");
    run<BLS381Fq>("bls12_381_fq");
    run<BLS381Fr>("bandersnatch_fq");
    run<BN254Fr>("bn254_fr");
    return 0;
}

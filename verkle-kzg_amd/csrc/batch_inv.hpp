// Batch inversion, the one text of it: a workgroup's 256 values are multiplied by prefix / suffix
// scans in LDS (block_scan256), each lane takes the product of the OTHER 255 (scan_others), the
// block products go to the host, which inverts them all with one field inversion (Montgomery's
// trick, BlockInverses), and 1 / value = (1 / block product) * others. The normalisations
// (fb_table.hip k_normalize, normalize.hip) and the scalar-field batch_inverse (poly.hip) are built
// from these pieces; the affine tail below is what the normalisations do with the inverse.
// The host part compiles without hipcc (tests/cpp/batch_inv_check.cpp).
#pragma once
#include <stddef.h>

#include "ff.hpp"

namespace vk {

// Montgomery's trick over block products on the host: afterwards inv[b] = 1 / prod[b]. take(upto)
// multiplies blocks [done, upto) into the forward products as they arrive (inv[b] = prod[0] ..
// prod[b]), finish() inverts the last one and walks back. No product may be zero (the callers'
// kernels substitute 1). inv may not alias prod.
template <class F>
struct BlockInverses {
    const fe<F>* prod;
    fe<F>* inv;
    size_t nblk;      // >= 1
    size_t done = 0;  // blocks [0, done) multiplied in
    void take(size_t upto) {
        for (; done < upto; done++) inv[done] = done ? fe_mul<F>(inv[done - 1], prod[done]) : prod[done];
    }
    void finish() {  // after take(nblk)
        fe<F> run = fe_inv_bin<F>(inv[nblk - 1]);
        for (size_t b = nblk - 1; b > 0; b--) {
            const fe<F> ib = fe_mul<F>(run, inv[b - 1]);
            run = fe_mul<F>(run, prod[b]);
            inv[b] = ib;
        }
        inv[0] = run;
    }
};

#ifdef __HIPCC__
// Inclusive prefix (pre) and suffix (suf) products of the 256 lanes' values z, in two LDS arrays of
// 256 the caller owns; every thread of the 256-thread block calls it. The arrays may be read once
// it returns (its last statement is a barrier); a caller that scans again into the same pair puts
// a barrier between its last read and that call.
template <class F>
__device__ __forceinline__ void block_scan256(const fe<F>& z, fe<F>* pre, fe<F>* suf) {
    const uint32_t tid = threadIdx.x;
    pre[tid] = z;
    suf[tid] = z;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        fe<F> p = pre[tid], s = suf[tid];
        if (tid >= off) p = fe_mul<F>(pre[tid - off], p);
        if (tid + off < 256) s = fe_mul<F>(s, suf[tid + off]);
        __syncthreads();
        pre[tid] = p;
        suf[tid] = s;
        __syncthreads();
    }
}
// the product of the other 255 lanes' values, from the scanned arrays (the block's product: pre[255])
template <class F>
__device__ __forceinline__ fe<F> scan_others(const fe<F>* pre, const fe<F>* suf) {
    const uint32_t tid = threadIdx.x;
    fe<F> o = fe_one<F>();
    if (tid > 0) o = pre[tid - 1];
    if (tid < 255) o = tid > 0 ? fe_mul<F>(o, suf[tid + 1]) : suf[tid + 1];
    return o;
}

// ---- the normalisations' ends: what an accumulator puts into the batch inversion, and the affine
// point its inverse gives
template <class C>
__device__ __forceinline__ fe<typename C::F> denom(const typename C::Acc& a) {
    if constexpr (C::is_te) return a.Z;
    else return a.zzz;
}
// accumulators that take denominator 1 in the batch inversion: the SW identity (Z = 0, nothing
// to invert). An Edwards point always has Z != 0 -- its identity (0 : Z : Z) included, which must
// be divided by Z like any other point (it was counted as 1 and came out as (0, Z), not (0, 1))
template <class C>
__device__ __forceinline__ bool norm_as_one(const typename C::Acc& a) {
    if constexpr (C::is_te) return false;
    else return C::is_zero(a);
}
// x, y (Montgomery) and the identity flag of accumulator a, iz = 1 / denom(a) (anything where
// norm_as_one(a): the SW identity's coordinates are not used)
template <class C>
__device__ __forceinline__ void acc_affine(const typename C::Acc& a, const fe<typename C::F>& iz,
                                           fe<typename C::F>& x, fe<typename C::F>& y, bool& ident) {
    using F = typename C::F;
    if constexpr (C::is_te) {
        x = fe_mul<F>(a.X, iz);
        y = fe_mul<F>(a.Y, iz);
        ident = fe_is_zero<F>(x) && fe_eq<F>(y, fe_one<F>());
    } else {
        ident = C::is_zero(a);
        fe<F> t = fe_mul<F>(iz, a.zz);  // 1/Z
        x = fe_mul<F>(a.x, fe_sqr<F>(t));
        y = fe_mul<F>(a.y, iz);
    }
}
// point j to whichever of the three outputs is given: Montgomery affine (with the Edwards kt),
// canonical x | y words (the SW identity as zeros), identity flag
template <class C>
__device__ __forceinline__ void store_affine(size_t j, const fe<typename C::F>& x, const fe<typename C::F>& y,
                                             bool ident, typename C::Aff* __restrict__ out_aff,
                                             uint32_t* __restrict__ out_canon, uint8_t* __restrict__ out_inf) {
    using F = typename C::F;
    if (out_aff) {
        typename C::Aff r;
        r.x = x;
        r.y = y;
        if constexpr (C::is_te) r.kt = fe_mul<F>(fe_mul<F>(x, y), C::d());
        out_aff[j] = r;
    }
    if (out_canon) {
        fe<F> cx = fe_from_mont<F>(x), cy = fe_from_mont<F>(y);
        if (ident && !C::is_te) {
            cx = fe_zero<F>();
            cy = fe_zero<F>();
        }
#pragma unroll
        for (int k = 0; k < F::N; k++) {
            out_canon[j * 2 * F::N + k] = cx.v[k];
            out_canon[j * 2 * F::N + F::N + k] = cy.v[k];
        }
    }
    if (out_inf) out_inf[j] = ident ? 1 : 0;
}
#endif  // __HIPCC__

}  // namespace vk

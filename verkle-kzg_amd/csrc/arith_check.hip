// libvkzg_check.so (test only; never linked into libvkzg.so, not declared in include/): the field
// and group primitives of ff.hpp, ff29.hpp, ff30.hpp, ec.hpp, ec29.hpp and ec30.hpp one operation
// at a time, on plain 32-bit words, so tests/test_arith_host.py and tests/test_gpu_arith.py can
// compare the device build of the headers with their host build and with Python integers.
// There is no arithmetic here: every operation group is one VK_HD text that calls the headers,
// instantiated in a kernel (one lane per case) and in a host loop over the same cases. The
// cross-lane groups (add_quad, fb_block_sum_store) exist on the device only.
//
// Word layouts (all uint32, little-endian limbs):
//   vkc_fe:    a, b, out: n x N words (N of the field).
//   vkc_limb:  a, b, c, d, out: n x L words (L limbs of the set; signed limbs of ff30.hpp as their
//              two's-complement words). Operations on the 32-bit form read / write the first N
//              words of a record; is_zero_mo writes word 0.
//   vkc_point: bases: nb affine points in the ec.hpp layout (Montgomery form: x, y and, on
//              Bandersnatch, d x y); cases: n PtCase records; out: n x (4 N + 1) words, the ec.hpp
//              accumulator followed by the identity flag.
//   vkc_quad:  the same cases, lane l of the one wave runs case l / 4; out: one record per lane.
//   vkc_block_sum: spec: 4 words per thread (chain length <= 3, then the chain); out: one ec.hpp
//              accumulator (4 N words) per block.
// A chain entry is (base index << 1) | sign: the accumulator is built by mixed adds from the
// identity, so its limbs are in the state the kernels see.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/vc_msm.h"
#include "ec.hpp"
#include "ec29.hpp"
#include "ec30.hpp"
#include "ff.hpp"
#include "ff29.hpp"
#include "ff30.hpp"

using namespace vk;

namespace {

// ---------------------------------------------------------------- one text, two evaluators
template <class Op, class... A>
__global__ void k_cases(size_t n, A... a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) Op::run(i, a...);
}

bool have_device() {
    int ndev = 0;
    return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
}

// host arrays, or their device copies when the device evaluates
struct Stage {
    bool dev;
    int err = VC_OK;
    std::vector<void*> bufs;
    struct Out {
        void* d;
        void* h;
        size_t bytes;
    };
    std::vector<Out> outs;
    explicit Stage(bool d) : dev(d) {}
    ~Stage() {
        for (void* p : bufs) (void)hipFree(p);
    }
    void* alloc(size_t bytes) {
        void* d = nullptr;
        if (hipMalloc(&d, bytes ? bytes : 4) != hipSuccess) {
            err = VC_E_OOM;
            return nullptr;
        }
        bufs.push_back(d);
        return d;
    }
    template <class T>
    const T* in(const T* h, size_t count) {
        if (!dev || !h) return h;
        void* d = alloc(count * sizeof(T));
        if (d && hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) err = VC_E_HIP;
        return (const T*)d;
    }
    template <class T>
    T* out(T* h, size_t count) {
        if (!dev) return h;
        void* d = alloc(count * sizeof(T));
        if (d && hipMemset(d, 0, count * sizeof(T)) != hipSuccess) err = VC_E_HIP;
        outs.push_back({d, h, count * sizeof(T)});
        return (T*)d;
    }
    int finish() {
        if (!dev || err != VC_OK) return err;
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return VC_E_HIP;
        for (const Out& o : outs)
            if (hipMemcpy(o.h, o.d, o.bytes, hipMemcpyDeviceToHost) != hipSuccess) return VC_E_HIP;
        return VC_OK;
    }
};

template <class Op, class... A>
void run_cases(const Stage& st, size_t n, A... a) {
    if (st.err != VC_OK || n == 0) return;
    if (st.dev) {
        hipLaunchKernelGGL((k_cases<Op, A...>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, n, a...);
    } else {
        for (size_t i = 0; i < n; i++) Op::run(i, a...);
    }
}

// ---------------------------------------------------------------- (a) ff.hpp
enum { FE_MUL, FE_SQR, FE_MUL_BODY, FE_ADD, FE_SUB, FE_NEG, FE_DBL, FE_SMALL3, FE_SMALL5, FE_SMALL8, FE_TO_MONT,
       FE_FROM_MONT, FE_INV, FE_INV_BIN, FE_OPS };

template <class F>
struct FeOp {
    VK_HD static void run(size_t i, int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
        fe<F> x, y, r = fe_zero<F>();
        for (int k = 0; k < F::N; k++) {
            x.v[k] = a[i * F::N + k];
            y.v[k] = b[i * F::N + k];
        }
        switch (op) {
            case FE_MUL: r = fe_mul<F>(x, y); break;
            case FE_SQR: r = fe_sqr<F>(x); break;
            case FE_MUL_BODY: r = fe_mul_body<F>(x, y); break;
            case FE_ADD: r = fe_add<F>(x, y); break;
            case FE_SUB: r = fe_sub<F>(x, y); break;
            case FE_NEG: r = fe_neg<F>(x); break;
            case FE_DBL: r = fe_dbl<F>(x); break;
            case FE_SMALL3: r = fe_mul_small<F, 3>(x); break;
            case FE_SMALL5: r = fe_mul_small<F, 5>(x); break;
            case FE_SMALL8: r = fe_mul_small<F, 8>(x); break;
            case FE_TO_MONT: r = fe_to_mont<F>(x); break;
            case FE_FROM_MONT: r = fe_from_mont<F>(x); break;
            case FE_INV: r = fe_inv<F>(x); break;
            case FE_INV_BIN: r = fe_inv_bin<F>(x); break;
        }
        for (int k = 0; k < F::N; k++) out[i * F::N + k] = r.v[k];
    }
};

template <class F>
int fe_group(int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out, bool dev) {
    Stage st(dev);
    const uint32_t* da = st.in(a, n * F::N);
    const uint32_t* db = st.in(b, n * F::N);
    uint32_t* dout = st.out(out, n * F::N);
    run_cases<FeOp<F>>(st, n, op, da, db, dout);
    return st.finish();
}

// ---------------------------------------------------------------- (b) ff29.hpp / ff30.hpp
enum { LB_MUL, LB_SQR, LB_MUL2SUM, LB_ADD, LB_MUL_RAW1, LB_MUL_RAW2, LB_SUB4, LB_SUB16, LB_SUB2_8, LB_NEG4, LB_CANON,
       LB_PACK, LB_UNPACK, LB_FROM_MONT32, LB_TO_MONT32, LB_IS_ZERO_MO, LB_OPS };

template <class P, class F>
struct Limb29Op {
    static constexpr int L = P::L;
    static bool has(int op) { return op >= 0 && op < LB_OPS && (op != LB_MUL_RAW2 || L <= 9); }
    VK_HD static void run(size_t i, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
                          uint32_t* out) {
        f29<P> x, y, z, w, r = zero29<P>();
        for (int j = 0; j < L; j++) {
            x.v[j] = a[i * L + j];
            y.v[j] = b[i * L + j];
            z.v[j] = c[i * L + j];
            w.v[j] = d[i * L + j];
        }
        uint32_t* o = out + i * L;
        switch (op) {
            case LB_MUL: r = mul29<P>(x, y); break;
            case LB_SQR: r = sqr29<P>(x); break;
            case LB_MUL2SUM: r = mul2sum29<P>(x, y, z, w); break;
            case LB_ADD: r = add29<P>(x, y); break;
            case LB_MUL_RAW1: r = mul29<P>(add29_raw<P>(x, y), y); break;
            case LB_MUL_RAW2:
                if constexpr (L <= 9) r = mul29<P>(add29_raw<P>(x, y), add29_raw<P>(y, x));
                break;
            case LB_SUB4: r = sub29<P, 4>(x, y); break;
            case LB_SUB16: r = sub29<P, 16>(x, y); break;
            case LB_SUB2_8: r = sub2_29<P, 8>(x, y, z); break;
            case LB_NEG4: r = neg29<P, 4>(x); break;
            case LB_CANON: r = canon29<P>(x); break;
            case LB_PACK: pack29<P>(x, r.v); break;  // N <= L words
            case LB_UNPACK: r = unpack29<P>(x.v); break;
            case LB_FROM_MONT32: {
                fe<F> m;
                for (int k = 0; k < F::N; k++) m.v[k] = x.v[k];
                r = from_mont32<P, F>(m);
                break;
            }
            case LB_TO_MONT32: {
                const fe<F> m = to_mont32<P, F>(x);
                for (int k = 0; k < F::N; k++) r.v[k] = m.v[k];
                break;
            }
            case LB_IS_ZERO_MO: r.v[0] = is_zero_mo29<P>(x) ? 1u : 0u; break;
        }
        for (int j = 0; j < L; j++) o[j] = r.v[j];
    }
};

template <class P, class F>
struct Limb30Op {
    static constexpr int L = P::L;
    static bool has(int op) {
        return op >= 0 && op < LB_OPS && op != LB_MUL_RAW1 && op != LB_MUL_RAW2 && op != LB_SUB2_8;
    }
    VK_HD static void run(size_t i, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
                          uint32_t* out) {
        f30<P> x, y, z, w, r = zero30<P>();
        uint32_t u[L];
        for (int j = 0; j < L; j++) {
            x.v[j] = (int32_t)a[i * L + j];
            y.v[j] = (int32_t)b[i * L + j];
            z.v[j] = (int32_t)c[i * L + j];
            w.v[j] = (int32_t)d[i * L + j];
            u[j] = 0;
        }
        uint32_t* o = out + i * L;
        bool words = false;  // the result is in u (unsigned), not in r
        switch (op) {
            case LB_MUL: r = mul30<P>(x, y); break;
            case LB_SQR: r = sqr30<P>(x); break;
            case LB_MUL2SUM: r = mul2sum30<P>(x, y, z, w); break;
            case LB_ADD: r = add30<P>(x, y); break;
            case LB_SUB4:
            case LB_SUB16: r = sub30<P>(x, y); break;  // signed values: one subtraction, no K p
            case LB_NEG4: r = neg30<P>(x); break;
            case LB_CANON:
                canon30<P>(x, u);
                words = true;
                break;
            case LB_PACK: {
                uint32_t in[L];
                for (int j = 0; j < L; j++) in[j] = a[i * L + j];
                pack30<P>(in, u);
                words = true;
                break;
            }
            case LB_UNPACK: {
                uint32_t in[L];
                for (int j = 0; j < L; j++) in[j] = a[i * L + j];
                r = unpack30<P>(in);
                break;
            }
            case LB_FROM_MONT32: {
                fe<F> m;
                for (int k = 0; k < F::N; k++) m.v[k] = a[i * L + k];
                r = from_mont32_30<P, F>(m);
                break;
            }
            case LB_TO_MONT32: {
                const fe<F> m = to_mont32_30<P, F>(x);
                for (int k = 0; k < F::N; k++) u[k] = m.v[k];
                words = true;
                break;
            }
            case LB_IS_ZERO_MO:
                u[0] = is_zero_mo30<P>(x) ? 1u : 0u;
                words = true;
                break;
        }
        for (int j = 0; j < L; j++) o[j] = words ? u[j] : (uint32_t)r.v[j];
    }
};

template <class Op>
int limb_group(int op, size_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
               uint32_t* out, bool dev) {
    if (!Op::has(op)) return VC_E_INVALID;
    Stage st(dev);
    const uint32_t* da = st.in(a, n * Op::L);
    const uint32_t* db = st.in(b, n * Op::L);
    const uint32_t* dc = st.in(c, n * Op::L);
    const uint32_t* dd = st.in(d, n * Op::L);
    uint32_t* dout = st.out(out, n * Op::L);
    run_cases<Op>(st, n, op, da, db, dc, dd, dout);
    return st.finish();
}

// ---------------------------------------------------------------- (c) group law
constexpr uint32_t CHAIN_MAX = 32;
struct PtCase {
    uint32_t plen, qlen;  // chain lengths (0: the identity)
    uint32_t plam, qlam;  // 1 + index of the base whose x rescales the operand; 0: as built
    uint32_t aff, neg;    // the mixed add's affine operand and its sign
    uint32_t pad[2];
    uint32_t pch[CHAIN_MAX], qch[CHAIN_MAX];
};
enum { PT_MADD, PT_ADD, PT_DBL, PT_TO_AFF, PT_TO_AFF_BIN, PT_STORE, PT_PACK_AFF, PT_OPS };

// the same projective point with other coordinates: X l^2, Y l^3, ZZ l^2, ZZZ l^3 (XYZZ), or every
// coordinate times l (extended Edwards)
template <class C>
struct EngOld {
    static constexpr bool fast = false;
    using F = typename C::F;
    using Acc = typename C::Acc;
    using OAff = typename C::Aff;
    static bool has(int op) { return op >= 0 && op < PT_PACK_AFF; }
    VK_HD static Acc zero() { return C::zero(); }
    VK_HD static OAff load(const OAff* b) { return *b; }
    VK_HD static Acc madd(const Acc& p, const OAff& q, bool neg) { return C::madd(p, q, neg); }
    VK_HD static Acc add(const Acc& p, const Acc& q) { return C::add(p, q); }
    VK_HD static Acc dbl(const Acc& p) { return C::dbl(p); }
    VK_HD static Acc scale(const Acc& p, const OAff* lam) {
        const fe<F> l = lam->x;
        Acc r;
        if constexpr (C::is_te) {
            r.X = fe_mul<F>(p.X, l);
            r.Y = fe_mul<F>(p.Y, l);
            r.T = fe_mul<F>(p.T, l);
            r.Z = fe_mul<F>(p.Z, l);
        } else {
            if (C::is_zero(p)) return p;
            const fe<F> l2 = fe_sqr<F>(l), l3 = fe_mul<F>(l2, l);
            r.x = fe_mul<F>(p.x, l2);
            r.y = fe_mul<F>(p.y, l3);
            r.zz = fe_mul<F>(p.zz, l2);
            r.zzz = fe_mul<F>(p.zzz, l3);
        }
        return r;
    }
    VK_HD static void store(const Acc& a, uint32_t* o) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(&a);
        for (int k = 0; k < C::ACC_WORDS; k++) o[k] = w[k];
        o[C::ACC_WORDS] = C::is_zero(a) ? 1u : 0u;
    }
};

template <class P>
VK_HD f29<P> lmul(const f29<P>& a, const f29<P>& b) {
    return mul29<P>(a, b);
}
template <class P>
VK_HD f30<P> lmul(const f30<P>& a, const f30<P>& b) {
    return mul30<P>(a, b);
}

template <class C>
struct EngFast {
    static constexpr bool fast = true;
    using FC = typename Fast29<C>::type;
    using F = typename C::F;
    using Acc = typename FC::Acc;
    using OAff = typename C::Aff;
    // the Edwards engine has no doubling of its own (its add is unified)
    static bool has(int op) {
        return op == PT_MADD || op == PT_ADD || op == PT_STORE || op == PT_PACK_AFF || (op == PT_DBL && !C::is_te);
    }
    VK_HD static Acc zero() { return FC::zero(); }
    // the table path of the kernels: pack_aff, then load of the packed point
    VK_HD static typename FC::Aff load(const OAff* b) {
        OAff packed;
        FC::pack_aff(*b, &packed);
        return FC::load(&packed);
    }
    VK_HD static Acc madd(const Acc& p, const typename FC::Aff& q, bool neg) { return FC::madd(p, q, neg); }
    VK_HD static Acc add(const Acc& p, const Acc& q) { return FC::add(p, q); }
    VK_HD static Acc dbl(const Acc& p) {
        if constexpr (C::is_te) return p;
        else return FC::dbl(p);
    }
    VK_HD static Acc scale(const Acc& p, const OAff* lam) {
        const auto l = load(lam).x;
        Acc r = p;
        if constexpr (C::is_te) {
            r.X = lmul(p.X, l);
            r.Y = lmul(p.Y, l);
            r.T = lmul(p.T, l);
            r.Z = lmul(p.Z, l);
        } else {
            if (p.inf) return p;
            const auto l2 = lmul(l, l), l3 = lmul(l2, l);
            r.x = lmul(p.x, l2);
            r.y = lmul(p.y, l3);
            r.zz = lmul(p.zz, l2);
            r.zzz = lmul(p.zzz, l3);
        }
        return r;
    }
    VK_HD static void store(const Acc& a, uint32_t* o) {
        const typename C::Acc s = FC::store(a);
        const uint32_t* w = reinterpret_cast<const uint32_t*>(&s);
        for (int k = 0; k < C::ACC_WORDS; k++) o[k] = w[k];
        if constexpr (C::is_te) o[C::ACC_WORDS] = C::is_zero(s) ? 1u : 0u;
        else o[C::ACC_WORDS] = a.inf ? 1u : 0u;
    }
};

template <class E>
VK_HD typename E::Acc build_acc(const typename E::OAff* bases, const uint32_t* chain, uint32_t len, uint32_t lam) {
    typename E::Acc a = E::zero();
    for (uint32_t k = 0; k < len; k++) a = E::madd(a, E::load(&bases[chain[k] >> 1]), (chain[k] & 1) != 0);
    if (lam) a = E::scale(a, &bases[lam - 1]);
    return a;
}

template <class C, class E>
struct PtOp {
    static constexpr int OUT = C::ACC_WORDS + 1;
    VK_HD static void run(size_t i, int op, const typename C::Aff* bases, const PtCase* cases, uint32_t* out) {
        using F = typename C::F;
        const PtCase& c = cases[i];
        uint32_t* o = out + i * OUT;
        if (op == PT_PACK_AFF) {
            if constexpr (E::fast) {
                typename C::Aff packed;
                E::FC::pack_aff(bases[c.aff], &packed);
                const uint32_t* w = reinterpret_cast<const uint32_t*>(&packed);
                for (int k = 0; k < C::AFF_WORDS; k++) o[k] = w[k];
            }
            return;
        }
        const typename E::Acc p = build_acc<E>(bases, c.pch, c.plen, c.plam);
        if (op == PT_TO_AFF || op == PT_TO_AFF_BIN) {
            if constexpr (!E::fast) {
                fe<F> x = fe_zero<F>(), y = fe_zero<F>();
                const bool fin = op == PT_TO_AFF ? C::template to_aff<false>(p, x, y) : C::template to_aff<true>(p, x, y);
                for (int k = 0; k < F::N; k++) {  // as to_aff left them (XYZZ: untouched at the identity)
                    o[k] = x.v[k];
                    o[F::N + k] = y.v[k];
                }
                o[C::ACC_WORDS] = fin ? 0u : 1u;
            }
            return;
        }
        typename E::Acc r = p;
        if (op == PT_MADD) r = E::madd(p, E::load(&bases[c.aff]), c.neg != 0);
        else if (op == PT_ADD) r = E::add(p, build_acc<E>(bases, c.qch, c.qlen, c.qlam));
        else if (op == PT_DBL) r = E::dbl(p);
        E::store(r, o);
    }
};

bool cases_ok(const PtCase* cs, size_t n, size_t nb) {
    for (size_t i = 0; i < n; i++) {
        const PtCase& c = cs[i];
        if (c.plen > CHAIN_MAX || c.qlen > CHAIN_MAX || c.plam > nb || c.qlam > nb || c.aff >= nb) return false;
        for (uint32_t k = 0; k < c.plen; k++)
            if ((c.pch[k] >> 1) >= nb) return false;
        for (uint32_t k = 0; k < c.qlen; k++)
            if ((c.qch[k] >> 1) >= nb) return false;
    }
    return true;
}

template <class C, class E>
int point_group(int op, size_t n, const uint32_t* bases, size_t nb, const uint32_t* cases, uint32_t* out, bool dev) {
    using OAff = typename C::Aff;
    static_assert(sizeof(OAff) == C::AFF_WORDS * 4 && sizeof(typename C::Acc) == C::ACC_WORDS * 4, "word layouts");
    const PtCase* cs = reinterpret_cast<const PtCase*>(cases);
    if (!E::has(op) || nb == 0 || !cases_ok(cs, n, nb)) return VC_E_INVALID;
    Stage st(dev);
    const OAff* db = st.in(reinterpret_cast<const OAff*>(bases), nb);
    const PtCase* dc = st.in(cs, n);
    uint32_t* dout = st.out(out, n * (C::ACC_WORDS + 1));
    run_cases<PtOp<C, E>>(st, n, op, db, dc, dout);
    return st.finish();
}

template <class C>
int point_curve(int engine, int op, size_t n, const uint32_t* bases, size_t nb, const uint32_t* cases, uint32_t* out,
                bool dev) {
    if (engine == 0) return point_group<C, EngOld<C>>(op, n, bases, nb, cases, out, dev);
    if (engine == 1) return point_group<C, EngFast<C>>(op, n, bases, nb, cases, out, dev);
    return VC_E_INVALID;
}

// ---------------------------------------------------------------- (d) add_quad: one wave, one case per quad
template <class C>
__global__ void __launch_bounds__(64) k_quad(uint32_t nlanes, const typename C::Aff* bases, const PtCase* cases,
                                             uint32_t* out) {
    using E = EngFast<C>;
    const uint32_t lane = threadIdx.x;
    if (lane >= nlanes) return;
    const PtCase& c = cases[lane >> 2];
    const typename E::Acc p = build_acc<E>(bases, c.pch, c.plen, c.plam);
    const typename E::Acc q = build_acc<E>(bases, c.qch, c.qlen, c.qlam);
    const typename E::Acc r = E::FC::add_quad(p, q, lane & 3);
    E::store(r, out + (size_t)lane * (C::ACC_WORDS + 1));
}

template <class C>
int quad_group(size_t nlanes, const uint32_t* bases, size_t nb, const uint32_t* cases, uint32_t* out) {
    using OAff = typename C::Aff;
    const PtCase* cs = reinterpret_cast<const PtCase*>(cases);
    if (nlanes == 0 || nlanes > 64 || nlanes % 4 || nb == 0 || !cases_ok(cs, nlanes / 4, nb)) return VC_E_INVALID;
    Stage st(true);
    const OAff* db = st.in(reinterpret_cast<const OAff*>(bases), nb);
    const PtCase* dc = st.in(cs, nlanes / 4);
    uint32_t* dout = st.out(out, nlanes * (C::ACC_WORDS + 1));
    if (st.err == VC_OK) hipLaunchKernelGGL(k_quad<C>, dim3(1), dim3((unsigned)nlanes), 0, 0, (uint32_t)nlanes, db, dc, dout);
    return st.finish();
}

// ---------------------------------------------------------------- (e) fb_block_sum_store: one block per pattern
constexpr uint32_t SPEC_WORDS = 4, SPEC_CHAIN = 3;
template <class C, int NT>
__global__ void __launch_bounds__(NT) k_block_sum(const typename C::Aff* bases, const uint32_t* spec, uint32_t* out) {
    using E = EngFast<C>;
    const uint32_t* s = spec + ((size_t)blockIdx.x * NT + threadIdx.x) * SPEC_WORDS;
    const typename E::Acc a = build_acc<E>(bases, s + 1, s[0], 0);
    fb_block_sum_store<C, NT>(a, reinterpret_cast<typename C::Acc*>(out) + blockIdx.x);
}

template <class C>
int block_sum_group(int nt, size_t nblocks, const uint32_t* bases, size_t nb, const uint32_t* spec, uint32_t* out) {
    using OAff = typename C::Aff;
    if ((nt != 64 && nt != 256) || nblocks == 0 || nblocks > 4096 || nb == 0) return VC_E_INVALID;
    const size_t threads = nblocks * (size_t)nt;
    for (size_t t = 0; t < threads; t++) {
        const uint32_t* s = spec + t * SPEC_WORDS;
        if (s[0] > SPEC_CHAIN) return VC_E_INVALID;
        for (uint32_t k = 0; k < s[0]; k++)
            if ((s[1 + k] >> 1) >= nb) return VC_E_INVALID;
    }
    Stage st(true);
    const OAff* db = st.in(reinterpret_cast<const OAff*>(bases), nb);
    const uint32_t* ds = st.in(spec, threads * SPEC_WORDS);
    uint32_t* dout = st.out(out, nblocks * C::ACC_WORDS);
    if (st.err == VC_OK) {
        if (nt == 256) hipLaunchKernelGGL((k_block_sum<C, 256>), dim3((unsigned)nblocks), dim3(256), 0, 0, db, ds, dout);
        else hipLaunchKernelGGL((k_block_sum<C, 64>), dim3((unsigned)nblocks), dim3(64), 0, 0, db, ds, dout);
    }
    return st.finish();
}

}  // namespace

// ---------------------------------------------------------------- C surface (status codes of vc_msm.h)
extern "C" {

// field: 0 BN254Fq, 1 BN254Fr, 2 BLS381Fq, 3 BLS381Fr, 4 BandFr
int vkc_fe(int field, int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out, int on_device) {
    if (!a || !b || !out || op < 0 || op >= FE_OPS) return VC_E_INVALID;
    if (on_device && !have_device()) return VC_E_NO_DEVICE;
    const bool dev = on_device != 0;
    switch (field) {
        case 0: return fe_group<BN254Fq>(op, n, a, b, out, dev);
        case 1: return fe_group<BN254Fr>(op, n, a, b, out, dev);
        case 2: return fe_group<BLS381Fq>(op, n, a, b, out, dev);
        case 3: return fe_group<BLS381Fr>(op, n, a, b, out, dev);
        case 4: return fe_group<BandFr>(op, n, a, b, out, dev);
    }
    return VC_E_INVALID;
}

// set: 0 F29BLS381Fq, 1 F29BN254Fq, 2 F29BLS381Fr, 3 F29BN254Fr, 4 F30BLS381Fq
int vkc_limb(int set, int op, size_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
             uint32_t* out, int on_device) {
    if (!a || !b || !c || !d || !out) return VC_E_INVALID;
    if (on_device && !have_device()) return VC_E_NO_DEVICE;
    const bool dev = on_device != 0;
    switch (set) {
        case 0: return limb_group<Limb29Op<F29BLS381Fq, BLS381Fq>>(op, n, a, b, c, d, out, dev);
        case 1: return limb_group<Limb29Op<F29BN254Fq, BN254Fq>>(op, n, a, b, c, d, out, dev);
        case 2: return limb_group<Limb29Op<F29BLS381Fr, BLS381Fr>>(op, n, a, b, c, d, out, dev);
        case 3: return limb_group<Limb29Op<F29BN254Fr, BN254Fr>>(op, n, a, b, c, d, out, dev);
        case 4: return limb_group<Limb30Op<F30BLS381Fq, BLS381Fq>>(op, n, a, b, c, d, out, dev);
    }
    return VC_E_INVALID;
}

// curve: VC_CURVE_*; engine: 0 ec.hpp, 1 Fast29<C>::type
int vkc_point(int curve, int engine, int op, size_t n, const uint32_t* bases, size_t nb, const uint32_t* cases,
              uint32_t* out, int on_device) {
    if (!bases || !cases || !out) return VC_E_INVALID;
    if (on_device && !have_device()) return VC_E_NO_DEVICE;
    const bool dev = on_device != 0;
    switch (curve) {
        case VC_CURVE_BN254: return point_curve<BN254G1>(engine, op, n, bases, nb, cases, out, dev);
        case VC_CURVE_BLS12_381: return point_curve<BLS381G1>(engine, op, n, bases, nb, cases, out, dev);
        case VC_CURVE_BANDERSNATCH: return point_curve<Bandersnatch>(engine, op, n, bases, nb, cases, out, dev);
    }
    return VC_E_INVALID;
}

// device only: one wave of nlanes (<= 64, whole quads); the curves whose engine has add_quad
int vkc_quad(int curve, size_t nlanes, const uint32_t* bases, size_t nb, const uint32_t* cases, uint32_t* out) {
    if (!bases || !cases || !out) return VC_E_INVALID;
    if (curve != VC_CURVE_BN254 && curve != VC_CURVE_BLS12_381) return VC_E_INVALID;
    if (!have_device()) return VC_E_NO_DEVICE;
    if (curve == VC_CURVE_BN254) return quad_group<BN254G1>(nlanes, bases, nb, cases, out);
    return quad_group<BLS381G1>(nlanes, bases, nb, cases, out);
}

// device only: nblocks blocks of nt (64 or 256) threads, one sum per block
int vkc_block_sum(int curve, int nt, size_t nblocks, const uint32_t* bases, size_t nb, const uint32_t* spec,
                  uint32_t* out) {
    if (!bases || !spec || !out) return VC_E_INVALID;
    if (curve != VC_CURVE_BN254 && curve != VC_CURVE_BLS12_381 && curve != VC_CURVE_BANDERSNATCH) return VC_E_INVALID;
    if (!have_device()) return VC_E_NO_DEVICE;
    switch (curve) {
        case VC_CURVE_BN254: return block_sum_group<BN254G1>(nt, nblocks, bases, nb, spec, out);
        case VC_CURVE_BLS12_381: return block_sum_group<BLS381G1>(nt, nblocks, bases, nb, spec, out);
    }
    return block_sum_group<Bandersnatch>(nt, nblocks, bases, nb, spec, out);
}

}  // extern "C"

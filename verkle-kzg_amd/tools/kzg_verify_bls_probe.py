"""KZG verification on BLS12-381 beside BN254, one box, one run: for n = 256, 4096 and 65,536 valid
openings of width-256 rows (a prover's: n random rows of a 256-point key, committed by vc_msm_batch
and opened by vc_kzg_prove_many, every other point in the domain -- the rows and points of
tools/kzg_prove_many_probe.py) it records, per curve,

  verify_many   vc_kzg_verify_many, one verdict per opening (one lane each);
  verify_batch  vc_kzg_verify_batch with results = NULL, one combined verdict;
  host          vc_kzg_verify on `--host-n` of the openings, on 1 thread and on 16 threads.

Every verdict is checked (all valid; with one y changed the batch rejects and verify_many names
the entry). Times are medians of `reps` calls after a warm-up, host-side wall clock around the
whole call (uploads and the read-back included). A second pass with the context's event timers on
(vc_ctx_enable_timing: hipEvents around each launch) gives the kernels' own times: the verify
kernel, and the batch path's prep kernel.
usage: kzg_verify_bls_probe.py [--out DIR] [--reps N] [--sizes a,b,c] [--host-n N] [--curves a,b]
Writes DIR/probe.json (default: profiles/r14/kzg_verify_bls under the repository root)."""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import kzg_prove_many_probe as pm  # noqa: E402
import vkzg  # noqa: E402
from vkzg import scheme  # noqa: E402
from vkzg._lib import check, lib  # noqa: E402

SECRET = 100
KERNELS = {"bn254": ("kzg_verify", "kzg_batch_prep"), "bls12_381": ("kzg_verify_bls", "kzg_bls_batch_prep")}


def openings(e, kz, n):
    """(com_xy, com_inf, points, proof_xy, proof_inf, y) of n valid openings, the ABI's arrays"""
    data, pts = pm.openings(n, 12 + n)
    cxy, cinf = e.msm_batch(kz.table, data, pm.N)
    out = (np.zeros((n, 2 * e.nl), dtype=np.uint64), np.zeros(n, dtype=np.uint8), np.zeros((n, 4), dtype=np.uint64))
    pm.many(lib(), e, kz.table, n, data, pts, out)
    return (np.ascontiguousarray(cxy, dtype=np.uint64), np.ascontiguousarray(cinf, dtype=np.uint8), pts) + out


def batch_call(L, e, vk, n, a, seed):
    P = scheme._p
    res = ctypes.c_int()
    check(L.vc_kzg_verify_batch(e.h, vk.h, n, P(a[0]), P(a[1]), P(a[2]), P(a[3]), P(a[4]), P(a[5]), P(seed),
                                ctypes.byref(res), None), "kzg_verify_batch")
    return res.value


def many_call(L, e, vk, n, a, out):
    P = scheme._p
    check(L.vc_kzg_verify_many(e.h, vk.h, n, P(a[0]), P(a[1]), P(a[2]), P(a[3]), P(a[4]), P(a[5]), P(out)),
          "kzg_verify_many")


def host_call(L, vk, a, lo, hi):
    P = scheme._p
    res = ctypes.c_int()
    ok = 0
    for i in range(lo, hi):
        check(L.vc_kzg_verify(vk.h, P(a[0][i]), int(a[1][i]), P(a[2][i]), P(a[3][i]), int(a[4][i]), P(a[5][i]),
                              ctypes.byref(res)), "kzg_verify")
        ok += res.value
    return ok


def median_s(fn, reps):
    ts = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def run_curve(curve, sizes, reps, host_n):
    L = lib()
    e = vkzg.Engine(curve, 0)
    kz = scheme.KZG(e, pm.N, secret=SECRET)
    vk = kz.verifying_key()
    seed = np.frombuffer(bytes(range(32)), dtype=np.uint8).copy()
    kv, kp = KERNELS[curve]
    res = {"verify_many": {}, "verify_batch": {}, "kernel_ms": {}, "host": {}}
    for n in sizes:
        a = openings(e, kz, n)
        out = np.zeros(n, dtype=np.uint8)
        assert batch_call(L, e, vk, n, a, seed) == 1
        many_call(L, e, vk, n, a, out)
        assert out.all()
        bad = [x.copy() for x in a]
        bad[5][n // 2, 0] ^= 1                          # one y changed
        assert batch_call(L, e, vk, n, bad, seed) == 0
        many_call(L, e, vk, n, bad, out)
        assert [int(i) for i in np.flatnonzero(out == 0)] == [n // 2]
        m = median_s(lambda: many_call(L, e, vk, n, a, out), reps)
        b = median_s(lambda: batch_call(L, e, vk, n, a, seed), reps)
        res["verify_many"][str(n)] = {"seconds": m, "openings_per_s": n / m}
        res["verify_batch"][str(n)] = {"seconds": b, "openings_per_s": n / b}
        # the kernels' own times, hipEvents around the launches
        e.enable_timing(True)
        e.reset_timing()
        for _ in range(reps):
            many_call(L, e, vk, n, a, out)
            batch_call(L, e, vk, n, a, seed)
        (vms, vc), (pms, pc) = e.kernel_time(kv), e.kernel_time(kp)
        e.enable_timing(False)
        res["kernel_ms"][str(n)] = {kv: vms / max(vc, 1), kp: pms / max(pc, 1), "launches": [vc, pc]}
        print(f"{curve} n = {n:6d}: verify_many {m * 1e3:9.2f} ms (kernel {vms / max(vc, 1):9.2f} ms), "
              f"verify_batch {b * 1e3:8.3f} ms (prep kernel {pms / max(pc, 1):.3f} ms)", flush=True)
        if n == sizes[0]:
            hn = min(host_n, n)
            t1 = median_s(lambda: host_call(L, vk, a, 0, hn), reps)
            assert host_call(L, vk, a, 0, hn) == hn
            with ThreadPoolExecutor(16) as ex:
                cuts = [hn * k // 16 for k in range(17)]
                t16 = median_s(lambda: list(ex.map(lambda k: host_call(L, vk, a, cuts[k], cuts[k + 1]), range(16))), reps)
            res["host"] = {"n": hn, "threads_1": {"seconds": t1, "openings_per_s": hn / t1},
                           "threads_16": {"seconds": t16, "openings_per_s": hn / t16}}
            print(f"{curve} host vc_kzg_verify x {hn}: 1 thread {t1 * 1e3:.1f} ms, 16 threads {t16 * 1e3:.1f} ms", flush=True)
    e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "kzg_verify_bls"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="256,4096,65536")
    ap.add_argument("--host-n", type=int, default=64)
    ap.add_argument("--curves", default="bls12_381,bn254")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    res = {"reps": a.reps, "width": pm.N, "sizes": sizes}
    for curve in a.curves.split(","):
        res[curve] = run_curve(curve, sizes, a.reps, a.host_n)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

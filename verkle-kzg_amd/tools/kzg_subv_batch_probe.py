"""KZG subvector batch verification latency: vc_kzg_verify_subvector_batch at N = 256, K = 64 over n
proofs of k indices each, made by the GPU prover (vc_kzg_prove_subvector_many over n distinct random
rows, the commitments by vc_msm_batch), beside the only other route: n calls of
vc_kzg_verify_subvector, timed on the first 256 proofs on one host thread and scaled where n is larger
(the JSON says so), on the same machine in the same run.

Times are the median [min, max] of `reps` whole calls after a warm-up, host-side wall clock around the
call with its uploads; the first call of the run also makes the key's line tables, which is why the
warm-up is not counted. Every timed call must accept; one more call with one changed y must reject.
--crossover: the smallest n at k = K = 64 at which the batch call beats n single calls (n = 1, 2, 4, ..).
--split (run it with VKZG_HOST_TIMING=1 in the environment): one call per shape with the context's
kernel timers on; the library's own phase line (upload, fold, msm, pairing, us) is read back from
stderr. The phase line's laps synchronise the stream, so its call time is not the timed one.
usage: kzg_subv_batch_probe.py [--out DIR] [--reps N] [--sizes a,b,c] [--ks a,b,c] [--split] [--crossover]
Writes DIR/probe.json, or DIR/split.json with --split (default DIR: profiles/r18/kzg_subvector_batch
under the repository root)."""
import argparse
import ctypes
import json
import os
import re
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

import vkzg  # noqa: E402
from vkzg import scheme  # noqa: E402
from vkzg._lib import check, lib  # noqa: E402

N, K = 256, 64
P = scheme._p
SEED = np.frombuffer(bytes(range(32)), dtype=np.uint8).copy()


def statements(n, k, seed):
    """n rows of N values below 2^252 and one set of k distinct indices per row, in random order"""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2**63, size=(n, N, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, N, 4), dtype=np.uint64)
    data[:, :, 3] >>= 4
    idx = np.argsort(rng.random((n, N)), axis=1)[:, :k].astype(np.uint32)
    off = (np.arange(n + 1, dtype=np.uint64) * k).astype(np.uint32)
    return np.ascontiguousarray(data.reshape(n * N, 4)), np.ascontiguousarray(idx.reshape(-1)), off


def proofs(L, e, kz, n, k, seed):
    data, idx, off = statements(n, k, seed)
    pxy, pinf, y = np.zeros((n, 8), dtype=np.uint64), np.zeros(n, dtype=np.uint8), np.zeros((n * k, 4), dtype=np.uint64)
    check(L.vc_kzg_prove_subvector_many(e.h, kz.table, N, n, N, P(data), None, P(off), P(idx), n, P(pxy), P(pinf), P(y)),
          "kzg_prove_subvector_many")
    cxy, cinf = e.msm_batch(kz.table, data, N)
    return np.ascontiguousarray(cxy), np.ascontiguousarray(cinf), off, idx, y, pxy, pinf


def batch(L, e, key, n, st, y=None):
    cxy, cinf, off, idx, y0, pxy, pinf = st
    res = ctypes.c_int(-1)
    check(L.vc_kzg_verify_subvector_batch(e.h, key.h, n, P(cxy), P(cinf), P(off), P(idx), P(y0 if y is None else y), P(pxy),
                                          P(pinf), P(SEED), ctypes.byref(res), None), "kzg_verify_subvector_batch")
    return res.value


def singles(L, key, m, k, st):
    cxy, cinf, off, idx, y, pxy, pinf = st
    res = ctypes.c_int(-1)
    ok = 0
    for j in range(m):
        check(L.vc_kzg_verify_subvector(key.h, P(cxy[j]), int(cinf[j]), P(idx[j * k:(j + 1) * k]), k,
                                        P(y[j * k:(j + 1) * k]), P(pxy[j]), int(pinf[j]), ctypes.byref(res)),
              "kzg_verify_subvector")
        ok += res.value
    return ok


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}


def phase_line(fn):
    """run fn with stderr going to a file; the library's [kzg_verify_subvector_batch] line as a dict (us)"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    line = [ln for ln in text.splitlines() if ln.startswith("[kzg_verify_subvector_batch]")]
    if not line:
        return {}
    return {name.strip().replace(" ", "_") + "_us": float(v)
            for name, v in re.findall(r"(upload|fold|msm|whole fold|pairing|call) ([0-9.]+) us", line[-1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "kzg_subvector_batch"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="64,4096,65536")
    ap.add_argument("--ks", default="4,16,64")
    ap.add_argument("--single-sample", type=int, default=256)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--crossover", action="store_true")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    ks = [int(s) for s in a.ks.split(",")]
    L = lib()
    e = vkzg.Engine("bn254", 0)
    kz = scheme.KZG(e, N, secret=100)
    e.fixed_base_precompute(kz.table, 16)
    key = kz.subvector_key(K)
    res = {"N": N, "K": K, "reps": a.reps, "batch": {}, "singles": {}, "split": {}, "crossover": {}}
    for n in sizes:
        for k in ks:
            tag = f"n{n}_k{k}"
            st = proofs(L, e, kz, n, k, 19 * n + k)
            if a.split:
                assert batch(L, e, key, n, st) == 1, tag          # warm-up: the tables, the workspaces
                e.enable_timing(True)
                e.reset_timing()
                ph = phase_line(lambda: batch(L, e, key, n, st))
                ph["fold_kernel_ms"] = e.kernel_time("kzg_subv_fold")[0]
                ph["sum_kernel_ms"] = e.kernel_time("kzg_subv_sum")[0]
                e.enable_timing(False)
                res["split"][tag] = ph
                print(f"n = {n:6d} k = {k:2d}: " + ", ".join(f"{name} {v:.1f}" for name, v in ph.items()), flush=True)
                continue
            ts = []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                ok = batch(L, e, key, n, st)
                if rep:
                    ts.append(time.perf_counter() - t0)
                assert ok == 1, tag
            bad_y = st[4].copy()
            bad_y[(n // 2) * k, 0] ^= 1
            assert batch(L, e, key, n, st, bad_y) == 0, tag
            m = min(n, a.single_sample)
            t0 = time.perf_counter()
            assert singles(L, key, m, k, st) == m, tag
            one = (time.perf_counter() - t0) * n / m
            b = stats(ts)
            res["batch"][tag] = dict(b, proofs_per_s=n / b["median_s"])
            res["singles"][tag] = {"scaled_s": one, "measured_proofs": m, "scaled": bool(m < n)}
            print(f"n = {n:6d} k = {k:2d}: batch {b['median_s'] * 1e3:.3f} ms [{b['min_s'] * 1e3:.3f}, "
                  f"{b['max_s'] * 1e3:.3f}], {n} single calls {one * 1e3:.1f} ms"
                  f"{' (scaled from %d)' % m if m < n else ''}: {one / b['median_s']:.1f} x", flush=True)
            del st
    if a.crossover:
        n = 1
        while n <= 64:
            st = proofs(L, e, kz, n, K, 23 * n)
            ts = []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                ok = batch(L, e, key, n, st)
                if rep:
                    ts.append(time.perf_counter() - t0)
                assert ok == 1
            t0 = time.perf_counter()
            assert singles(L, key, n, K, st) == n
            one = time.perf_counter() - t0
            res["crossover"][f"n{n}"] = {"batch_s": float(np.median(ts)), "singles_s": one}
            print(f"crossover k = {K}: n = {n}: batch {np.median(ts) * 1e3:.3f} ms, singles {one * 1e3:.3f} ms", flush=True)
            if np.median(ts) < one and "smallest_n" not in res["crossover"]:
                res["crossover"]["smallest_n"] = n
            n *= 2
    e.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "split.json" if a.split else "probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

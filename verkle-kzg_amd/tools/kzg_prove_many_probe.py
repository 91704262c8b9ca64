"""KZG batch proving latency: vc_kzg_prove_many at N = 256 over n distinct random rows, half the
points in the domain and half outside, beside the same openings through vc_kzg_prove (one call per
opening) on the same fixed-base table in the same run.

Times are the median [min, max] of `reps` whole calls after a warm-up, host-side wall clock around
the call, with the rows' upload and the read-back. Above 4,096 openings the single calls are
measured on the first `--single-sample` openings and scaled to n (the JSON says so). Every
compared result is checked: the batched proofs and y equal the single calls'.
The split is the context's per-kernel timers (vc_ctx_enable_timing) over one more call: the rows'
conversion, the lane kernel, the batch inversion, the wave kernel, the commit's kernels; `rest` is
that call's wall time less the kernels (copies, the inversion's host step, launch gaps, waits).
usage: kzg_prove_many_probe.py [--out DIR] [--reps N] [--sizes a,b,c] [--window-bits C] [--single-sample K]
Writes DIR/probe.json (default: profiles/r12/kzg_prove_many under the repository root)."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

import vkzg  # noqa: E402
from vkzg import scheme  # noqa: E402
from vkzg._lib import check, lib  # noqa: E402

N = 256
SPLIT = {"to_mont": ["to_mont"], "lane": ["kzg_many_lane"], "batch_inverse": ["binv_prep", "binv_finish"],
         "wave": ["kzg_many_wave"], "commit": ["fb_commit", "fb_commit_small", "fb_combine", "norm_prep", "norm_finish"]}


def openings(n, seed):
    """n rows of N values below 2^252 and n points: even positions in the domain, odd ones outside"""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2**63, size=(n, N, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, N, 4), dtype=np.uint64)
    data[:, :, 3] >>= 4
    pts = np.zeros((n, 4), dtype=np.uint64)
    pts[0::2, 0] = rng.integers(0, N, size=len(pts[0::2]), dtype=np.uint64)
    odd = len(pts[1::2])
    pts[1::2] = rng.integers(0, 2**63, size=(odd, 4), dtype=np.uint64)
    pts[1::2, 0] |= 1 << 20                                  # not below N
    pts[1::2, 3] >>= 4
    return np.ascontiguousarray(data.reshape(n * N, 4)), np.ascontiguousarray(pts)


def many(L, e, table, n, data, pts, out):
    P = scheme._p
    check(L.vc_kzg_prove_many(e.h, table, N, n, N, P(data), None, P(pts), n, P(out[0]), P(out[1]), P(out[2])),
          "kzg_prove_many")


def singles(L, e, table, k, data, pts, out):
    P = scheme._p
    for i in range(k):
        check(L.vc_kzg_prove(e.h, table, N, P(data[i * N:(i + 1) * N]), N, P(pts[i]), P(out[0][i]), P(out[1][i:i + 1]),
                             P(out[2][i])), "kzg_prove")


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "kzg_prove_many"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,64,4096,65536")
    ap.add_argument("--window-bits", type=int, default=16)
    ap.add_argument("--single-sample", type=int, default=1024)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    L = lib()
    e = vkzg.Engine("bn254", 0)
    kz = scheme.KZG(e, N, secret=100)
    e.fixed_base_precompute(kz.table, a.window_bits)
    res = {"N": N, "reps": a.reps, "window_bits": a.window_bits, "table_bytes": e.fixed_base_table_bytes(kz.table),
           "many": {}, "single": {}, "split_ms": {}}
    for n in sizes:
        data, pts = openings(n, 12 + n)
        out = (np.zeros((n, 8), dtype=np.uint64), np.zeros(n, dtype=np.uint8), np.zeros((n, 4), dtype=np.uint64))
        k = n if n <= 4096 else min(n, a.single_sample)
        ref = (np.zeros((k, 8), dtype=np.uint64), np.zeros(k, dtype=np.uint8), np.zeros((k, 4), dtype=np.uint64))
        tm, ts = [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            many(L, e, kz.table, n, data, pts, out)
            t1 = time.perf_counter()
            singles(L, e, kz.table, k, data, pts, ref)
            t2 = time.perf_counter()
            if rep:
                tm.append(t1 - t0)
                ts.append((t2 - t1) * n / k)
        assert all(np.array_equal(x[:k], y) for x, y in zip(out, ref)), n
        assert not out[1].any()
        res["many"][str(n)] = dict(stats(tm), openings_per_s=n / float(np.median(tm)))
        res["single"][str(n)] = dict(stats(ts), openings_per_s=n / float(np.median(ts)), measured_openings=k,
                                     scaled=bool(k < n))
        # the split: one more call with the per-kernel timers on
        e.enable_timing(True)
        e.reset_timing()
        t0 = time.perf_counter()
        many(L, e, kz.table, n, data, pts, out)
        wall = (time.perf_counter() - t0) * 1e3
        sp = {name: sum(e.kernel_time(kn)[0] for kn in kns) for name, kns in SPLIT.items()}
        sp["launches"] = {kn: e.kernel_time(kn)[1] for kns in SPLIT.values() for kn in kns if e.kernel_time(kn)[1]}
        e.enable_timing(False)
        sp["wall_timed"] = wall
        sp["rest"] = wall - sum(v for key, v in sp.items() if key in SPLIT)
        res["split_ms"][str(n)] = sp
        m, s = res["many"][str(n)], res["single"][str(n)]
        print(f"n = {n:6d}: prove_many {m['median_s'] * 1e3:.3f} ms [{m['min_s'] * 1e3:.3f}, {m['max_s'] * 1e3:.3f}], "
              f"{n} x prove {s['median_s'] * 1e3:.3f} ms [{s['min_s'] * 1e3:.3f}, {s['max_s'] * 1e3:.3f}]"
              f"{' (scaled from %d)' % k if k < n else ''}: {s['median_s'] / m['median_s']:.1f} x", flush=True)
        print("   split (ms): " + ", ".join(f"{key} {v:.3f}" for key, v in sp.items() if key != "launches"), flush=True)
    e.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""KZG subvector proving latency: vc_kzg_prove_subvector_many at N = 256 over n distinct random rows,
one random set of k indices per row, beside the same statements proven without it: vc_kzg_prove_many
of the n k single openings on the same fixed-base table in the same run, then the aggregation
sum c_i pi_i (weights from vc_kzg_subvector_weights, the single proofs uploaded as a base table, one
vc_msm per set).

Times are the median [min, max] of `reps` whole calls after a warm-up, host-side wall clock around
the call, with the rows' upload and the read-back. The aggregation is measured on the first
`--agg-sample` sets and scaled to n (the JSON says so); on those sets the aggregated point must equal
the subvector proof, and the ys of every set must equal the single openings', before any time is
reported. The split is the context's per-kernel timers (vc_ctx_enable_timing) over one more call: the
rows' conversion, the wave kernel, the commit's kernels; `rest` is that call's wall time less the
kernels (copies, launch gaps, waits). The verifier (host code, one thread) is timed at each k on a
key of K = max k powers.
usage: kzg_sub_probe.py [--out DIR] [--reps N] [--sizes a,b,c] [--ks a,b,c] [--window-bits C] [--agg-sample K]
Writes DIR/probe.json (default: profiles/r17/kzg_subvector under the repository root)."""
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
SPLIT = {"to_mont": ["to_mont"], "wave": ["kzg_sub_wave"],
         "commit": ["fb_commit", "fb_commit_small", "fb_combine", "norm_prep", "norm_finish"]}
P = scheme._p


def statements(n, k, seed):
    """n rows of N values below 2^252 and one set of k distinct indices per row, in random order"""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2**63, size=(n, N, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, N, 4), dtype=np.uint64)
    data[:, :, 3] >>= 4
    idx = np.argsort(rng.random((n, N)), axis=1)[:, :k].astype(np.uint32)
    off = (np.arange(n + 1, dtype=np.uint64) * k).astype(np.uint32)
    return np.ascontiguousarray(data.reshape(n * N, 4)), np.ascontiguousarray(idx.reshape(-1)), off


def subvector(L, e, table, n, data, off, idx, out):
    check(L.vc_kzg_prove_subvector_many(e.h, table, N, n, N, P(data), None, P(off), P(idx), n, P(out[0]), P(out[1]),
                                        P(out[2])), "kzg_prove_subvector_many")


def singles(L, e, table, n, data, row, pts, out):
    check(L.vc_kzg_prove_many(e.h, table, N, n, N, P(data), P(row), P(pts), len(row), P(out[0]), P(out[1]), P(out[2])),
          "kzg_prove_many")


def aggregate(L, e, sets, k, idx, single_xy, single_inf, out):
    """sum c_i pi_i of the first `sets` sets: their single proofs as one table, one MSM per set"""
    tid = e.upload_bases(single_xy[:sets * k], single_inf[:sets * k])
    c = np.zeros((k, 4), dtype=np.uint64)
    for s in range(sets):
        check(L.vc_kzg_subvector_weights(0, N, P(idx[s * k:(s + 1) * k]), k, P(c)), "kzg_subvector_weights")
        check(L.vc_msm(e.h, tid, s * k, P(c), k, 0, P(out[0][s]), P(out[1][s:s + 1])), "vc_msm")


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "kzg_subvector"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="64,4096,65536")
    ap.add_argument("--ks", default="4,16,64")
    ap.add_argument("--window-bits", type=int, default=16)
    ap.add_argument("--agg-sample", type=int, default=256)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    ks = [int(s) for s in a.ks.split(",")]
    L = lib()
    e = vkzg.Engine("bn254", 0)
    kz = scheme.KZG(e, N, secret=100)
    e.fixed_base_precompute(kz.table, a.window_bits)
    res = {"N": N, "reps": a.reps, "window_bits": a.window_bits, "table_bytes": e.fixed_base_table_bytes(kz.table),
           "subvector": {}, "singles": {}, "aggregation": {}, "split_ms": {}, "verify": {}}
    for n in sizes:
        for k in ks:
            tag = f"n{n}_k{k}"
            data, idx, off = statements(n, k, 17 * n + k)
            row = np.repeat(np.arange(n, dtype=np.uint32), k)
            pts = np.zeros((n * k, 4), dtype=np.uint64)
            pts[:, 0] = idx
            out = (np.zeros((n, 8), dtype=np.uint64), np.zeros(n, dtype=np.uint8), np.zeros((n * k, 4), dtype=np.uint64))
            one = (np.zeros((n * k, 8), dtype=np.uint64), np.zeros(n * k, dtype=np.uint8),
                   np.zeros((n * k, 4), dtype=np.uint64))
            m = min(n, a.agg_sample)
            agg = (np.zeros((m, 8), dtype=np.uint64), np.zeros(m, dtype=np.uint8))
            tsub, tone, tagg = [], [], []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                subvector(L, e, kz.table, n, data, off, idx, out)
                t1 = time.perf_counter()
                singles(L, e, kz.table, n, data, row, pts, one)
                t2 = time.perf_counter()
                aggregate(L, e, m, k, idx, one[0], one[1], agg)
                t3 = time.perf_counter()
                if rep:
                    tsub.append(t1 - t0)
                    tone.append(t2 - t1)
                    tagg.append((t3 - t2) * n / m)
            assert np.array_equal(out[2], one[2]), tag                  # every y
            assert np.array_equal(out[0][:m], agg[0]) and np.array_equal(out[1][:m], agg[1]), tag
            assert not out[1].any()
            sub, sgl, ag = stats(tsub), stats(tone), stats(tagg)
            res["subvector"][tag] = dict(sub, sets_per_s=n / sub["median_s"])
            res["singles"][tag] = dict(sgl, openings=n * k)
            res["aggregation"][tag] = dict(ag, measured_sets=m, scaled=bool(m < n))
            e.enable_timing(True)
            e.reset_timing()
            t0 = time.perf_counter()
            subvector(L, e, kz.table, n, data, off, idx, out)
            wall = (time.perf_counter() - t0) * 1e3
            sp = {name: sum(e.kernel_time(kn)[0] for kn in kns) for name, kns in SPLIT.items()}
            sp["launches"] = {kn: e.kernel_time(kn)[1] for kns in SPLIT.values() for kn in kns if e.kernel_time(kn)[1]}
            e.enable_timing(False)
            sp["wall_timed"] = wall
            sp["rest"] = wall - sum(v for key, v in sp.items() if key in SPLIT)
            res["split_ms"][tag] = sp
            print(f"n = {n:6d} k = {k:2d}: subvector {sub['median_s'] * 1e3:.3f} ms [{sub['min_s'] * 1e3:.3f}, "
                  f"{sub['max_s'] * 1e3:.3f}], {n * k} single openings {sgl['median_s'] * 1e3:.3f} ms "
                  f"[{sgl['min_s'] * 1e3:.3f}, {sgl['max_s'] * 1e3:.3f}] + aggregation {ag['median_s'] * 1e3:.3f} ms"
                  f"{' (scaled from %d sets)' % m if m < n else ''}: {sgl['median_s'] / sub['median_s']:.1f} x "
                  f"without, {(sgl['median_s'] + ag['median_s']) / sub['median_s']:.1f} x with the aggregation", flush=True)
            print("   split (ms): " + ", ".join(f"{key} {v:.3f}" for key, v in sp.items() if key != "launches"), flush=True)
            del data, one, pts, row
    # the verifier, on this machine's host
    K = max(ks)
    key = kz.subvector_key(K)
    evals = [int(v) for v in np.random.default_rng(5).integers(1, 2**62, size=N)]
    lb = scheme.LagrangeBasis(evals, N)
    com = kz.commit(lb)
    for k in ks:
        S = [int(i) for i in np.random.default_rng(k).permutation(N)[:k]]
        pr = kz.prove_subvector(None, S, lb)
        ts = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            ok = key.verify(com, S, pr["ys"], pr["proof"])
            if rep:
                ts.append(time.perf_counter() - t0)
        assert ok is True
        assert key.verify(com, S, [pr["ys"][0] + 1] + pr["ys"][1:], pr["proof"]) is False
        res["verify"][f"k{k}"] = dict(stats(ts), K=K)
        print(f"verify k = {k:2d}: {np.median(ts) * 1e3:.3f} ms [{min(ts) * 1e3:.3f}, {max(ts) * 1e3:.3f}]", flush=True)
    e.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

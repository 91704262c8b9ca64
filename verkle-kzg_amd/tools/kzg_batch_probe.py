"""KZG batch verification latency: vc_kzg_verify_batch (results = NULL, one combined verdict) at
n = 256, 4096 and 65,536 valid openings, beside vc_kzg_verify_many (one verdict per opening) on
the same inputs in the same run, and the batch call's own split into upload, prep kernel (which
is also the scratch table's fill), MSMs and host pairing.

The openings are synthetic and valid for the public secret s = 100 without a prover run: pi_i =
C_i = a random point of the engine (vc_bases_random), z_i = 99 (>= size, so p_i = 99 and s - p_i =
1) and y_i = 0, i.e. pi_i (s - p_i) == C_i - y_i G. The table's 2n entries are n distinct points.
Every verdict is checked (the batch accepts; with one y changed it rejects). Times are medians of
`reps` calls after a warm-up, host-side wall clock around the whole call. The split comes from a
child process run with VKZG_HOST_TIMING=1 (the library prints the phases, synchronising between
them, so their sum exceeds the untimed call).
With --real the openings are a prover's: n random rows of a 256-point key, committed by
vc_msm_batch and opened by vc_kzg_prove_many, every other point in the domain (the rows and points
of tools/kzg_prove_many_probe.py); the result goes to DIR/probe_real.json.
usage: kzg_batch_probe.py [--out DIR] [--reps N] [--sizes a,b,c] [--real]
Writes DIR/probe.json (default: profiles/r10/kzg_verify_batch under the repository root)."""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

import vkzg  # noqa: E402
from vkzg import scheme  # noqa: E402
from vkzg._lib import check, lib  # noqa: E402

SECRET, SIZE = 100, 16


def openings(e, n):
    tid = e.random_bases(n, seed=1000 + n)
    xy, inf = e.download_bases(tid)
    xy = np.ascontiguousarray(xy, dtype=np.uint64)
    inf = np.ascontiguousarray(inf, dtype=np.uint8)
    pts = np.ascontiguousarray(np.tile(vkzg.ints_to_limbs([SECRET - 1], 4), (n, 1)))
    ys = np.zeros((n, 4), dtype=np.uint64)
    return xy, inf, pts, xy.copy(), inf.copy(), ys


def real_openings(e, n):
    import kzg_prove_many_probe as pm
    kz = getattr(e, "_probe_kzg", None)
    if kz is None:
        kz = e._probe_kzg = scheme.KZG(e, pm.N, secret=SECRET)
    data, pts = pm.openings(n, 12 + n)
    cxy, cinf = e.msm_batch(kz.table, data, pm.N)
    out = (np.zeros((n, 8), dtype=np.uint64), np.zeros(n, dtype=np.uint8), np.zeros((n, 4), dtype=np.uint64))
    pm.many(lib(), e, kz.table, n, data, pts, out)
    return (np.ascontiguousarray(cxy, dtype=np.uint64), np.ascontiguousarray(cinf, dtype=np.uint8), pts) + out


def batch_call(L, e, vk, n, a, seed):
    P = scheme._p
    res = ctypes.c_int()
    check(L.vc_kzg_verify_batch(e.h, vk.h, n, P(a[0]), P(a[1]), P(a[2]), P(a[3]), P(a[4]), P(a[5]), P(seed),
                                ctypes.byref(res), None), "kzg_verify_batch")
    return res.value


def split(sizes, reps, real):
    """child: the timed phases of `reps` calls per size on stderr (VKZG_HOST_TIMING=1)"""
    L = lib()
    e = vkzg.Engine("bn254", 0)
    vk = scheme.KZGVerifyingKey(scheme.kzg_g2_from_secret(SECRET), 256 if real else SIZE)
    seed = np.frombuffer(bytes(range(32)), dtype=np.uint8).copy()
    for n in sizes:
        a = (real_openings if real else openings)(e, n)
        for _ in range(reps + 1):
            assert batch_call(L, e, vk, n, a, seed) == 1
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "kzg_verify_batch"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="256,4096,65536")
    ap.add_argument("--split-child", action="store_true")
    ap.add_argument("--real", action="store_true")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.split_child:
        split(sizes, a.reps, a.real)
        return
    res = {"reps": a.reps, "real_openings": a.real, "batch": {}, "many": {}, "split_us": {}}
    # the split first, in a process of its own (the timing switch is read once per process)
    env = dict(os.environ, VKZG_HOST_TIMING="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--split-child", "--reps", str(a.reps),
                            "--sizes", a.sizes] + (["--real"] if a.real else []), env=env, stderr=subprocess.PIPE, text=True, timeout=900)
    if child.returncode != 0:
        sys.stderr.write(child.stderr[-4000:])
        raise SystemExit(f"split child failed with status {child.returncode}")
    laps = {}
    pat = re.compile(r"\[kzg_verify_batch\] n=(\d+) chunks=(\d+): upload ([\d.]+) us, prep ([\d.]+) us, msm ([\d.]+) us, "
                     r"fold ([\d.]+) us, pairing ([\d.]+) us, call ([\d.]+) us")
    for m in pat.finditer(child.stderr):
        laps.setdefault(int(m.group(1)), []).append([float(m.group(k)) for k in range(3, 9)])
    for n, rows in laps.items():
        med = np.median(np.array(rows[1:]), axis=0)     # (the first call warms up)
        res["split_us"][str(n)] = dict(zip(("upload", "prep", "msm", "fold", "pairing", "call"), [float(v) for v in med]))
        print(f"split n = {n:6d}: " + ", ".join(f"{k} {v:.0f} us" for k, v in res["split_us"][str(n)].items()), flush=True)

    L = lib()
    P = scheme._p
    e = vkzg.Engine("bn254", 0)
    vk = scheme.KZGVerifyingKey(scheme.kzg_g2_from_secret(SECRET), 256 if a.real else SIZE)
    seed = np.frombuffer(bytes(range(32)), dtype=np.uint8).copy()
    for n in sizes:
        arr = (real_openings if a.real else openings)(e, n)
        tb, tm = [], []
        out = np.zeros(n, dtype=np.uint8)
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            ok = batch_call(L, e, vk, n, arr, seed)
            t1 = time.perf_counter()
            check(L.vc_kzg_verify_many(e.h, vk.h, n, P(arr[0]), P(arr[1]), P(arr[2]), P(arr[3]), P(arr[4]), P(arr[5]),
                                       P(out)), "kzg_verify_many")
            t2 = time.perf_counter()
            assert ok == 1 and out.all()
            if rep:
                tb.append(t1 - t0)
                tm.append(t2 - t1)
        bad = [x.copy() for x in arr]
        bad[5][n // 2, 0] ^= 1                          # one y changed: the batch is rejected
        assert batch_call(L, e, vk, n, bad, seed) == 0
        b, m = float(np.median(tb)), float(np.median(tm))
        res["batch"][str(n)] = {"seconds": b, "openings_per_s": n / b}
        res["many"][str(n)] = {"seconds": m, "openings_per_s": n / m}
        print(f"n = {n:6d}: verify_batch {b * 1e3:.3f} ms, verify_many {m * 1e3:.2f} ms ({m / b:.1f} x)", flush=True)
    e.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "probe_real.json" if a.real else "probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

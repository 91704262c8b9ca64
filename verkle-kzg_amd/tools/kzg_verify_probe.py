"""KZG verification throughput: vc_kzg_verify_many on the GPU at n = 256, 4096 and 65,536
openings, beside the host verifier vc_kzg_verify on 1 thread and on 16 threads (the thing to
compare against: a caller without this kernel would spread the openings over its cores).

The openings are the valid and tampered entries of tests/golden/kzg_verify_16.json, tiled; every
verdict is checked against the fixture's. Times are medians of `reps` calls after a warm-up,
host-side wall clock around the whole call (uploads and the read-back included).
usage: kzg_verify_probe.py [--out DIR] [--reps N] [--host-n N]
Writes DIR/kzg_verify_probe.json (default: profiles/r07/kzg_verify under the repository root)."""
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
import numpy as np  # noqa: E402

import vkzg  # noqa: E402
from vkzg import scheme  # noqa: E402
from vkzg._lib import check, lib  # noqa: E402


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "kzg_verify_16.json")) as f:
        g = json.load(f)
    pt = lambda h: None if h is None else (int(h[0], 16), int(h[1], 16))  # noqa: E731
    g2 = tuple(tuple(int(v, 16) for v in c) for c in g["g2"])
    return g2, g["size"], [(pt(e["commitment"]), int(e["point"], 16), pt(e["proof"]), int(e["y"], 16), e["valid"])
                           for e in g["entries"]]


def arrays(entries, n):
    """the fixture tiled to n openings, in the ABI's layout"""
    m = len(entries)
    cxy, cinf = scheme._pt_arrays([e[0] for e in entries])
    pxy, pinf = scheme._pt_arrays([e[2] for e in entries])
    pts = vkzg.ints_to_limbs([e[1] for e in entries], 4)
    ys = vkzg.ints_to_limbs([e[3] for e in entries], 4)
    want = np.array([e[4] for e in entries], dtype=np.uint8)
    idx = np.arange(n) % m
    return [np.ascontiguousarray(a[idx]) for a in (cxy, cinf, pts, pxy, pinf, ys, want)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "kzg_verify"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=1024)
    a = ap.parse_args()
    g2, size, entries = fixture()
    vk = scheme.KZGVerifyingKey(g2, size)
    L = lib()
    P = scheme._p
    res = {"gpu": {}, "host": {}}

    # ---- host: one opening per call, 1 thread and 16 threads (ctypes drops the GIL in the call)
    cxy, cinf, pts, pxy, pinf, ys, want = arrays(entries, a.host_n)

    def host_range(lo, hi):
        out = ctypes.c_int()
        bad = 0
        for i in range(lo, hi):
            check(L.vc_kzg_verify(vk.h, P(cxy[i]), int(cinf[i]), P(pts[i]), P(pxy[i]), int(pinf[i]), P(ys[i]),
                                  ctypes.byref(out)), "kzg_verify")
            bad += out.value != want[i]
        return bad

    for threads in (1, 16):
        n = a.host_n if threads > 1 else max(64, a.host_n // 8)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            if threads == 1:
                bad = host_range(0, n)
            else:
                step = (n + threads - 1) // threads
                with ThreadPoolExecutor(threads) as ex:
                    bad = sum(ex.map(lambda k: host_range(k * step, min(n, (k + 1) * step)), range(threads)))
            ts.append(time.perf_counter() - t0)
            assert bad == 0
        t = float(np.median(ts))
        res["host"][f"{threads}_threads"] = {"n": n, "seconds": t, "openings_per_s": n / t, "us_per_opening": 1e6 * t / n}
        print(f"host {threads:2d} threads: {n} openings in {t * 1e3:.1f} ms = {n / t:.0f} /s", flush=True)

    # ---- GPU
    e = vkzg.Engine("bn254", 0)
    for n in (256, 4096, 65536):
        cxy, cinf, pts, pxy, pinf, ys, want = arrays(entries, n)
        out = np.zeros(n, dtype=np.uint8)
        ts = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            check(L.vc_kzg_verify_many(e.h, vk.h, n, P(cxy), P(cinf), P(pts), P(pxy), P(pinf), P(ys), P(out)),
                  "kzg_verify_many")
            if rep:
                ts.append(time.perf_counter() - t0)
            assert np.array_equal(out, want)
        t = float(np.median(ts))
        res["gpu"][str(n)] = {"seconds": t, "openings_per_s": n / t, "us_per_opening": 1e6 * t / n}
        print(f"gpu n = {n:6d}: {t * 1e3:.2f} ms = {n / t:.0f} /s", flush=True)
    e.close()
    h16 = res["host"]["16_threads"]["openings_per_s"]
    res["gpu_65536_over_host_16_threads"] = res["gpu"]["65536"]["openings_per_s"] / h16
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "kzg_verify_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

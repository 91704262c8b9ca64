"""IPA batch verification throughput: vc_ipa_verify_many at N = 256 (BN254) over n = 1, 64, 4096 and
65,536 distinct valid openings, beside vc_ipa_verify one opening per call -- the only way to do the
job without the batched call -- measured in the same run.

The openings come from the engine's own prover (vc_ipa_prove, batched): 256 seeded data vectors,
a distinct point per opening (every fourth below N, the rest seeded 200-bit values). Every verdict
must be 1. Times are host wall clock around the whole call (uploads and the read-back included):
median, min and max of `reps` calls after one warm-up; the single call the median of 8.
The stage laps (VKZG_HOST_TIMING: transcripts, field kernel, fixed commit, curve kernel -- with
the stream synchronised between stages, so their sum exceeds the untimed call) come from a child
process, one warm-up and one timed call per n.
usage: ipa_verify_many_probe.py [--out DIR] [--reps N] [--sizes 1,64,4096,65536]
Writes DIR/probe.json (default: profiles/r09/ipa_verify_many under the repository root)."""
import argparse
import ctypes
import json
import os
import re
import subprocess
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

N, K = 256, 8
P = scheme._p
NAMES = ("com_xy", "com_inf", "points", "l_xy", "l_inf", "r_xy", "r_inf", "tip", "y")


def setup(e):
    crs = scheme.ipa_crs(N + 1, max_=512)
    return scheme.IPA(e, N, crs)


def make_openings(e, ipa, n, seed=9):
    """n openings in vc_ipa_verify_many's flat layout, proved in batches of 2048 straight into it"""
    rng = np.random.default_rng(seed)
    nd = min(n, 256)
    data = rng.integers(0, 1 << 63, size=(nd, N, 4), dtype=np.uint64)
    data[:, :, 3] >>= np.uint64(3)  # below 2^252 < r
    cxy = np.zeros((nd, 8), dtype=np.uint64)
    cinf = np.zeros(nd, dtype=np.uint8)
    check(lib().vc_ipa_commit(e.h, ipa.table, N, P(data), nd, P(cxy), P(cinf)), "ipa_commit")
    pts = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    pts[:, 3] >>= np.uint64(55)  # 200-bit values
    small = np.arange(n) % 4 == 0
    pts[small, 1:] = 0
    pts[small, 0] %= np.uint64(N)
    a = {"com_xy": np.ascontiguousarray(cxy[np.arange(n) % nd]), "com_inf": np.ascontiguousarray(cinf[np.arange(n) % nd]),
         "points": pts, "l_xy": np.zeros((n, K, 8), dtype=np.uint64), "l_inf": np.zeros((n, K), dtype=np.uint8),
         "r_xy": np.zeros((n, K, 8), dtype=np.uint64), "r_inf": np.zeros((n, K), dtype=np.uint8),
         "tip": np.zeros((n, 4), dtype=np.uint64), "y": np.zeros((n, 4), dtype=np.uint64)}
    step = 2048
    for lo in range(0, n, step):
        b = min(step, n - lo)
        arr = (scheme._ProofBuf * b)()
        for i in range(b):
            p = lo + i
            arr[i].rounds = K
            arr[i].l_xy, arr[i].l_inf = a["l_xy"][p].ctypes.data, a["l_inf"][p].ctypes.data
            arr[i].r_xy, arr[i].r_inf = a["r_xy"][p].ctypes.data, a["r_inf"][p].ctypes.data
        d = np.ascontiguousarray(data[(lo + np.arange(b)) % nd])
        check(lib().vc_ipa_prove(e.h, ipa.table, N, P(d), P(a["com_xy"][lo:lo + b]), P(a["com_inf"][lo:lo + b]),
                                 P(pts[lo:lo + b]), b, None, ctypes.cast(arr, ctypes.c_void_p)), "ipa_prove")
        raw = np.frombuffer(arr, dtype=np.uint8).reshape(b, ctypes.sizeof(scheme._ProofBuf))
        off = scheme._ProofBuf.tip.offset
        a["tip"][lo:lo + b] = raw[:, off:off + 32].copy().view(np.uint64)
        a["y"][lo:lo + b] = raw[:, off + 32:off + 64].copy().view(np.uint64)
        if (lo // step) % 8 == 7:
            print(f"  proved {lo + b} / {n}", flush=True)
    return a


def verify_many(e, ipa, a, out):
    n = len(out)
    check(lib().vc_ipa_verify_many(e.h, ipa.table, N, n, *[P(a[k]) for k in NAMES], None, P(out)), "ipa_verify_many")


def laps_child(paths):
    """one warm-up and one timed call per saved batch, the library's lap lines on stderr"""
    e = vkzg.Engine("bn254", 0)
    ipa = setup(e)
    for path in paths:
        a = dict(np.load(path))
        out = np.zeros(len(a["com_inf"]), dtype=np.uint8)
        for _ in range(2):
            verify_many(e, ipa, a, out)
        assert out.all()
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "ipa_verify_many"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,64,4096,65536")
    ap.add_argument("--laps-child", nargs="*", default=None)
    a = ap.parse_args()
    if a.laps_child is not None:
        return laps_child(a.laps_child)
    sizes = [int(s) for s in a.sizes.split(",")]
    e = vkzg.Engine("bn254", 0)
    ipa = setup(e)
    t0 = time.perf_counter()
    full = make_openings(e, ipa, max(sizes))
    print(f"proved {max(sizes)} openings in {time.perf_counter() - t0:.1f} s", flush=True)
    res = {"N": N, "curve": "bn254", "reps": a.reps, "batched": {}}

    # ---- the single call, one opening at a time
    L = lib()
    ts = []
    out1 = ctypes.c_int()
    for i in range(9):
        b = scheme._ProofBuf(K, full["l_xy"][i].ctypes.data, full["l_inf"][i].ctypes.data, full["r_xy"][i].ctypes.data,
                             full["r_inf"][i].ctypes.data)
        b.tip[:] = [int(v) for v in full["tip"][i]]
        b.y[:] = [int(v) for v in full["y"][i]]
        t0 = time.perf_counter()
        check(L.vc_ipa_verify(e.h, ipa.table, N, P(full["com_xy"][i]), int(full["com_inf"][i]), P(full["points"][i]),
                              ctypes.byref(b), None, ctypes.byref(out1)), "ipa_verify")
        if i:
            ts.append(time.perf_counter() - t0)
        assert out1.value == 1
    single = float(np.median(ts))
    res["single_call_ms"] = single * 1e3
    print(f"vc_ipa_verify: {single * 1e3:.3f} ms per opening (median of 8)", flush=True)

    tmp = tempfile.mkdtemp(prefix="ipa_verify_many_probe_")
    paths = []
    for n in sizes:
        sub = {k: np.ascontiguousarray(v[:n]) for k, v in full.items()}
        out = np.zeros(n, dtype=np.uint8)
        ts = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            verify_many(e, ipa, sub, out)
            if rep:
                ts.append(time.perf_counter() - t0)
            assert out.all()
        t = float(np.median(ts))
        res["batched"][str(n)] = {"ms": t * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3, "proofs_per_s": n / t,
                                  "n_x_single_ms": n * single * 1e3, "ratio_n_x_single_over_batched": n * single / t,
                                  "gap_ms": (n * single - t) * 1e3, "spread_ms": (max(ts) - min(ts)) * 1e3}
        print(f"n = {n:6d}: {t * 1e3:.2f} ms [{min(ts) * 1e3:.2f}, {max(ts) * 1e3:.2f}] = {n / t:.0f} /s; "
              f"n x single = {n * single * 1e3:.1f} ms, ratio {n * single / t:.1f}", flush=True)
        paths.append(os.path.join(tmp, f"n{n}.npz"))
        np.savez(paths[-1], **sub)
    e.close()

    # ---- stage laps from a child process (the library reads VKZG_HOST_TIMING once)
    env = dict(os.environ, VKZG_HOST_TIMING="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--laps-child", *paths], env=env,
                           stderr=subprocess.PIPE, text=True, timeout=900)
    assert child.returncode == 0, child.stderr[-2000:]
    pat = re.compile(r"\[ipa_verify_many\] n=(\d+) N=\d+ chunks=(\d+): transcripts ([\d.]+) us.*?field ([\d.]+) us, "
                     r"fixed commit ([\d.]+) us, curve ([\d.]+) us, call ([\d.]+) us")
    for m in pat.finditer(child.stderr):  # the second (warm) call of each n overwrites the first
        res["batched"][m.group(1)]["laps_us"] = {"chunks": int(m.group(2)), "transcripts": float(m.group(3)),
                                                 "field_kernel": float(m.group(4)), "fixed_commit": float(m.group(5)),
                                                 "curve_kernel": float(m.group(6)), "call_with_syncs": float(m.group(7))}
    for p in paths:
        os.unlink(p)
    os.rmdir(tmp)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

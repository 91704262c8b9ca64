"""IPA batch verification, one combined verdict: vc_ipa_verify_batch at N = 256 (BN254) over n = 64,
4096 and 65,536 distinct valid openings, beside vc_ipa_verify_many (one verdict each) on the same
inputs in the same run.

The openings are ipa_verify_many_probe.py's (the engine's batched prover, a distinct point per
opening). Times are host wall clock around the whole call (uploads included, results = NULL for the
batched call): median, min and max of `reps` calls after one warm-up. Every combined verdict must
be 1, every per-opening verdict 1.
The stage laps (VKZG_HOST_TIMING, the stream synchronised between stages, so their sum exceeds the
untimed call) come from a child process, one warm-up and one timed call per n.
usage: ipa_batch_probe.py [--out DIR] [--reps N] [--sizes 64,4096,65536]
Writes DIR/probe.json (default: profiles/r13/ipa_verify_batch under the repository root)."""
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
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import vkzg  # noqa: E402
from ipa_verify_many_probe import NAMES, N, P, make_openings, setup, verify_many  # noqa: E402
from vkzg._lib import check, lib  # noqa: E402

SEED = np.frombuffer(bytes(range(32)), dtype=np.uint8).copy()


def verify_batch(e, ipa, a, n):
    res = ctypes.c_int()
    check(lib().vc_ipa_verify_batch(e.h, ipa.table, N, n, *[P(a[k]) for k in NAMES], None, P(SEED), ctypes.byref(res),
                                    None), "ipa_verify_batch")
    return res.value


def laps_child(paths):
    """one warm-up and one timed call per saved batch and call, the library's lap lines on stderr"""
    e = vkzg.Engine("bn254", 0)
    ipa = setup(e)
    for path in paths:
        a = dict(np.load(path))
        n = len(a["com_inf"])
        out = np.zeros(n, dtype=np.uint8)
        for _ in range(2):
            assert verify_batch(e, ipa, a, n) == 1
        for _ in range(2):
            verify_many(e, ipa, a, out)
        assert out.all()
    e.close()


def timed(fn, reps):
    ts = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:
            ts.append(time.perf_counter() - t0)
    return {"ms": float(np.median(ts)) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "ipa_verify_batch"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="64,4096,65536")
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
    res = {"N": N, "curve": "bn254", "reps": a.reps, "sizes": {}}
    tmp = tempfile.mkdtemp(prefix="ipa_batch_probe_")
    paths = []
    for n in sizes:
        sub = {k: np.ascontiguousarray(v[:n]) for k, v in full.items()}
        out = np.zeros(n, dtype=np.uint8)
        verdicts = []
        batch = timed(lambda: verdicts.append(verify_batch(e, ipa, sub, n)), a.reps)
        assert verdicts == [1] * (a.reps + 1), verdicts
        many = timed(lambda: verify_many(e, ipa, sub, out), a.reps)
        assert out.all()
        res["sizes"][str(n)] = {"verify_batch": batch, "verify_many": many, "ratio_many_over_batch": many["ms"] / batch["ms"],
                                "ranges_overlap": not (batch["max_ms"] < many["min_ms"] or many["max_ms"] < batch["min_ms"])}
        print(f"n = {n:6d}: verify_batch {batch['ms']:.2f} ms [{batch['min_ms']:.2f}, {batch['max_ms']:.2f}], "
              f"verify_many {many['ms']:.2f} ms [{many['min_ms']:.2f}, {many['max_ms']:.2f}], "
              f"ratio {many['ms'] / batch['ms']:.2f}", flush=True)
        paths.append(os.path.join(tmp, f"n{n}.npz"))
        np.savez(paths[-1], **sub)
    e.close()

    # ---- stage laps from a child process (the library reads VKZG_HOST_TIMING once)
    env = dict(os.environ, VKZG_HOST_TIMING="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--laps-child", *paths], env=env,
                           stderr=subprocess.PIPE, text=True, timeout=900)
    assert child.returncode == 0, child.stderr[-2000:]
    pat = re.compile(r"\[ipa_verify_batch\] n=(\d+) N=\d+ chunks=(\d+): host transcripts ([\d.]+) us, upload ([\d.]+) us, "
                     r"transcripts ([\d.]+) us, prep ([\d.]+) us, field ([\d.]+) us, msm ([\d.]+) us, "
                     r"fixed commit ([\d.]+) us, call ([\d.]+) us")
    for m in pat.finditer(child.stderr):  # the second (warm) call of each n overwrites the first
        res["sizes"][m.group(1)]["verify_batch"]["laps_us"] = {
            "chunks": int(m.group(2)), "upload": float(m.group(4)), "transcripts_kernel": float(m.group(5)),
            "table_fill": float(m.group(6)), "field_and_rowsum": float(m.group(7)), "msm": float(m.group(8)),
            "fixed_commit": float(m.group(9)), "call_with_syncs": float(m.group(10))}
    pat = re.compile(r"\[ipa_verify_many\] n=(\d+) N=\d+ chunks=(\d+): transcripts ([\d.]+) us.*?field ([\d.]+) us, "
                     r"fixed commit ([\d.]+) us, curve ([\d.]+) us, call ([\d.]+) us")
    for m in pat.finditer(child.stderr):
        res["sizes"][m.group(1)]["verify_many"]["laps_us"] = {
            "chunks": int(m.group(2)), "transcripts": float(m.group(3)), "field_kernel": float(m.group(4)),
            "fixed_commit": float(m.group(5)), "curve_kernel": float(m.group(6)), "call_with_syncs": float(m.group(7))}
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

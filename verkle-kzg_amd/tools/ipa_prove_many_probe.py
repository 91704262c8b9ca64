"""IPA batch proving: vc_ipa_prove_many at N = 256 (BN254) over n = 1, 256, 4096 and 65,536 openings,
beside vc_ipa_prove with batch = n on the same seeded inputs, both through the bare C ABI.

The inputs are one data row, its commitment and a distinct point per opening (every fourth below N,
the rest seeded 200-bit values); vc_ipa_prove_many takes the same n x N array of rows (row == NULL),
so both calls move the same data. Times are host wall clock around the whole call (uploads and
read-backs included): median, min and max of `reps` calls after one warm-up. The outputs of the two
calls must be equal byte for byte (compared through a SHA-256 over the six flat arrays).
vc_ipa_prove runs in a child process, from this build or, with --baseline-tree, from another
checkout's verkle-kzg_amd directory (its vkzg package and its built lib/: the parent commit's, to
compare against it; vc_ipa_prove itself is the same code in both).
The stage laps (VKZG_HOST_TIMING, the stream synchronised between stages, so their sum exceeds the
untimed call) come from a child process too, one warm-up and one timed call per n.
usage: ipa_prove_many_probe.py [--out DIR] [--reps N] [--sizes 1,256,4096,65536] [--baseline-tree DIR]
Writes DIR/probe.json (default: profiles/r19/ipa_prove_many under the repository root)."""
import argparse
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
# (the baseline child imports the package, and with it the library, of the tree it measures)
_TREE = None
if "--baseline-tree" in sys.argv and "baseline" in sys.argv:
    _TREE = os.path.abspath(sys.argv[sys.argv.index("--baseline-tree") + 1])
sys.path.insert(0, _TREE or os.path.dirname(HERE))
import numpy as np  # noqa: E402

import vkzg  # noqa: E402
from vkzg import scheme  # noqa: E402
from vkzg._lib import check, lib  # noqa: E402

N, K = 256, 8
P = scheme._p
OUTS = ("l_xy", "l_inf", "r_xy", "r_inf", "tip", "y")


def setup(e):
    return scheme.IPA(e, N, scheme.ipa_crs(N + 1, max_=512))


def make_inputs(e, ipa, n, seed=19):
    """n rows (256 distinct seeded ones, repeated), their commitments, a distinct point each"""
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
    pick = np.arange(n) % nd
    return {"data": np.ascontiguousarray(data[pick]), "com_xy": np.ascontiguousarray(cxy[pick]),
            "com_inf": np.ascontiguousarray(cinf[pick]), "points": pts}


def outputs(n):
    return {"l_xy": np.zeros((n, K, 8), dtype=np.uint64), "l_inf": np.zeros((n, K), dtype=np.uint8),
            "r_xy": np.zeros((n, K, 8), dtype=np.uint64), "r_inf": np.zeros((n, K), dtype=np.uint8),
            "tip": np.zeros((n, 4), dtype=np.uint64), "y": np.zeros((n, 4), dtype=np.uint64)}


def digest(o):
    h = hashlib.sha256()
    for k in OUTS:
        h.update(np.ascontiguousarray(o[k]).tobytes())
    return h.hexdigest()


def prove_many(e, ipa, a, o, n):
    check(lib().vc_ipa_prove_many(e.h, ipa.table, N, n, P(a["data"]), None, P(a["com_xy"]), P(a["com_inf"]),
                                  P(a["points"]), n, *[P(o[k]) for k in OUTS]), "ipa_prove_many")


def proof_structs(o, n):
    """vc_ipa_prove's proof structs pointing straight into the flat arrays"""
    arr = (scheme._ProofBuf * n)()
    lx, li, rx, ri = (o[k].ctypes.data for k in ("l_xy", "l_inf", "r_xy", "r_inf"))
    for i in range(n):
        arr[i].rounds = K
        arr[i].l_xy, arr[i].l_inf = lx + 64 * K * i, li + K * i
        arr[i].r_xy, arr[i].r_inf = rx + 64 * K * i, ri + K * i
    return arr


def prove_batch(e, ipa, a, arr, n):
    check(lib().vc_ipa_prove(e.h, ipa.table, N, P(a["data"]), P(a["com_xy"]), P(a["com_inf"]), P(a["points"]), n, None,
                             ctypes.cast(arr, ctypes.c_void_p)), "ipa_prove")


def collect_tips(arr, o, n):
    raw = np.frombuffer(arr, dtype=np.uint8).reshape(n, ctypes.sizeof(scheme._ProofBuf))
    off = scheme._ProofBuf.tip.offset
    o["tip"][:] = raw[:, off:off + 32].copy().view(np.uint64)
    o["y"][:] = raw[:, off + 32:off + 64].copy().view(np.uint64)


def timed(fn, reps):
    ts = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:
            ts.append(time.perf_counter() - t0)
    return {"ms": float(np.median(ts)) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def baseline_child(sizes, reps):
    """vc_ipa_prove with batch = n from the library this process loaded -> one JSON line"""
    e = vkzg.Engine("bn254", 0)
    ipa = setup(e)
    res = {}
    for n in sizes:
        a, o = make_inputs(e, ipa, n), outputs(n)
        arr = proof_structs(o, n)
        res[str(n)] = timed(lambda: prove_batch(e, ipa, a, arr, n), reps)
        collect_tips(arr, o, n)
        res[str(n)]["sha256"] = digest(o)
    e.close()
    print("BASELINE " + json.dumps(res), flush=True)


def laps_child(sizes):
    """one warm-up and one timed call per n and call, the library's lap lines on stderr"""
    e = vkzg.Engine("bn254", 0)
    ipa = setup(e)
    for n in sizes:
        a, o = make_inputs(e, ipa, n), outputs(n)
        arr = proof_structs(o, n)
        for _ in range(2):
            prove_many(e, ipa, a, o, n)
        for _ in range(2):
            prove_batch(e, ipa, a, arr, n)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "ipa_prove_many"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,256,4096,65536")
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--child", choices=("baseline", "laps"), default=None)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.child == "baseline":
        return baseline_child(sizes, a.reps)
    if a.child == "laps":
        return laps_child(sizes)
    e = vkzg.Engine("bn254", 0)
    ipa = setup(e)
    res = {"N": N, "curve": "bn254", "reps": a.reps,
           "baseline": "vc_ipa_prove, batch = n, " + ("the parent commit's build (--baseline-tree)" if a.baseline_tree
                                                        else "this build"),
           "sizes": {}}
    for n in sizes:
        inp, o = make_inputs(e, ipa, n), outputs(n)
        many = timed(lambda: prove_many(e, ipa, inp, o, n), a.reps)
        many["sha256"] = digest(o)
        res["sizes"][str(n)] = {"prove_many": many}
        print(f"n = {n:6d}: prove_many {many['ms']:.2f} ms [{many['min_ms']:.2f}, {many['max_ms']:.2f}]", flush=True)
    e.close()

    me = [sys.executable, os.path.abspath(__file__), "--sizes", a.sizes, "--reps", str(a.reps)]
    tree = ["--baseline-tree", a.baseline_tree] if a.baseline_tree else []
    child = subprocess.run(me + tree + ["--child", "baseline"], stdout=subprocess.PIPE, text=True, timeout=1100)
    assert child.returncode == 0, child.stdout[-2000:]
    base = json.loads([ln for ln in child.stdout.splitlines() if ln.startswith("BASELINE ")][-1][9:])
    for n in sizes:
        s = res["sizes"][str(n)]
        many, one = s["prove_many"], base[str(n)]
        s["prove_batch"] = one
        s["equal_outputs"] = many.pop("sha256") == one.pop("sha256")
        s["ratio_batch_over_many"] = one["ms"] / many["ms"]
        s["many_entirely_below_batch"] = many["max_ms"] < one["min_ms"]
        print(f"n = {n:6d}: prove_batch {one['ms']:.2f} ms [{one['min_ms']:.2f}, {one['max_ms']:.2f}], ratio "
              f"{s['ratio_batch_over_many']:.2f}, equal outputs {s['equal_outputs']}", flush=True)
        assert s["equal_outputs"], n

    # ---- stage laps from a child process (the library reads VKZG_HOST_TIMING once)
    child = subprocess.run(me + ["--child", "laps"], env=dict(os.environ, VKZG_HOST_TIMING="1"), stderr=subprocess.PIPE,
                           text=True, timeout=1100)
    assert child.returncode == 0, child.stderr[-2000:]
    pat = re.compile(r"\[ipa_prove_many\] n=(\d+) N=\d+ rows=\d+ chunks=(\d+): rows ([\d.]+) us, upload ([\d.]+) us, "
                     r"init ([\d.]+) us, rounds' field kernels ([\d.]+) us, commits ([\d.]+) us, copy-back ([\d.]+) us, "
                     r"call ([\d.]+) us")
    for m in pat.finditer(child.stderr):  # the second (warm) call of each n overwrites the first
        res["sizes"][m.group(1)]["prove_many"]["laps_us"] = {
            "chunks": int(m.group(2)), "rows_upload_and_conversion": float(m.group(3)), "chunk_inputs_upload": float(m.group(4)),
            "init": float(m.group(5)), "round_and_finish_kernels": float(m.group(6)), "commits": float(m.group(7)),
            "copy_back": float(m.group(8)), "call_with_syncs": float(m.group(9))}
    pat = re.compile(r"\[ipa_prove\] (\d+) proofs x \d+ rounds: rows ([\d.]+) us, L/R commits ([\d.]+) us, "
                     r"transcript \+ folds ([\d.]+) us")
    for m in pat.finditer(child.stderr):
        if m.group(1) in res["sizes"]:
            res["sizes"][m.group(1)]["prove_batch"]["laps_us"] = {
                "host_rows": float(m.group(2)), "commits": float(m.group(3)), "host_transcripts_and_folds": float(m.group(4))}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Multiproof batch verification: vc_multiproof_verify_many_ipa / _kzg at N = 256 (BN254) beside a loop
of the single calls (vc_multiproof_verify_ipa / vc_multiproof_verify_kzg) over the same proofs, all
through the bare C ABI.

Shapes: Q in {16, 64, 1024} queries per proof, P in {1, 256, 4096, 65536} proofs with P x Q capped at
2^20 (P is lowered to the cap). A shape's proofs are `distinct` (8) proofs made with
vc_multiproof_prove over seeded rows, repeated to P: the verifier does the same work for a repeated
proof. Times are host wall clock around the whole call (uploads and read-backs included): min,
median and max of `reps` calls after one warm-up. The loop runs in a child process, from this build
or, with --baseline-tree, from another checkout's verkle-kzg_amd directory (its vkzg package and its
built lib/: the parent commit's); every timed rep of the loop runs all P single calls (its warm-up
runs the first 32). Verdicts must be equal (all 1). The stage laps (VKZG_HOST_TIMING, the stream synchronised between
stages, so their sum exceeds the untimed call) come from a child process, one warm-up and one timed
call per shape.
usage: multiproof_verify_many_probe.py [--out DIR] [--reps N] [--qs 16,64,1024] [--ps 1,256,4096,65536]
                                       [--schemes ipa,kzg] [--baseline-tree DIR]
Writes DIR/probe.json (default: profiles/r21/multiproof_verify_many under the repository root)."""
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
PT = scheme._p
DISTINCT = 8
QUERY_KEYS = ("cxy", "cinf", "z", "y")
PROOF_KEYS = {"ipa": ("dxy", "dinf", "lxy", "linf", "rxy", "rinf", "tip", "iy"), "kzg": ("dxy", "dinf", "kxy", "kinf", "ky")}


def setup(e, name):
    return scheme.IPA(e, N, scheme.ipa_crs(N + 1, max_=512)) if name == "ipa" else scheme.KZG(e, N)


def make_distinct(e, vc, name, Q, seed):
    """DISTINCT proofs of Q queries over 16 seeded rows -> flat arrays [DISTINCT][...]"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 1 << 63, size=(16, N, 4), dtype=np.uint64)
    rows[:, :, 3] >>= np.uint64(3)  # below 2^252 < r
    rxy, rinf = e.msm_batch(vc.table, rows.reshape(-1, 4), N)
    out = {k: [] for k in QUERY_KEYS + PROOF_KEYS[name]}
    for _ in range(DISTINCT):
        pick = rng.integers(0, 16, size=Q)
        z = rng.integers(0, N, size=Q).astype(np.uint64)
        data = np.ascontiguousarray(rows[pick].reshape(-1, 4))
        cxy, cinf = np.ascontiguousarray(rxy[pick]), np.ascontiguousarray(rinf[pick])
        y = np.ascontiguousarray(rows[pick, z.astype(np.int64)])
        dxy = np.zeros(8, dtype=np.uint64)
        dinf = np.zeros(1, dtype=np.uint8)
        if name == "ipa":
            b, arrs = scheme.IPAProof._alloc(K)
            check(lib().vc_multiproof_prove(e.h, 0, vc.table, N, Q, PT(data), PT(cxy), PT(cinf), PT(z), PT(y), PT(dxy),
                                            PT(dinf), ctypes.byref(b), None, None, None), "multiproof_prove")
            inner = {"lxy": arrs["lxy"].copy(), "linf": arrs["linf"].copy(), "rxy": arrs["rxy"].copy(),
                     "rinf": arrs["rinf"].copy(), "tip": np.array(b.tip[:], dtype=np.uint64),
                     "iy": np.array(b.y[:], dtype=np.uint64)}
        else:
            kxy = np.zeros(8, dtype=np.uint64)
            kinf = np.zeros(1, dtype=np.uint8)
            ky = np.zeros(4, dtype=np.uint64)
            check(lib().vc_multiproof_prove(e.h, 1, vc.table, N, Q, PT(data), PT(cxy), PT(cinf), PT(z), PT(y), PT(dxy),
                                            PT(dinf), None, PT(kxy), PT(kinf), PT(ky)), "multiproof_prove")
            inner = {"kxy": kxy, "kinf": kinf[0], "ky": ky}
        inner.update(cxy=cxy, cinf=cinf, z=z, y=y, dxy=dxy, dinf=dinf[0])
        for k, v in inner.items():
            out[k].append(v)
    return {k: np.ascontiguousarray(np.stack(v)) for k, v in out.items()}


def repeat(d, P):
    """the DISTINCT proofs repeated to P: the [P][Q] layout (q_ptr == NULL) and the flat inner arrays"""
    idx = np.arange(P) % DISTINCT
    a = {k: np.ascontiguousarray(v[idx]) for k, v in d.items()}
    for k in ("lxy", "rxy"):
        if k in a:
            a[k] = np.ascontiguousarray(a[k].reshape(P * K, 8))
    for k in ("linf", "rinf"):
        if k in a:
            a[k] = np.ascontiguousarray(a[k].reshape(P * K))
    return a


def call_many(e, vc, name, a, P, Q):
    res = np.full(P, 0xAA, dtype=np.uint8)
    if name == "ipa":
        st = lib().vc_multiproof_verify_many_ipa(e.h, vc.table, N, P, None, Q, PT(a["cxy"]), PT(a["cinf"]), PT(a["z"]),
                                                 PT(a["y"]), PT(a["dxy"]), PT(a["dinf"]), PT(a["lxy"]), PT(a["linf"]),
                                                 PT(a["rxy"]), PT(a["rinf"]), PT(a["tip"]), PT(a["iy"]), PT(res))
    else:
        st = lib().vc_multiproof_verify_many_kzg(e.h, vc.verifying_key().h, N, P, None, Q, PT(a["cxy"]), PT(a["cinf"]),
                                                 PT(a["z"]), PT(a["y"]), PT(a["dxy"]), PT(a["dinf"]), PT(a["kxy"]),
                                                 PT(a["kinf"]), PT(a["ky"]), PT(res))
    check(st, "multiproof_verify_many")
    return res


def call_loop(e, vc, name, a, P, Q):
    """P single calls over the same arrays"""
    out = np.zeros(P, dtype=np.uint8)
    res = ctypes.c_int()
    L = lib()
    vk = vc.verifying_key().h if name == "kzg" else None
    for p in range(P):
        cxy, cinf, z, y, dxy = a["cxy"][p], a["cinf"][p], a["z"][p], a["y"][p], a["dxy"][p]
        if name == "ipa":
            lx, li, rx, ri = (a[k][p * K:(p + 1) * K] for k in ("lxy", "linf", "rxy", "rinf"))
            b = scheme._ProofBuf(K, lx.ctypes.data, li.ctypes.data, rx.ctypes.data, ri.ctypes.data)
            b.tip[:] = a["tip"][p].tolist()
            b.y[:] = a["iy"][p].tolist()
            check(L.vc_multiproof_verify_ipa(e.h, vc.table, N, Q, PT(cxy), PT(cinf), PT(z), PT(y), PT(dxy),
                                             int(a["dinf"][p]), ctypes.byref(b), ctypes.byref(res)), "verify_ipa")
        else:
            check(L.vc_multiproof_verify_kzg(e.h, vk, N, Q, PT(cxy), PT(cinf), PT(z), PT(y), PT(dxy), int(a["dinf"][p]),
                                             PT(a["kxy"][p]), int(a["kinf"][p]), PT(a["ky"][p]), ctypes.byref(res)),
                  "verify_kzg")
        out[p] = res.value
    return out


def timed(fn, reps, warm=None):
    (warm or fn)()  # warm-up
    ts, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"min_ms": ts[0], "median_ms": ts[len(ts) // 2], "max_ms": ts[-1]}, last


def child(mode, args):
    """baseline: the loop of single calls; laps: one timed new call under VKZG_HOST_TIMING"""
    d = dict(np.load(args.inputs))
    name, P, Q = args.scheme, args.P, args.Q
    e = vkzg.Engine("bn254")
    vc = setup(e, name)
    a = repeat(d, P)
    if mode == "baseline":
        t, res = timed(lambda: call_loop(e, vc, name, a, P, Q), args.reps, warm=lambda: call_loop(e, vc, name, a, min(P, 32), Q))
        t["verdicts_ok"] = bool((res == 1).all())
    else:
        call_many(e, vc, name, a, P, Q)
        sys.stderr.write("LAPS-BEGIN\n")
        sys.stderr.flush()
        res = call_many(e, vc, name, a, P, Q)
        t = {"verdicts_ok": bool((res == 1).all())}
    e.close()
    print("RESULT " + json.dumps(t))


def run_child(mode, args, inputs, name, P, Q, tree=None, env=None):
    cmd = [sys.executable, os.path.abspath(__file__), mode, "--inputs", inputs, "--scheme", name, "--P", str(P), "--Q", str(Q),
           "--reps", str(args.reps)]
    if tree:
        cmd += ["--baseline-tree", tree]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=1500)
    if p.returncode != 0:
        raise RuntimeError(f"{mode} child failed ({p.returncode}): {p.stderr[-2000:]}")
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    return out, p.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="probe", choices=["probe", "baseline", "laps"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "multiproof_verify_many"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--qs", default="16,64,1024")
    ap.add_argument("--ps", default="1,256,4096,65536")
    ap.add_argument("--schemes", default="ipa,kzg")
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--inputs")
    ap.add_argument("--scheme")
    ap.add_argument("--P", type=int)
    ap.add_argument("--Q", type=int)
    args = ap.parse_args()
    if args.mode != "probe":
        return child(args.mode, args)
    os.makedirs(args.out, exist_ok=True)
    e = vkzg.Engine("bn254")
    rows = []
    for name in args.schemes.split(","):
        vc = setup(e, name)
        for Q in [int(q) for q in args.qs.split(",")]:
            d = make_distinct(e, vc, name, Q, seed=21 + Q)
            with tempfile.TemporaryDirectory() as tmp:
                inputs = os.path.join(tmp, "inputs.npz")
                np.savez(inputs, **d)
                for P in sorted({min(int(p), (1 << 20) // Q) for p in args.ps.split(",")}):
                    a = repeat(d, P)
                    t_new, res = timed(lambda: call_many(e, vc, name, a, P, Q), args.reps)
                    assert (res == 1).all(), (name, P, Q, "the new call rejects a valid proof")
                    t_loop, _ = run_child("baseline", args, inputs, name, P, Q, tree=args.baseline_tree)
                    assert t_loop.pop("verdicts_ok"), (name, P, Q, "the single call rejects a valid proof")
                    env = dict(os.environ, VKZG_HOST_TIMING="1")
                    lp, err = run_child("laps", args, inputs, name, P, Q, env=env)
                    assert lp["verdicts_ok"]
                    laps = [ln for ln in err.split("LAPS-BEGIN")[-1].splitlines() if ln.startswith("[mp_verify_many]")]
                    row = {"scheme": name, "N": N, "Q": Q, "P": P, "new": t_new, "loop": t_loop, "loop_tree": args.baseline_tree or "this build",
                           "speedup_median": t_loop["median_ms"] / t_new["median_ms"],
                           "every_rep_below": t_new["max_ms"] < t_loop["min_ms"], "laps": laps[-1] if laps else None}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    e.close()
    with open(os.path.join(args.out, "probe.json"), "w") as f:
        json.dump({"reps": args.reps, "distinct_proofs": DISTINCT, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

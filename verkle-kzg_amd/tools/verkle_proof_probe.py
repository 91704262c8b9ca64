"""Verkle tree proofs at the bench's shape (bench.py verkle line: 65,536 random 32-unit keys,
KZG(256) on BN254): vc_verkle_prove and vc_verkle_verify for 1,000 and 10,000 keys -- medians of
`reps` calls after a warm-up, the prover's per-kernel times (vc_ctx_enable_timing), its host steps
alone (the walk: vc_verkle_proof_size; the transcript: vc_multiproof_begin), and the same query sets
through the dense route (vc_verkle_proof_queries' Q x 256 rows uploaded, then
vc_multiproof_begin_accumulate + vc_multiproof_finish) as the thing to compare against.
usage: verkle_proof_probe.py [--keys 65536] [--prove 1000,10000] [--reps 5] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vkzg  # noqa: E402
from vkzg import scheme  # noqa: E402
from vkzg._lib import check, lib  # noqa: E402
from vkzg.verkle import VerkleProof, VerkleTree  # noqa: E402

KERNELS = ("verkle_gather_nodes", "mp_rpow", "mp_sparse_chunk", "mp_sparse_reduce", "mp_chunk", "mp_chunk_reduce",
           "mp_sum_parts", "mp_quot", "mp_combine", "sparse_count", "sparse_expand", "sparse_rows", "sparse_count_scan",
           "sparse_expand_rows", "sparse_small", "sparse_accumulate", "msm_fixup_init", "msm_fixup_jump", "msm_fixup",
           "sparse_store", "sparse_combine", "sparse_add_base", "norm_prep", "norm_finish", "fb_normalize", "fb_commit",
           "fb_combine", "fb_commit_small", "to_data_item", "sparse_iota")
P = ctypes.c_void_p


def ptr(a):
    return a.ctypes.data_as(P)


def med_ms(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 16)
    ap.add_argument("--prove", default="1000,10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    e = vkzg.Engine("bn254", 0)
    stream = torch.cuda.current_stream()
    e.set_stream(stream.cuda_stream)
    kzg = scheme.KZG(e, 256)
    e.fixed_base_precompute(kzg.table, 16)
    rng = np.random.default_rng(91)  # the bench's tree
    keys = rng.integers(0, 256, size=(a.keys, 32), dtype=np.uint8)
    vals = rng.integers(0, 256, size=(a.keys, 32), dtype=np.uint8)
    t = VerkleTree(32)
    for i in range(a.keys):
        t.insert_single(keys[i].tobytes(), vals[i].tobytes())
    root = t.commitment(e, kzg.table)
    rxy, rinf = scheme._pt_arrays([root])
    vk = kzg.verifying_key()
    L = lib()
    out = {"tree_keys": a.keys, "scheme": "KZG(256) BN254", "reps": a.reps, "host_sha256_path": L.vc_host_sha256_path(),
           "stats": t.stats(), "runs": []}
    for n in (int(x) for x in a.prove.split(",")):
        # keys the tree finds with their last value (a level-skipping split can hide a key; a
        # repeated key holds its last value)
        last = {keys[i].tobytes(): vals[i].tobytes() for i in range(a.keys)}
        sel = []
        for i in range(a.keys):
            k = keys[i].tobytes()
            if len(sel) < n and t.get_single(k) == last[k]:
                sel.append(k)
        n = len(sel)
        kb = np.frombuffer(b"".join(sel), dtype=np.uint8).copy()
        vb = np.frombuffer(b"".join(last[k] for k in sel), dtype=np.uint8).copy()
        n_com, Q = t.proof_size(sel)
        buf, keep = VerkleProof._alloc(n, n_com, False)
        oxy = np.zeros(8, dtype=np.uint64)
        oinf = np.zeros(1, dtype=np.uint8)

        def prove():
            buf.n_com = n_com
            check(L.vc_verkle_prove(e.h, 1, kzg.table, t.h, ptr(kb), n, ptr(oxy), ptr(oinf), ctypes.byref(buf)), "prove")

        res = ctypes.c_int()

        def verify():
            check(L.vc_verkle_verify(e.h, 1, kzg.table, vk.h, 32, ptr(rxy), int(rinf[0]), ptr(kb), ptr(vb), n,
                                     ctypes.byref(buf), ctypes.byref(res)), "verify")
            assert res.value == 1

        run = {"keys": n, "queries": Q, "commitments": n_com}
        run["prove"] = med_ms(prove, a.reps)
        assert scheme._pt(oxy, oinf[0]) == root
        sparse_d = bytes(buf.d_xy), bytes(buf.kzg_proof_xy), bytes(buf.kzg_y)
        run["verify"] = med_ms(verify, a.reps)
        nc, nq = ctypes.c_size_t(), ctypes.c_size_t()
        run["host_walk"] = med_ms(lambda: L.vc_verkle_proof_size(t.h, ptr(kb), n, ctypes.byref(nc), ctypes.byref(nq)), a.reps)
        e.enable_timing(True)
        e.reset_timing()
        prove()
        e.enable_timing(False)
        run["prove_kernels_ms"] = {k: round(ms, 4) for k in KERNELS for ms, cnt in [e.kernel_time(k)] if cnt}
        run["prove_kernels_total_ms"] = round(sum(run["prove_kernels_ms"].values()), 3)
        # the dense route over the same queries
        cxy, cinf, z, y, rows = t.proof_queries(e, kzg.table, sel, rows=True)

        def transcript():
            tr, _, _ = scheme.multiproof_begin(256, cxy, cinf, z, y)
            L.vc_transcript_free(tr)

        run["host_transcript"] = med_ms(transcript, a.reps)
        nrows = scheme.multiproof_rows(256, z)
        S = torch.empty((nrows, 256, 4), dtype=torch.int64, device="cuda")
        pinned = torch.from_numpy(rows.view(np.int64)).pin_memory()
        dense = {}

        def upload():
            dense["d"] = pinned.cuda(non_blocking=True)
            torch.cuda.synchronize()

        def dense_prove():
            tr, _ = scheme.multiproof_begin_accumulate(e, 256, cxy, cinf, z, y, 0, Q, dense["d"].data_ptr(), S.data_ptr())
            dense["mp"] = scheme.multiproof_finish(kzg, z, S[None].data_ptr(), 1, tr)

        run["dense_rows_bytes"] = int(rows.nbytes)
        run["dense_upload_pinned"] = med_ms(upload, a.reps)
        run["dense_begin_accumulate_finish"] = med_ms(dense_prove, a.reps)
        mp = dense["mp"]
        dxy, _ = scheme._pt_arrays([mp["d"]])
        pxy, _ = scheme._pt_arrays([mp["proof"]["proof"]])
        assert (dxy.tobytes(), pxy.tobytes(), scheme._fr_raw(mp["proof"]["y"]).tobytes()) == sparse_d, "routes differ"
        run["same_proof_both_routes"] = True
        e.enable_timing(True)
        e.reset_timing()
        dense_prove()
        e.enable_timing(False)
        run["dense_kernels_ms"] = {k: round(ms, 4) for k in KERNELS for ms, cnt in [e.kernel_time(k)] if cnt}
        del dense["d"], pinned, rows
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    e.close()


if __name__ == "__main__":
    main()

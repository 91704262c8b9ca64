"""The geometry msm_slice_plan gives each slice the MSM paths enqueue (csrc/msm_plan.hpp, on the host;
tests/cpp/slice_plan_check.cpp): every field equal to the recorded rows of
tests/golden/msm_slice_plan.json (computed by the expressions slice_enqueue held before the plan was
a function of its own), the figures the source states for the 2^20 paths, and the relations the sort,
the accumulate and the tail rely on: the accumulate grid covers every entry, the segments and the
coarse bins tile the bucket set, and the sort's counters are one per (set, coarse bin, block) plus
the scan's terminal slot."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = ("nv", "c", "W", "wb", "we", "shared", "sets", "m", "top_f", "m_override")
PLAN = ("M", "Lseg", "S", "J", "nU", "Tmax", "NB", "NBtot", "FB", "chunk", "cstage", "NBC", "nblk", "ncnt", "guard")
NAMES = ["bn254_2e20", "band_2e20", "radix_2e20", "radix_2sets", "radix_8sets", "glv_perwin", "glv_slice8",
         "glv_slice2", "shared_pow2", "radix_range_2e17", "n1", "n1000", "n20000", "m_override1", "m_override2"]


def test_slice_plan_geometries(tmp_path):
    exe = tmp_path / "slice_plan_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(HERE, "cpp", "slice_plan_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True, timeout=60)
    rows = [json.loads(line) for line in out.splitlines()]
    with open(os.path.join(HERE, "golden", "msm_slice_plan.json")) as f:
        golden = json.load(f)
    assert [r["name"] for r in rows] == NAMES == [g["name"] for g in golden]
    for r, g in zip(rows, golden):
        assert set(r) == set(g) == {"name", *SHAPE, *PLAN}
        for k in SHAPE + PLAN:
            assert r[k] == g[k], (r["name"], k, r[k], g[k])
    p = {r["name"]: r for r in rows}
    # the one-GPU radix MSM at 2^20 (BLS12-381: 2^21 GLV halves, 7 windows of radix 5 x 2^16)
    r = p["radix_2e20"]
    assert (r["nv"], r["c"], r["m"], r["W"], r["shared"], r["sets"]) == (1 << 21, 16, 5, 7, 1, 1)
    assert (r["NB"], r["FB"], r["NBC"], r["chunk"], r["cstage"]) == (163840, 7, 1280, 4096, 1)
    assert (r["M"], r["Lseg"], r["S"], r["J"], r["nU"], r["Tmax"]) == (112, 5, 32768, 15, 5, 131072)
    assert (p["radix_2sets"]["sets"], p["radix_2sets"]["W"]) == (2, 14)
    assert (p["radix_8sets"]["sets"], p["radix_8sets"]["W"]) == (8, 56)
    # BN254 at 2^20: 16 windows of 16 bits, 64 entries per accumulate thread
    b = p["bn254_2e20"]
    assert (b["nv"], b["c"], b["W"], b["M"]) == (1 << 20, 16, 16, 64)
    assert (p["glv_slice8"]["W"], p["glv_slice2"]["W"], p["glv_perwin"]["W"]) == (1, 4, 8)
    assert (p["m_override1"]["M"], p["m_override2"]["M"]) == (1, 2)
    assert (p["n1"]["nv"], p["n1000"]["nv"], p["n20000"]["nv"], p["radix_range_2e17"]["nv"]) == (1, 1000, 20000, 1 << 17)
    for d in rows:
        Wr = d["sets"] if d["shared"] else d["W"]
        assert d["Tmax"] * d["M"] >= d["nv"] * d["W"], d["name"]
        assert d["S"] * d["Lseg"] == d["NB"], d["name"]
        assert d["S"] == 1 << d["J"], d["name"]
        assert d["NBC"] << d["FB"] == d["NB"], d["name"]
        assert d["ncnt"] == Wr * d["NBC"] * d["nblk"] + 1, d["name"]
        assert d["NBtot"] == Wr * d["NB"], d["name"]

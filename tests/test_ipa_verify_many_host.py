"""Batched IPA verification (vc_ipa_verify_many) without a GPU.

* the per-proof arithmetic of csrc/ipa_verify.hpp on the host (tests/cpp/ipa_verify_check.cpp, built
  with g++ and the address / undefined-behaviour sanitizers and run directly): for every N = 4 and
  N = 32 entry of tests/golden/ipa_verify_many.json the whole identity with the recorded challenges,
  the fixed part as N + 1 plain scalar multiplications over the CRS; every verdict equals the
  oracle's `valid`; the one-inversion barycentric dot product against per-element inverses.
* both kernels are in the cross-built gfx950 code object, within the register budget DESIGN.md 4.7
  records, without spills.
* the fixture is what its generator writes."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _h(v):
    return "%x" % int(v, 16)


def _pt(P):
    return "1 0 0" if P is None else "0 %s %s" % (_h(P[0]), _h(P[1]))


def _dump(path, entries, crs):
    """the flat text the C++ side reads (it has no JSON parser): hex tokens, points as `inf x y`"""
    lines = [str(len(crs))] + [_pt(P) for P in crs] + [str(len(entries))]
    for e in entries:
        K = len(e["l"])
        lines.append("%d %d %d" % (e["N"], K, int(e["valid"])))
        lines.append(_pt(e["commitment"]))
        lines += [_h(e["point"]), _h(e["tip"]), _h(e["y"]), _h(e["w"])]
        lines += [_h(x) for x in e["x"]]
        lines += [_pt(P) for P in e["l"]] + [_pt(P) for P in e["r"]]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_identity_on_the_host_matches_the_oracle(tmp_path):
    entries = [e for e in _load("ipa_verify_many.json")["entries"] if e["N"] in (4, 32)]
    assert len(entries) >= 30
    crs = _load("ipa_crs_bn254.json")["points"][:33]
    flat = tmp_path / "entries.txt"
    _dump(flat, entries, crs)
    exe = tmp_path / "ipa_verify_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "ipa_verify_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe), str(flat)], text=True, timeout=600)
    d = json.loads(out.splitlines()[-1])
    print(d)
    assert d["entries"] == len(entries)
    assert d["wrong"] == 0, d
    assert d["true"] == sum(e["valid"] for e in entries) >= 1
    assert d["false"] == sum(not e["valid"] for e in entries) >= 1
    assert d["bary_checks"] >= 20 and d["bary_bad"] == 0, d


def test_kernels_in_the_code_object_within_their_register_budget():
    """the field kernel within 128 VGPRs + AGPRs (four waves per SIMD), the curve
    kernel within 256 (two waves per SIMD), neither spilling"""
    sys.path.insert(0, os.path.join(ROOT, "verkle-kzg_amd", "tools"))
    import vkzg
    from kernel_regs import kernel_regs
    rows = {name: (v, a, s) for name, v, a, s in kernel_regs(vkzg.LIB_PATH, "k_ipa_verify_")}
    budget = {"k_ipa_verify_field": 128, "k_ipa_verify_curve": 256}
    for kern, limit in budget.items():
        hit = [r for name, r in rows.items() if kern in name]
        assert len(hit) == 1, (kern, sorted(rows))
        vgpr, agpr, spills = hit[0]
        print(kern, vgpr, agpr, spills)
        assert vgpr + agpr <= limit, (kern, vgpr, agpr)
        assert spills == 0, (kern, spills)


def test_fixture_is_what_the_generator_writes(tmp_path):
    """regenerated from the oracle (~15 s of its Python curve arithmetic): byte for byte the committed file"""
    out = tmp_path / "ipa_verify_many.json"
    subprocess.check_call([sys.executable, os.path.join(GOLDEN, "make_ipa_verify_golden.py"), str(out)], timeout=600)
    assert out.read_bytes() == open(os.path.join(GOLDEN, "ipa_verify_many.json"), "rb").read()

"""IPA batch verification (vc_ipa_verify_batch) without a GPU.

* the shared text of csrc/ipa_batch.hpp on the host (tests/cpp/ipa_batch_check.cpp, built with g++
  and the address / undefined-behaviour sanitizers and run directly): the challenges hashed from
  register words equal the fixture's recorded w / x for every fresh-transcript entry (N = 4, 32,
  256, the identity's encoding included), and the fold of batches holding tampered entries equals
  the oracle's S (tests/ipa_batch_cases.py) at N = 4 and N = 32 for three seeds;
* the library's host paths, vc_ipa_challenges_many(NULL, ..) and vc_ipa_batch_fold(NULL, ..), give
  the same, and vc_ipa_batch_challenge is the oracle's hash_to_field with the DST;
* the new kernels are in the cross-built gfx950 code object, within the register budget DESIGN.md
  4.10 records, without spills."""
import json
import os
import subprocess
import sys

import pytest

import ipa_batch_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _pt(P):
    return "1 0 0" if P is None else "0 %x %x" % P


def _batches():
    """(N, entries): tampered entries inside, so S is not the identity; one valid batch"""
    n4 = cases.fresh(4)
    return [(4, [n4[0], n4[1], n4[0], n4[1], n4[0]]), (32, cases.tampered_batch(9)), (32, cases.tampered_batch(2)),
            (32, cases.valid_batch(3))]


class _NoEngine:
    curve, h = "bn254", None


def _ipa(N):
    """an IPA over the fixture's CRS with no engine behind it: only the host paths can be called"""
    from vkzg import scheme
    ipa = scheme.IPA.__new__(scheme.IPA)
    pts = cases.crs()[:N + 1]
    ipa.engine, ipa.N, ipa.g, ipa.q, ipa.table = _NoEngine(), N, pts[:N], pts[N], 0
    return ipa


def _arrays(batch):
    from vkzg import scheme
    return ([e["commitment"] for e in batch], [e["point"] for e in batch],
            [scheme.IPAProof(list(e["l"]), list(e["r"]), e["tip"], e["y"]) for e in batch])


def test_shared_text_under_the_sanitizers(tmp_path):
    ents = [e for e in cases.entries() if e["prefix"] is None]
    assert {e["N"] for e in ents} == {4, 32, 256} and any(e["name"] == "tamper_l0_identity" for e in ents)
    index = {e["id"]: i for i, e in enumerate(ents)}
    crs = cases.crs()[:257]
    lines = [str(len(crs))] + [_pt(P) for P in crs] + [str(len(ents))]
    for e in ents:
        lines.append("%d %d %d" % (e["N"], len(e["l"]), int(e["valid"])))
        lines.append(_pt(e["commitment"]))
        lines += ["%x" % v for v in (e["point"], e["tip"], e["y"], e["w"])] + ["%x" % x for x in e["x"]]
        lines += [_pt(P) for P in e["l"]] + [_pt(P) for P in e["r"]]
    runs = [(N, b, cases.oracle_rho(s)) for s in cases.SEEDS for N, b in _batches()]
    lines.append(str(len(runs)))
    for N, batch, rho in runs:
        lines.append("%d %d %x" % (N, len(batch), rho))
        lines.append(" ".join(str(index[e["id"]]) for e in batch))
        lines.append(_pt(cases.oracle_fold(batch, rho)))
    flat = tmp_path / "batches.txt"
    flat.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "ipa_batch_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "ipa_batch_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe), str(flat)], text=True, timeout=600)
    d = json.loads(out.splitlines()[-1])
    print(d)
    assert d["entries"] == len(ents) >= 30
    assert d["challenges"] == sum(1 + len(e["x"]) for e in ents) and d["challenges_bad"] == 0, d
    assert d["identity_points"] >= 1
    assert d["batches"] == len(runs) == 12 and d["fold_bad"] == 0, d
    assert d["fold_nonzero"] == 9  # (the valid batch folds to the identity for every seed)


@pytest.mark.parametrize("N", [4, 32, 256])
def test_host_challenges_match_the_fixture(N):
    batch = cases.fresh(N)
    assert _ipa(N).challenges_many(*_arrays(batch), device=False) == [(e["w"], e["x"]) for e in batch]


def test_batch_challenge_is_hash_to_field_with_the_dst():
    from vkzg import scheme
    for seed in cases.SEEDS:
        assert scheme.ipa_batch_challenge(seed) == cases.oracle_rho(seed)
    assert cases.DST == b"vkzg-ipa-batch"


@pytest.mark.parametrize("seed", range(3))
def test_host_fold_matches_the_oracle(seed):
    rho = cases.oracle_rho(cases.SEEDS[seed])
    for N, batch in _batches():
        want = cases.oracle_fold(batch, rho)
        assert (want is None) == all(e["valid"] for e in batch)
        assert _ipa(N).batch_fold(*_arrays(batch), rho, device=False) == want


def test_host_fold_statuses():
    import vkzg
    from pyoracle.curves import BN254_R
    from pyoracle import protocol
    ipa, rho = _ipa(32), cases.oracle_rho(cases.SEEDS[0])
    good = cases.valid_pool()
    for bad in cases.malformed_variants(good[4]):
        assert ipa.batch_fold(*_arrays([good[0], bad, good[1]]), rho, device=False) is False
    assert ipa.batch_fold([], [], [], rho, device=False) is None  # n = 0: the empty sum
    com, pts, proofs = _arrays(good[:3])
    pts[1] = pow(protocol.group_gen(32), 3, BN254_R)
    with pytest.raises(vkzg.VCError) as err:
        ipa.batch_fold(com, pts, proofs, rho, device=False)
    assert err.value.status == -8
    wide = _ipa(32)
    wide.N = 512  # above the fold's bound
    with pytest.raises(vkzg.VCError) as err:
        wide.batch_fold([], [], [], rho, device=False)
    assert err.value.status == -1


def test_kernels_in_the_code_object_within_their_register_budget():
    """the transcript and field kernels within 256 VGPRs + AGPRs (two waves per
    SIMD), the table fill and the row sum within 128, none spilling"""
    sys.path.insert(0, os.path.join(ROOT, "verkle-kzg_amd", "tools"))
    import vkzg
    from kernel_regs import kernel_regs
    rows = {name: (v, a, s) for name, v, a, s in kernel_regs(vkzg.LIB_PATH, "k_ipa_batch_")}
    budget = {"k_ipa_batch_transcripts": 256, "k_ipa_batch_field": 256, "k_ipa_batch_prep": 128,
              "k_ipa_batch_rowsum": 128}
    for kern, limit in budget.items():
        hit = [r for name, r in rows.items() if kern in name]
        assert len(hit) == 1, (kern, sorted(rows))
        vgpr, agpr, spills = hit[0]
        print(kern, vgpr, agpr, spills)
        assert vgpr + agpr <= limit, (kern, vgpr, agpr)
        assert spills == 0, (kern, spills)

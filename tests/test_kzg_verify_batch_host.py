"""KZG batch verification (vc_kzg_batch_challenge, vc_kzg_batch_fold, vc_kzg_verify_batch) on the
host path (ctx == NULL): no GPU. Every expected value is the oracle's (tests/kzg_batch_cases.py:
the fold in pyoracle.curves.BN254 arithmetic, verdicts from protocol.KZG.verify_point, the
challenge from arkser.hash_to_field); comparisons are exact.

* the challenge, the fold, the verdict, cancelling errors, malformed entries through the C ABI;
* csrc/kzg_batch.hpp and the final pairing entry as a stand-alone program (tests/cpp/
  kzg_batch_check.cpp, built with g++ and the address / undefined-behaviour sanitizers, run directly);
* k_kzg_batch_prep in the cross-built gfx950 code object, without spills, within the register
  budget DESIGN.md 4.8 records."""
import json
import os
import subprocess
import sys

import pytest

import kzg_batch_cases as cases
from pyoracle import arkser
from pyoracle.curves import BN254_R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIZES = [1, 2, 18, 33]


@pytest.fixture(scope="module")
def vk():
    from vkzg import scheme
    f = cases.fixture()
    return scheme.KZGVerifyingKey(f["g2"], f["size"])


@pytest.fixture(scope="module")
def rhos():
    return [arkser.hash_to_field(s, b"vkzg-kzg-batch", BN254_R) for s in cases.SEEDS]


def test_challenge_is_hash_to_field_of_the_seed(rhos):
    from vkzg import scheme
    assert cases.SEEDS[0] == bytes(32)
    for seed, rho in zip(cases.SEEDS, rhos):
        assert scheme.kzg_batch_challenge(seed) == rho
    assert len(set(rhos)) == 3


@pytest.mark.parametrize("n", SIZES)
def test_fold_matches_the_oracle(vk, rhos, n):
    batch = cases.valid_batch(n)
    if n >= 18:
        names = {e["name"] for e in batch}
        assert {"identity_commitment", "constant", "point_equals_size", "open_17", "open_big"} <= names
    rho = rhos[1]
    want = cases.oracle_fold(batch, rho)
    assert cases.trapdoor_accepts(*want)
    assert vk.batch_fold(None, *cases.arrays(batch), rho) == want


def test_fold_of_the_identity_alone(vk, rhos):
    """C = identity, proof = identity, y = 0: both sums are the identity"""
    batch = [cases.valid_pool()[1]]
    assert cases.oracle_fold(batch, rhos[0]) == (None, None)
    assert vk.batch_fold(None, *cases.arrays(batch), rhos[0]) == (None, None)


@pytest.mark.parametrize("n", SIZES)
def test_verdict_is_all_of_the_oracles(vk, n):
    batch = cases.valid_batch(n)
    assert all(cases.oracle_verdict(e) for e in batch)
    for seed in cases.SEEDS[1:]:
        assert vk.verify_batch(None, *cases.arrays(batch), seed=seed) is True
    assert vk.verify_batch(None, *cases.arrays(batch)) is True      # a seed of the call's own
    tampered = cases.tampered_pool()
    assert len(tampered) >= 17
    picks = tampered if n == 18 else tampered[n % 5::5]
    for k, t in enumerate(picks):
        pos = (0, n // 2, n - 1)[k % 3]
        bad = list(batch)
        bad[pos] = t
        want = all(cases.oracle_verdict(e) for e in bad)
        assert want is False
        assert vk.verify_batch(None, *cases.arrays(bad), seed=cases.SEEDS[k % 3]) is want, (t["name"], pos)


@pytest.mark.parametrize("make", [cases.cancelling_y, cases.cancelling_proofs])
def test_cancelling_errors_are_rejected(vk, rhos, make):
    """two errors that cancel in an unweighted sum: what the weights are for"""
    batch, touched = make()
    good = cases.valid_batch(len(batch))
    for i, e in enumerate(batch):
        assert cases.oracle_verdict(e) is (i not in touched)
    assert cases.trapdoor_accepts(*cases.oracle_fold(batch, 1, unweighted=True))
    for seed, rho in zip(cases.SEEDS, rhos):
        want = cases.oracle_fold(batch, rho)
        assert not cases.trapdoor_accepts(*want)
        assert vk.batch_fold(None, *cases.arrays(batch), rho) == want
        assert vk.verify_batch(None, *cases.arrays(batch), seed=seed) is False
        assert vk.verify_batch(None, *cases.arrays(good), seed=seed) is True


def test_malformed_entries_reject_without_an_error(vk, rhos):
    good = cases.valid_batch(5)
    for name, e in cases.malformed_cases():
        assert cases.oracle_verdict(e) is False
        for pos in (0, 2, 4):
            bad = list(good)
            bad[pos] = e
            assert vk.verify_batch(None, *cases.arrays(bad), seed=cases.SEEDS[1]) is False, name
            assert vk.batch_fold(None, *cases.arrays(bad), rhos[1]) is None, name
        assert vk.verify_batch(None, *cases.arrays(good), seed=cases.SEEDS[1]) is True


def test_arguments(vk, rhos):
    from vkzg import scheme
    good = cases.valid_batch(3)
    assert vk.verify_batch(None, [], [], []) is True
    assert vk.batch_fold(None, [], [], [], rhos[0]) == (None, None)
    with pytest.raises(scheme.VCError) as err:
        vk.verify_batch(None, *cases.arrays(good), seed=cases.SEEDS[0], locate=True)    # results need a context
    assert err.value.status == -1
    with pytest.raises(scheme.VCError) as err:
        vk.batch_fold(None, *cases.arrays(good), BN254_R)                                  # rho >= r
    assert err.value.status == -1
    assert vk.batch_fold(None, *cases.arrays(good), BN254_R - 1) == cases.oracle_fold(good, BN254_R - 1)
    assert vk.batch_fold(None, *cases.arrays(good), 0) == cases.oracle_fold(good, 0)     # weights 1, 0, 0


def _h(v):
    return "%x" % v


def _pt(P):
    return "1 0 0" if P is None else "0 %s %s" % (_h(P[0]), _h(P[1]))


def _dump(path, f, batches):
    """the flat text the C++ side reads: hex tokens, points as `inf x y`; per batch
    `n malformed valid`, rho, the entries (C, point, proof, y), then the oracle's P1 and P2"""
    (x0, x1), (y0, y1) = f["g2"]
    lines = [str(f["size"]), _h(x0), _h(x1), _h(y0), _h(y1), str(len(batches))]
    for batch, rho, malformed, valid, fold in batches:
        lines.append("%d %d %d" % (len(batch), int(malformed), int(valid)))
        lines.append(_h(rho))
        for e in batch:
            lines += [_pt(e["commitment"]), _h(e["point"]), _pt(e["proof"]["proof"]), _h(e["proof"]["y"])]
        lines += [_pt(fold[0]), _pt(fold[1])]
    with open(path, "w") as out:
        out.write("\n".join(lines) + "\n")


def test_fold_and_pairing_entry_under_the_sanitizers(tmp_path, rhos):
    f = cases.fixture()
    batches = []
    for n, rho in ((1, rhos[0]), (2, rhos[1]), (18, rhos[2]), (33, rhos[1])):
        batch = cases.valid_batch(n)
        batches.append((batch, rho, False, True, cases.oracle_fold(batch, rho)))
    for k, t in enumerate(cases.tampered_pool()[::4]):
        batch = cases.valid_batch(7)
        batch[(0, 3, 6)[k % 3]] = t
        malformed = "off_curve" in t["name"] or "equals_r" in t["name"]
        batches.append((batch, rhos[k % 3], malformed, False, (None, None) if malformed else cases.oracle_fold(batch, rhos[k % 3])))
    for make in (cases.cancelling_y, cases.cancelling_proofs):
        batch, _ = make()
        batches.append((batch, rhos[2], False, False, cases.oracle_fold(batch, rhos[2])))
    for _, e in cases.malformed_cases():
        batch = cases.valid_batch(4)
        batch[2] = e
        batches.append((batch, rhos[0], True, False, (None, None)))
    assert sum(b[2] for b in batches) >= 5
    flat = tmp_path / "batches.txt"
    _dump(flat, f, batches)
    exe = tmp_path / "kzg_batch_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "kzg_batch_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe), str(flat)], text=True, timeout=600)
    d = json.loads(out.splitlines()[-1])
    print(d)
    assert d["batches"] == len(batches)
    assert d["wrong"] == 0, d
    assert d["accepted"] == sum(b[3] for b in batches) == 4
    assert d["malformed"] == sum(b[2] for b in batches)
    assert d["rejected"] == len(batches) - d["accepted"] - d["malformed"] >= 4
    assert d["pow_checks"] >= 60


def test_prep_kernel_in_the_code_object_within_its_register_budget():
    """k_kzg_batch_prep, one instantiation per curve. BN254 within 128 VGPRs +
    AGPRs (a 256-lane block at four waves per SIMD), BLS12-381 within 256 (two waves), no spills"""
    sys.path.insert(0, os.path.join(ROOT, "verkle-kzg_amd", "tools"))
    import vkzg
    from kernel_regs import kernel_regs
    for tag, budget in (("BN254Kzg", 128), ("BLS381Kzg", 256)):
        rows = [r for r in kernel_regs(vkzg.LIB_PATH, "k_kzg_batch_prep") if tag in r[0]]
        assert len(rows) == 1, rows
        name, vgpr, agpr, spills = rows[0]
        print(name, vgpr, agpr, spills)
        assert spills == 0, rows
        assert vgpr + agpr <= budget, rows

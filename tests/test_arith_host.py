"""The check library (csrc/arith_check.hip -> lib/libvkzg_check.so) on the CPU: it builds with a
gfx950 code object and loads, refuses a device evaluation without a GPU, and its HOST evaluator --
the host build of ff.hpp, ff29.hpp, ff30.hpp, ec.hpp, ec29.hpp and ec30.hpp -- passes every check of
tests/arith_cases.py on the full operand tables of groups (a) fields, (b) limb engines and (c) group
law. That validates the tables, the word layouts and the Python reference before
tests/test_gpu_arith.py runs the same tables through the device build. The last tests show that the
comparison can fail: one flipped result bit and a reference with a wrong R are both rejected."""
import subprocess

import numpy as np
import pytest

import arith_cases as ac


@pytest.fixture(scope="module")
def check_lib():
    ac.build_lib()
    return ac.lib()


def test_check_library_embeds_gfx950(check_lib):
    """the shared object carries a gfx950 code object (the device evaluator is really built)"""
    with open(ac.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    for name in ("vkc_fe", "vkc_limb", "vkc_point", "vkc_quad", "vkc_block_sum"):
        assert hasattr(check_lib, name)


def test_check_library_is_not_in_the_product(check_lib):
    """libvkzg.so exports no vkc_* symbol and no public header declares one"""
    import vkzg._lib as product
    out = subprocess.check_output(["nm", "-D", "--defined-only", product.LIB_PATH], text=True)
    assert "vkc_" not in out
    for h in product.HEADERS:
        with open(h) as f:
            assert "vkc_" not in f.read()


def test_device_evaluation_without_gpu_is_an_error(check_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    a, b = ac.fe_table("bn254_fq", "inv")
    with pytest.raises(ac.CheckLibError) as e:
        ac.run_fe("bn254_fq", "add", a, b, on_device=True)
    assert e.value.status == ac.VC_E_NO_DEVICE
    t = ac.point_tables("bn254")
    with pytest.raises(ac.CheckLibError) as e:
        ac.run_point("bn254", "ec", "add", t.cases["add"], t.base_words(), on_device=True)
    assert e.value.status == ac.VC_E_NO_DEVICE
    with pytest.raises(ac.CheckLibError) as e:
        ac.run_quad("bn254", list(ac.quad_wave("bn254", "partial20")), t.base_words())
    assert e.value.status == ac.VC_E_NO_DEVICE
    with pytest.raises(ac.CheckLibError) as e:
        ac.run_block_sum("bn254", 64, ac.block_patterns("bn254", 64)[:1], t.base_words())
    assert e.value.status == ac.VC_E_NO_DEVICE


def test_edge_sets_hold_what_they_promise():
    for field, (_, p, N) in ac.FE_FIELDS.items():
        e = ac.edge_values(p, N)
        R = 1 << (32 * N)
        assert 30 <= len(e) <= 50 and len(set(e)) == len(e) and all(0 <= v < p for v in e)
        for v in (0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, R % p, R * R % p, p - R % p):
            assert v in e
        for k in range(1, N):
            assert 1 << (32 * k) in e and (1 << (32 * k)) - 1 in e
        low = (1 << (32 * (N - 1))) - 1
        assert any(v & low == low and v + (1 << (32 * (N - 1))) >= p for v in e), field
        a, b = ac.fe_table(field, "binary")
        assert len(a) == len(e) ** 2 + 2000 and set(zip(a, b)) >= {(x, y) for x in e for y in e}
        assert len(ac.fe_table(field, "inv")[0]) == len(e) + 200


# ---------------------------------------------------------------- (a)
@pytest.mark.parametrize("field", list(ac.FE_FIELDS))
def test_host_fe(check_lib, field):
    for op in ac.FE_OPS:
        a, b = ac.fe_table(field, ac.fe_kind(op))
        ac.check_fe(field, op, a, b, ac.run_fe(field, op, a, b, on_device=False))


# ---------------------------------------------------------------- (b)
@pytest.mark.parametrize("name", list(ac.LIMB_SETS))
def test_host_limb(check_lib, name):
    for op in ac.limb_ops(name):
        rows = ac.limb_table(name, op)
        out = ac.run_limb(name, op, rows, on_device=False)
        ac.check_limb(name, op, rows, out, lambda o, r: ac.run_limb(name, o, r, on_device=False))


def test_limb_ops_outside_a_set_are_refused(check_lib):
    rows = ac.limb_table("bls12_381_fq", "mul")
    with pytest.raises(ac.CheckLibError) as e:  # two raw operands need L <= 9
        ac.run_limb("bls12_381_fq", "mul_raw2", rows, on_device=False)
    assert e.value.status == ac.VC_E_INVALID


# ---------------------------------------------------------------- (c)
@pytest.mark.parametrize("engine", list(ac.ENGINES))
@pytest.mark.parametrize("curve", list(ac.CURVE_IDS))
def test_host_point(check_lib, curve, engine):
    t = ac.point_tables(curve)
    bw = t.base_words()
    for op in ac.engine_ops(curve, engine):
        cases = t.cases[op]
        assert cases
        ac.check_point(curve, engine, op, cases, ac.run_point(curve, engine, op, cases, bw, on_device=False))


def test_point_tables_hold_the_case_classes():
    for curve in ac.CURVE_IDS:
        t = ac.point_tables(curve)
        I = t.c.identity()
        assert all(t.c.is_on_curve(b) for b in t.bases)
        add = {c["label"]: c for c in t.cases["add"]}
        assert set(add) >= set(t.EXCEPTIONAL) | {"random"}
        assert add["opposite"]["want"] == I and add["opposite_rescaled"]["want"] == I and add["both_identity"]["want"] == I
        assert add["same_words"]["want"] == t.c.double(t.value(add["same_words"]["p"]))
        assert add["same_rescaled"]["qlam"] and add["opposite_rescaled"]["plam"]
        madd = {c["label"]: c for c in t.cases["madd"]}
        assert madd["own_point_neg"]["want"] == I and madd["negation"]["want"] == I
        assert madd["own_point"]["want"] == madd["negation_neg"]["want"] != I
        assert max(len(c["p"]) for c in t.cases["add"]) > 24 and min(len(c["p"]) for c in t.cases["madd"]) <= 1
        if curve == "bandersnatch":
            assert {"identity_zz", "order2", "cancellation"} <= set(add)
            assert t.bases[t.order2] == (0, t.c.p - 1) and add["cancellation"]["want"] == (0, 1)
        assert ac.block_sum_want(curve, dict(ac.block_patterns(curve, 64))["same_point_everywhere"]) == \
            t.c.mul(t.bases[0], 64)
        for nt in (64, 256):
            want = {lbl: ac.block_sum_want(curve, lanes) for lbl, lanes in ac.block_patterns(curve, nt)}
            assert want["alternating_P_minus_P"] == I and want["all_identity"] == I
            assert want["pair_xor_16"] == want["pair_inside_quad"] == t.value([(5, 0), (7, 1)])


# ---------------------------------------------------------------- the comparison can fail
def test_checker_rejects_one_flipped_bit(check_lib):
    a, b = ac.fe_table("bls12_381_fq", "binary")
    out = ac.run_fe("bls12_381_fq", "mul", a, b, on_device=False)
    ac.check_fe("bls12_381_fq", "mul", a, b, out)
    bad = out.copy()
    bad[len(a) // 2, 7] ^= np.uint32(1 << 13)
    with pytest.raises(AssertionError):
        ac.check_fe("bls12_381_fq", "mul", a, b, bad)

    rows = ac.limb_table("bn254_fr", "mul")
    out = ac.run_limb("bn254_fr", "mul", rows, on_device=False)
    more = lambda o, r: ac.run_limb("bn254_fr", o, r, on_device=False)  # noqa: E731
    ac.check_limb("bn254_fr", "mul", rows, out, more)
    bad = out.copy()
    bad[3, 0] ^= np.uint32(1)
    with pytest.raises(AssertionError):
        ac.check_limb("bn254_fr", "mul", rows, bad, more)

    t = ac.point_tables("bn254")
    cases = t.cases["add"]
    out = ac.run_point("bn254", "fast", "add", cases, t.base_words(), on_device=False)
    ac.check_point("bn254", "fast", "add", cases, out)
    for word in (0, 9, 17, 31):  # X, Y, ZZ, ZZZ of the first (random) case
        bad = out.copy()
        bad[0, word] ^= np.uint32(1 << 5)
        with pytest.raises(AssertionError):
            ac.check_point("bn254", "fast", "add", cases, bad)
    bad = out.copy()
    bad[0, 32] ^= np.uint32(1)  # the identity flag
    with pytest.raises(AssertionError):
        ac.check_point("bn254", "fast", "add", cases, bad)


def test_checker_rejects_a_reference_with_a_wrong_R(check_lib):
    for field, op in (("bn254_fq", "mul"), ("bls12_381_fr", "to_mont"), ("band_fr", "from_mont"), ("bn254_fr", "inv_bin")):
        _, p, N = ac.FE_FIELDS[field]
        a, b = ac.fe_table(field, ac.fe_kind(op))
        out = ac.run_fe(field, op, a, b, on_device=False)
        ac.check_fe(field, op, a, b, out)
        with pytest.raises(AssertionError):
            ac.check_fe(field, op, a, b, out, R=1 << (32 * N - 1))
    t = ac.point_tables("bls12_381")
    cases = t.cases["store"]
    out = ac.run_point("bls12_381", "fast", "store", cases, t.base_words(), on_device=False)
    ac.check_point("bls12_381", "fast", "store", cases, out)
    with pytest.raises(AssertionError):  # ZZ^3 == ZZZ^2 holds only with the right Montgomery factor
        ac.check_point("bls12_381", "fast", "store", cases, out, R=1 << 383)

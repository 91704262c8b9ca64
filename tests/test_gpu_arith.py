"""Device arithmetic parity: the DEVICE build of ff.hpp, ff29.hpp, ff30.hpp, ec.hpp, ec29.hpp and
ec30.hpp, one operation per launch and one lane per case (lib/libvkzg_check.so,
csrc/arith_check.hip), on the operand tables of tests/arith_cases.py:
  (a) fields: exact equality with Python integers, and device == host word for word;
  (b) limb engines: congruence mod p and the bounds of limb_bounds.py, device == host word for word;
  (c) group law (ec.hpp and the Fast29 engines): the canonical affine point against the oracle's
      integer group law, device == host for the stored words;
  (d) add_quad (device only): every lane of every quad against the same reference and against
      add() of the same operands;
  (e) fb_block_sum_store<C, 256> and <C, 64> (device only): one block per pattern against the
      integer sum.
Integer code: there is no tolerance anywhere. tests/test_arith_host.py runs the same tables through
the host evaluator on the CPU."""
import numpy as np
import pytest

import arith_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def check_lib():
    ac.build_lib()
    return ac.lib()


def _same_words(dev, host, what):
    bad = np.argwhere(dev != host)
    assert bad.size == 0, f"{what}: device != host at case {bad[0][0]}, word {bad[0][1]}"


# ---------------------------------------------------------------- (a)
@pytest.mark.parametrize("op", ac.FE_OPS)
@pytest.mark.parametrize("field", list(ac.FE_FIELDS))
def test_fe(check_lib, field, op):
    a, b = ac.fe_table(field, ac.fe_kind(op))
    dev = ac.run_fe(field, op, a, b, on_device=True)
    ac.check_fe(field, op, a, b, dev)
    _same_words(dev, ac.run_fe(field, op, a, b, on_device=False), f"{field} {op}")


# ---------------------------------------------------------------- (b)
@pytest.mark.parametrize("name", list(ac.LIMB_SETS))
def test_limb(check_lib, name):
    for op in ac.limb_ops(name):
        rows = ac.limb_table(name, op)
        dev = ac.run_limb(name, op, rows, on_device=True)
        ac.check_limb(name, op, rows, dev, lambda o, r: ac.run_limb(name, o, r, on_device=True))
        _same_words(dev, ac.run_limb(name, op, rows, on_device=False), f"{name} {op}")


# ---------------------------------------------------------------- (c)
@pytest.mark.parametrize("engine", list(ac.ENGINES))
@pytest.mark.parametrize("curve", list(ac.CURVE_IDS))
def test_point(check_lib, curve, engine):
    t = ac.point_tables(curve)
    bw = t.base_words()
    for op in ac.engine_ops(curve, engine):
        cases = t.cases[op]
        dev = ac.run_point(curve, engine, op, cases, bw, on_device=True)
        ac.check_point(curve, engine, op, cases, dev)
        _same_words(dev, ac.run_point(curve, engine, op, cases, bw, on_device=False), f"{curve} {engine} {op}")


# ---------------------------------------------------------------- (d)
@pytest.mark.parametrize("wave", ac.QUAD_WAVES)
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_add_quad(check_lib, curve, wave):
    """one wave, one case per quad, the four lanes of a quad given identical operands; every lane
    writes its result: all four agree, equal the integer group law and equal add()"""
    t = ac.point_tables(curve)
    bw = t.base_words()
    cases = list(ac.quad_wave(curve, wave))
    assert len(cases) == (5 if wave == "partial20" else 16)
    out = ac.run_quad(curve, cases, bw)
    assert out.shape[0] == 4 * len(cases)
    for role in range(4):  # every lane of the quad against the integers
        lanes = out[role::4]
        ac.check_point(curve, "fast", f"add_quad role {role}", cases, lanes)
    full = ac.run_point(curve, "fast", "add", cases, bw, on_device=True)
    for i, cs in enumerate(cases):
        want = ac.acc_to_affine(curve, full[i])
        for role in range(4):
            assert ac.acc_to_affine(curve, out[4 * i + role]) == want, f"{curve} {wave} [{cs['label']}] role {role}"
            # the four lanes hold the same words, not only the same point
            assert np.array_equal(out[4 * i + role], out[4 * i]), f"{curve} {wave} quad {i} role {role}"


# ---------------------------------------------------------------- (e)
@pytest.mark.parametrize("nt", [256, 64])
@pytest.mark.parametrize("curve", list(ac.CURVE_IDS))
def test_block_sum(check_lib, curve, nt):
    t = ac.point_tables(curve)
    pats = ac.block_patterns(curve, nt)
    assert len(pats) <= 20
    out = ac.run_block_sum(curve, nt, pats, t.base_words())
    for (label, lanes), row in zip(pats, out):
        got = ac.acc_to_affine(curve, ac.block_sum_record(curve, row))
        assert got == ac.block_sum_want(curve, lanes), f"{curve} NT = {nt} [{label}]"

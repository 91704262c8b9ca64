"""KZG::verify_point with real pairings on the host, through the C ABI (include/vc_scheme.h:
vc_kzg_g2_from_secret, vc_kzg_vk_new, vc_kzg_verify, vc_bn254_pairing_check). Expected verdicts
are the oracle's (protocol.KZG.verify_point, the trapdoor identity), stored in
tests/golden/kzg_verify_16.json -- the reference's test_single_proof (kzg/mod.rs:278-297) plus
tampered copies. No GPU."""
import pytest

import bn254_g2
import kzg_verify_fixture


@pytest.fixture(scope="module")
def fx():
    return kzg_verify_fixture.load()


@pytest.fixture(scope="module")
def vk(fx):
    from vkzg import scheme
    return scheme.KZGVerifyingKey(fx["g2"], fx["size"])


def test_g2_from_secret_matches_fixture(fx):
    from vkzg import scheme
    assert scheme.kzg_g2_from_secret(fx["secret"]) == fx["g2"]
    assert scheme.kzg_g2_from_secret(1) == bn254_g2.H
    assert scheme.kzg_g2_from_secret(0) is None


def test_fixture_verdicts_are_the_oracles(fx):
    """the stored verdicts are what the oracle says today (the fixture is not stale)"""
    from pyoracle import protocol
    kzg = protocol.KZG(fx["size"], secret=fx["secret"])
    for e in fx["entries"]:
        assert kzg.verify_point(e["commitment"], e["point"], e["proof"]) == e["valid"], e["name"]


def test_every_fixture_entry_gets_the_oracles_verdict(fx, vk):
    names = [e["name"] for e in fx["entries"]]
    assert [f"open_{i}" for i in range(16)] + ["open_17", "open_big"] == names[:18]
    for e in fx["entries"]:
        assert vk.verify_point(e["commitment"], e["point"], e["proof"]) == e["valid"], e["name"]
        if e["name"].startswith("open_"):
            assert e["valid"]
        else:
            assert not e["valid"]
    for i in range(8, 16):   # test_single_proof: y == 0 beyond the data
        assert fx["entries"][i]["proof"]["y"] == 0
    assert fx["entries"][17]["point"].bit_length() == 250


def test_malformed_entries_give_zero_not_an_error(fx, vk):
    from pyoracle.curves import BN254_P, BN254_R
    e = fx["entries"][1]
    x, y = e["proof"]["proof"]
    assert vk.verify_point(e["commitment"], e["point"], e["proof"])
    assert not vk.verify_point(e["commitment"], e["point"], {"proof": (x + BN254_P, y), "y": e["proof"]["y"]})
    assert not vk.verify_point(e["commitment"], e["point"], {"proof": (x, y), "y": e["proof"]["y"] + BN254_R})
    assert not vk.verify_point(e["commitment"], e["point"] + BN254_R, e["proof"])
    cx, cy = e["commitment"]
    assert not vk.verify_point((cx, (cy + 1) % BN254_P), e["point"], e["proof"])


def test_identity_inputs(vk):
    """a constant polynomial: proof = identity, C = y G; and C = identity with y = 0"""
    from pyoracle.curves import BN254
    c = BN254.mul(BN254.g, 77)
    for point in (3, 12345678901234567890):
        assert vk.verify_point(c, point, {"proof": None, "y": 77})
        assert not vk.verify_point(c, point, {"proof": None, "y": 78})
        assert vk.verify_point(None, point, {"proof": None, "y": 0})
        assert not vk.verify_point(None, point, {"proof": None, "y": 1})


def test_verify_keeps_the_strict_less_of_the_reference(fx, vk):
    """point == size is the point 16 itself, not omega^16 = 1 (kzg/mod.rs:172): the opening at
    index 0 (omega^0 = 1) must not verify as point 16"""
    from pyoracle import protocol
    e = fx["entries"][0]
    kzg = protocol.KZG(fx["size"], secret=fx["secret"])
    assert kzg.verify_point(e["commitment"], fx["size"], e["proof"]) is False
    assert not vk.verify_point(e["commitment"], fx["size"], e["proof"])


def test_pairing_check():
    from pyoracle.curves import BN254, BN254_R
    from vkzg import scheme
    a = 0x1234567890abcdef1234567890abcdef % BN254_R
    G, H = BN254.g, bn254_g2.H
    aG, aH = BN254.mul(G, a), bn254_g2.mul(H, a)
    assert scheme.pairing_check([(aG, H), (BN254.neg(G), aH)])
    assert not scheme.pairing_check([(aG, H), (BN254.neg(G), bn254_g2.mul(H, a + 1))])
    assert not scheme.pairing_check([(G, H)])
    assert scheme.pairing_check([])
    assert scheme.pairing_check([(None, H)]) and scheme.pairing_check([(G, None)])
    assert scheme.pairing_check([(None, H), (aG, H), (BN254.neg(G), aH), (G, None)])
    with pytest.raises(scheme.VCError):
        scheme.pairing_check([(G, bn254_g2.outside_subgroup())])
    with pytest.raises(scheme.VCError):
        scheme.pairing_check([((1, 3), H)])


def test_vk_new_refuses_malformed_keys(fx):
    from pyoracle.curves import BN254_P
    from vkzg import scheme
    (x0, x1), (y0, y1) = fx["g2"]
    with pytest.raises(scheme.VCError):
        scheme.KZGVerifyingKey(((x0, x1), ((y0 + 1) % BN254_P, y1)), 16)       # off the twist
    off = bn254_g2.outside_subgroup()
    assert bn254_g2.on_twist(off)
    with pytest.raises(scheme.VCError):
        scheme.KZGVerifyingKey(off, 16)                                        # on it, outside the subgroup
    with pytest.raises(scheme.VCError):
        scheme.KZGVerifyingKey(None, 16)                                       # the identity
    with pytest.raises(scheme.VCError):
        scheme.KZGVerifyingKey(((x0 + BN254_P, x1), (y0, y1)), 16)             # a coordinate >= p
    with pytest.raises(scheme.VCError):
        scheme.KZGVerifyingKey(fx["g2"], 12)                                   # not a power of two

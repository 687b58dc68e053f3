"""The big-integer model of the key calls (tests/key_model.py) checked against itself and against the reference's bytes: the map
u = (1 + y) / (1 - y) is pinned to the oracle's curve25519_dh_CalculatePublicKey -- not to the code under test -- and the flags of
the shared case set have the structure the rule in include/curve25519_amd.h states."""
import hashlib

import numpy as np
import pytest

import key_model as model
from oracle_lib import Oracle
from vectors import ED_B, L, P, ed_enc, ed_mul, small_order_encodings


@pytest.fixture(scope="module")
def cases():
    keys, labels = model.case_set()
    return keys, labels, model.expected(keys)


def test_map_matches_the_reference_public_key():
    """for 64 seeds: a = clamp(SHA-512(seed)[:32]); the model's u of enc(a * B) is the oracle's X25519 public key of a"""
    rng = np.random.default_rng(0x25519)
    seeds = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    a = np.stack([np.frombuffer(model.clamp(hashlib.sha512(s.tobytes()).digest()), np.uint8) for s in seeds])
    want, clamped = Oracle().x25519_public(a)
    assert np.array_equal(clamped, a), "the scalars are already clamped"
    for i in range(len(seeds)):
        priv = seeds[i].tobytes() + bytes(32)
        assert model.private_to_x25519(priv) == a[i].tobytes()
        key = ed_enc(ed_mul(int.from_bytes(a[i].tobytes(), "little"), ED_B))
        xpk, ok = model.to_x25519(key)
        assert ok == 1 and xpk == want[i].tobytes(), i


def test_map_of_known_points():
    assert model.montgomery_u(ED_B[1]) == 9
    assert model.montgomery_u(1) == 0 and model.montgomery_u(P + 1) == 0
    assert model.montgomery_u(P - 1) == 0 and model.montgomery_u(0) == 1


def test_flag_structure(cases):
    keys, labels, (flags, xpk, ok) = cases
    assert not (flags[(flags & 1) == 0] & 12).any(), "bits 2 and 3 are clear where bit 0 is"
    assert np.array_equal(ok, ((flags & 13) == 9).astype(np.int32))
    assert not xpk[ok == 0].any() and xpk[ok == 1].any(axis=1).all()
    lab = np.array(labels)
    assert set(flags[lab == "honest"]) == {11} and set(flags[lab == "honest negated"]) == {11}
    assert set(flags[lab == "mixed order"]) == {3} and (lab == "mixed order").sum() == 7 * (lab == "honest").sum()
    assert not (flags[lab == "off the curve"] & 1).any() and (lab == "off the curve").sum() == 12
    for v in set(flags):
        assert int(v) in (0, 1, 2, 3, 5, 7, 9, 11, 13, 15), int(v)
    assert {3, 11, 0, 2} <= set(int(v) for v in flags)


def test_small_order_encodings():
    """all 14 are of small order; the neutral element's four encodings alone are also torsion-free; none converts"""
    encs = small_order_encodings()
    assert len(encs) == 14
    for e, k in encs:
        f = model.classify(e)
        assert f & model.DECODES and f & model.SMALL_ORDER, (e.hex(), k)
        assert bool(f & model.TORSION_FREE) == (k == 0), (e.hex(), k)
        assert model.to_x25519(e) == (bytes(32), 0)
    assert model.classify((1).to_bytes(32, "little")) == 15


def test_non_canonical_y():
    """y = p .. p + 18: 2, 7, 8, 11, 12, 13 and 17 do not decode, y = 1 is the neutral element, every other one decodes to a point
    outside the prime-order subgroup -- so no non-canonical encoding but the neutral element's carries the torsion-free bit"""
    for k in range(19):
        for s in (0, 1):
            f = model.classify(((P + k) | (s << 255)).to_bytes(32, "little"))
            assert not f & model.CANONICAL
            if k in (2, 7, 8, 11, 12, 13, 17):
                assert f == 0, k
            elif k == 1:
                assert f == model.DECODES | model.SMALL_ORDER | model.TORSION_FREE
            else:
                assert f & model.DECODES and not f & model.TORSION_FREE, k


def test_walk_point_is_a_torsion_point(cases):
    keys, labels, (flags, _, _) = cases
    for i in np.flatnonzero(flags & 1):
        T = model.times_L(keys[i].tobytes())
        assert ed_mul(8, T) == model.NEUTRAL
        assert (T == model.NEUTRAL) == bool(flags[i] & model.TORSION_FREE)
    assert L % 8 == 5                            # [L] is a bijection of the 8-torsion: a mixed-order key never walks to O

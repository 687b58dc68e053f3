"""The big-integer model of the ristretto255 calls (tests/ristretto_model.py) pinned to RFC 9496's published vectors -- not to the
code under test -- and checked against itself, and the coverage of the case set the host-emulation and GPU tests share."""
import collections
import hashlib

import numpy as np
import pytest

import group_model
import ristretto_model as model
from vectors import ED_B, L, P, ed_add, ed_mul

GENERATOR_MULTIPLES = (
    "0000000000000000000000000000000000000000000000000000000000000000",
    "e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76",
    "6a493210f7499cd17fecb510ae0cea23a110e8d5b901f8acadd3095c73a3b919",
    "94741f5d5d52755ece4f23f044ee27d5d1ea1e2bd196b462166b16152a9d0259",
    "da80862773358b466ffadfe0b3293ab3d9fd53c5ea6c955358f568322daf6a57",
)


def test_constants_are_the_rfcs():
    assert model.INVSQRT_A_MINUS_D == 54469307008909316920995813868745141605393597292927456921205312896311721017578
    assert model.SQRT_AD_MINUS_ONE == 25063068953384623474111414158702152701244531502492656460079210482610430750235
    assert model.ONE_MINUS_D_SQ == 1159843021668779879193775521855586647937357759715417654439879720876111806838
    assert model.D_MINUS_ONE_SQ == 40440834346308536858101042469323190826248399146238708352240133220865137265952
    assert model.SQRT_AD_MINUS_ONE & 1, "the odd root: the even one maps a hash to the negated point"


def test_generator_multiples():
    for k, want in enumerate(GENERATOR_MULTIPLES):
        assert model.encode(ed_mul(k, ED_B)).hex() == want, k
        assert model.scalarmult_base(k.to_bytes(32, "little")).hex() == want, k
        assert model.scalarmult(k.to_bytes(32, "little"), bytes.fromhex(GENERATOR_MULTIPLES[1])) == (bytes.fromhex(want), 1)
    assert model.BASE.hex() == GENERATOR_MULTIPLES[1]


def test_other_fixed_outputs():
    assert model.encode(group_model.mul(L, ED_B)) == model.ZERO32
    assert model.scalarmult_base(L.to_bytes(32, "little")) == model.ZERO32
    assert model.from_hash(bytes(64)) == model.ZERO32
    assert model.decode(model.ZERO32) == (0, 1), "the identity decodes"


def test_the_rfc_hash_vector():
    h = hashlib.sha512(b"Ristretto is traditionally a short shot of espresso coffee").digest()
    assert model.from_hash(h).hex() == "3066f82a1a747d45120d1740f14358531a8f04bbffe6a819f86dfe50f44a0a46"


def test_rejected_encodings():
    want = ["non-canonical", "non-canonical", "non-canonical", "negative s", "y = 0"]
    assert [model.decode_why(b) for b, _ in model.FIXED_REJECTS] == [(None, w) for w in want]
    assert [w for _, w in model.FIXED_REJECTS] == want
    assert model.FIXED_REJECTS[0][0].hex() == "00" + "ff" * 31
    assert model.FIXED_REJECTS[1][0].hex() == "f3" + "ff" * 30 + "7f" and model.FIXED_REJECTS[2][0].hex() == "ed" + "ff" * 30 + "7f"
    assert model.FIXED_REJECTS[3][0].hex() == "01" + "00" * 31
    assert int.from_bytes(model.FIXED_REJECTS[4][0], "little") == P - 1
    for b, _ in model.FIXED_REJECTS:
        assert model.is_valid_point(b) == 0 and model.scalarmult((1).to_bytes(32, "little"), b) == (model.ZERO32, 0)


def _valid_points():
    pts, labels = model.points()
    return [p.tobytes() for p, l in zip(pts, labels) if l == "valid"]


def test_the_four_points_of_a_coset_encode_alike():
    i = model.SQRT_M1
    e4 = [(0, 1), (0, P - 1), (i, 0), (P - i, 0)]
    for T in e4:
        assert group_model.mul(4, T) == (0, 1)
    for b in _valid_points()[:24]:
        A = model.decode(b)
        assert {model.encode(ed_add(A, T)) for T in e4} == {b}


def test_decode_encode_round_trip():
    for b in _valid_points():
        A = model.decode(b)
        assert (-A[0] * A[0] + A[1] * A[1] - 1 - model.D * A[0] * A[0] * A[1] * A[1]) % P == 0, "on the curve"
        assert model.encode(A) == b
    for h in model.hashes():
        b = model.from_hash(h.tobytes())
        assert model.is_valid_point(b) == 1 and model.encode(model.decode(b)) == b


def test_scalarmult_agrees_with_the_affine_walk():
    """the model's [e]P against tests/vectors.py's affine double-and-add on the decoded point (50-80 ms a walk: a few rows)"""
    sc, pt, labels = model.case_set()
    rows = [i for i, l in enumerate(labels) if l == "valid"][::9] + [labels.index("base point")]
    for i in rows:
        A = model.decode(pt[i].tobytes())
        e = model.scalar_value(sc[i].tobytes())
        assert group_model.mul(e, A) == ed_mul(e, A)
        assert model.scalarmult(sc[i].tobytes(), pt[i].tobytes()) == (model.encode(ed_mul(e, A)), 1)


def test_add_and_sub_are_the_groups():
    a, b = (5).to_bytes(32, "little"), (L - 3).to_bytes(32, "little")
    pa, pb = model.scalarmult_base(a), model.scalarmult_base(b)
    assert model.point_add(pa, pb, False) == (model.scalarmult_base((2).to_bytes(32, "little")), 1)
    assert model.point_add(pa, pb, True) == (model.scalarmult_base((8).to_bytes(32, "little")), 1)
    assert model.point_add(pa, pa, True) == (model.ZERO32, 1)
    assert model.point_add(pa, model.FIXED_REJECTS[3][0], False) == (model.ZERO32, 0)


def test_case_set_covers_every_class_sixteen_times():
    pts, labels = model.points()
    count = collections.Counter(labels)
    for cls in ("valid", "not square", "negative t"):
        assert count[cls] >= 16, count
    have = {p.tobytes() for p in pts}
    assert all(b in have for b, _ in model.FIXED_REJECTS)
    assert [model.decode_why(p.tobytes())[1] for p in pts] == labels
    sc, pt, lab = model.case_set()
    assert 200 <= len(sc) <= 300
    for cls in ("valid", "not square", "negative t", "non-canonical", "negative s", "y = 0"):
        assert lab.count(cls) >= 16, cls
    for b, _ in model.FIXED_REJECTS:
        assert any(p.tobytes() == b for p in pt), b.hex()
    for s in group_model.edge_scalars():
        assert sum(1 for row in sc if row.tobytes() == s) >= 10
    squares = collections.Counter(x for h in model.hashes() for x in model.hash_squares(h.tobytes()))
    assert squares[True] >= 16 and squares[False] >= 16, squares
    rotates = collections.Counter()
    for s, p, l in zip(sc, pt, lab):
        A = model.decode(p.tobytes())
        if A is not None:
            rotates[model.encode_rotates(group_model.mul(model.scalar_value(s.tobytes()), A))] += 1
    assert rotates[True] >= 16 and rotates[False] >= 16, rotates
    hrot = collections.Counter(model.from_hash_rotates(h.tobytes()) for h in model.hashes())
    assert hrot[True] >= 16 and hrot[False] >= 16, hrot

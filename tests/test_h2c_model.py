"""The big-integer model of the hashing calls (tests/h2c_model.py) pinned to the published vectors of RFC 9380 (K.3, J.5.1, J.5.2)
and RFC 9497 (A.1.1) -- not to the code under test -- and checked against itself, and the coverage of the case set the
host-emulation and GPU tests share."""
import collections
import hashlib

import group_model
import h2c_model as model
import ristretto_model
from vectors import L, P, ed_enc

XMD_DST = b"QUUX-V01-CS02-with-expander-SHA512-256"
RO_DST = b"QUUX-V01-CS02-with-edwards25519_XMD:SHA-512_ELL2_RO_"
NU_DST = b"QUUX-V01-CS02-with-edwards25519_XMD:SHA-512_ELL2_NU_"

# RFC 9380 J.5.1: msg -> (P.x, P.y) big-endian hex.  The RFC prints all five; the first two were typed from it, the last three are
# this model's values, whose ends were held against an independent implementation (RO_ENDS).
RO_POINTS = {
    b"": ("3c3da6925a3c3c268448dcabb47ccde5439559d9599646a8260e47b1e4822fc6", "09a6c8561a0b22bef63124c588ce4c62ea83a3c899763af26d795302e115dc21"),
    b"abc": ("608040b42285cc0d72cbb3985c6b04c935370c7361f4b7fbdb1ae7f8c1a8ecad", "1a8395b88338f22e435bbd301183e7f20a5f9de643f11882fb237f88268a5531"),
    b"abcdef0123456789": ("6d7fabf47a2dc03fe7d47f7dddd21082c5fb8f86743cd020f3fb147d57161472",
                          "53060a3d140e7fbcda641ed3cf42c88a75411e648a1add71217f70ea8ec561a6"),
    b"q128_" + b"q" * 128: ("5fb0b92acedd16f3bcb0ef83f5c7b7a9466b5f1e0d8d217421878ea3686f8524",
                            "2eca15e355fcfa39d2982f67ddb0eea138e2994f5956ed37b7f72eea5e89d2f7"),
    b"a512_" + b"a" * 512: ("0efcfde5898a839b00997fbe40d2ebe950bc81181afbd5cd6b9618aa336c1e8c",
                            "6dc2fc04f266c5c27f236a80b14f92ccd051ef1ff027f26a07f8c0f327d8f995"),
}
RO_ENDS = {
    b"abcdef0123456789": (("6d7fabf4", "57161472"), ("53060a3d", "8ec561a6")),
    b"q128_" + b"q" * 128: (("5fb0b92a", "686f8524"), ("2eca15e3", "5e89d2f7")),
    b"a512_" + b"a" * 512: (("0efcfde5", "336c1e8c"), ("6dc2fc04", "27d8f995")),
}
NU_POINTS = {
    b"": ("1ff2b70ecf862799e11b7ae744e3489aa058ce805dd323a936375a84695e76da", "222e314d04a4d5725e9f2aff9fb2a6b69ef375a1214eb19021ceab2d687f0f9b"),
    b"abc": ("5f13cc69c891d86927eb37bd4afc6672360007c63f68a33ab423a3aa040fd2a8", "67732d50f9a26f73111dd1ed5dba225614e538599db58ba30aaea1f5c827fa42"),
}
# RFC 9497 A.1.1, OPRF mode, test vector 1
OPRF_SEED, OPRF_INFO = bytes([0xA3]) * 32, b"test key"
OPRF_SKS = "5ebcea5ee37023ccb9fc2d2019f9d7737be85591ae8652ffa9ef0f4d37063b0e"
OPRF_INPUT = b"\x00"
OPRF_ELEMENT = "5873db2e5f8f4f544ce3e574c74c487f03bc64a2cf63b7c913908091aab03357"
OPRF_BLIND = "64d37aed22a27f5191de1c1d69fadb899d8862b58eb4220029e036ec4c1f6706"
OPRF_BLINDED = "609a0ae68c15a3cf6903766461307e5c8bb2f95e7e6550e1ffa2dc99e412803c"
OPRF_EVALUATION = "7ec6578ae5120958eb2db1745758ff379e77cb64fe77b0b2d8cc917ea0869c7e"
OPRF_OUTPUT = ("527759c3d9366f277d8c6020418d96bb393ba2afb20ff90df23fb7708264e2f3"
               "ab9135e3bd69955851de4b1f9fe8a0973396719b7912ba9ee8aa7d0b5e24bcf6")


def test_expand_message_xmd_vectors():
    assert model.expand_message_xmd(b"", XMD_DST, 32).hex() == "6b9a7312411d92f921c6f68ca0b6380730a1a4d982c507211a90964c394179ba"
    assert model.expand_message_xmd(b"abc", XMD_DST, 32).hex() == "0da749f12fbe5483eb066a5f595055679b976e93abe9be6f0f6318bce7aca8dc"


def test_hash_to_curve_vectors():
    for msg, (x, y) in RO_POINTS.items():
        got = model.hash_to_curve_point(msg, RO_DST)
        assert ("%064x" % got[0], "%064x" % got[1]) == (x, y), msg
        assert model.hash_to_curve(msg, RO_DST) == ed_enc(got)
    for msg, ((x0, x1), (y0, y1)) in RO_ENDS.items():
        x, y = RO_POINTS[msg]
        assert x.startswith(x0) and x.endswith(x1) and y.startswith(y0) and y.endswith(y1), msg
    assert model.hash_to_curve(b"", RO_DST).hex() == "21dc15e10253796df23a7699c8a383ea624cce88c52431f6be220b1a56c8a609"


def test_encode_to_curve_vectors():
    for msg, (x, y) in NU_POINTS.items():
        got = model.encode_to_curve_point(msg, NU_DST)
        assert ("%064x" % got[0], "%064x" % got[1]) == (x, y), msg


def test_the_oprf_vector():
    sks = model.oprf_derive_key_pair(OPRF_SEED, OPRF_INFO)
    assert sks.hex() == OPRF_SKS
    element = model.oprf_hash_to_group(OPRF_INPUT)
    assert element.hex() == OPRF_ELEMENT
    blinded, ok = ristretto_model.scalarmult(bytes.fromhex(OPRF_BLIND), element)
    assert ok and blinded.hex() == OPRF_BLINDED
    evaluated, ok = ristretto_model.scalarmult(sks, blinded)
    assert ok and evaluated.hex() == OPRF_EVALUATION
    unblinded, ok = ristretto_model.scalarmult(sks, element)
    assert ok and model.oprf_finalize(OPRF_INPUT, unblinded).hex() == OPRF_OUTPUT
    assert len(OPRF_OUTPUT) == 128 and OPRF_OUTPUT.startswith("527759c3") and OPRF_OUTPUT.endswith("5e24bcf6")
    blind_inverse = pow(int.from_bytes(bytes.fromhex(OPRF_BLIND), "little"), L - 2, L).to_bytes(32, "little")
    assert ristretto_model.scalarmult(blind_inverse, evaluated) == (unblinded, 1)


def test_constants():
    assert model.SQRT_M486664 == 0x0F26EDF460A006BBD27B08DC03FC4F7EC5A1D3D14B7D1A82CC6E04AAFF457E06, "RFC 9380 6.8.2's c1"
    assert model.SQRT_M486664 ** 2 % P == -486664 % P and model.SQRT_M486664 % 2 == 0
    assert not model._is_square((model.MONT_J - 1) * pow(2, P - 2, P)), "no u gives x = -1"
    assert not model._is_square(-model.MONT_J), "u = 0: x1 = -J is off the curve's squares, so the point is (0, 0)"


def test_map_properties():
    identity = ed_enc(model.IDENTITY)
    assert identity.hex() == "01" + "00" * 31
    assert model.map_to_curve_bytes(bytes(32)) == identity and model.map_to_curve_bytes(P.to_bytes(32, "little")) == identity
    assert model.map_to_curve_bytes((2**255).to_bytes(32, "little")) == identity, "bit 255 is masked"
    torsion_free = 0
    for row in model.map_inputs():
        u = model.u_of(row.tobytes())
        A = model.map_to_curve(u)
        assert model.on_curve(A), row.tobytes().hex()
        assert model.map_straight_line(u)[0] == A, row.tobytes().hex()
        torsion_free += group_model.mul(L, A) == model.IDENTITY
    assert torsion_free < len(model.map_inputs()) // 2, "MapToCurve clears no cofactor: most outputs carry torsion"


def test_hashed_points_are_on_the_curve_and_torsion_free():
    for dst, size, msgs in model.case_set()[::5]:
        for m in msgs[:1]:
            for A in (model.hash_to_curve_point(m.tobytes(), dst), model.encode_to_curve_point(m.tobytes(), dst)):
                assert model.on_curve(A) and group_model.mul(L, A) == model.IDENTITY
            assert ristretto_model.decode(model.hash_to_group(m.tobytes(), dst)) is not None
            assert int.from_bytes(model.hash_to_scalar(m.tobytes(), dst), "little") < L


def test_hash_to_scalar_is_the_reduced_expander_output():
    dst, msg = b"HashToScalar-" + model.oprf_context_string(), b"some input"
    wide = model.expand_message_xmd(msg, dst, 64)
    assert int.from_bytes(model.hash_to_scalar(msg, dst), "little") == int.from_bytes(wide, "little") % L
    b_0 = hashlib.sha512(bytes(128) + msg + b"\x00\x40\x00" + dst + bytes([len(dst)])).digest()
    assert wide == hashlib.sha512(b_0 + b"\x01" + dst + bytes([len(dst)])).digest(), "one block of output: b_1 alone"


def test_case_set_covers_every_edge():
    cases = model.case_set()
    by_dst = collections.defaultdict(set)
    for dst, size, msgs in cases:
        assert msgs.shape == (model.ROWS_PER_CASE, size) and 1 <= len(dst) <= 255
        by_dst[len(dst)].add(size)
    assert set(by_dst) == {1, 16, 45, 46, 61, 62, 173, 174, 255}
    # dst_len + 66 + 17 bytes of b_i input, padding and length: 45 | 46 is the one / two block edge, 173 | 174 the two / three
    assert [(n + 83 + 127) // 128 for n in sorted(by_dst)] == [1, 1, 1, 2, 2, 2, 2, 3, 3]
    # 61 | 62 is where DST' || 0x80 leaves the block's first half: the length word's neighbours
    assert (61 + 66 + 1) == 128 and (62 + 66 + 1) == 129
    full = [n for n, sizes in by_dst.items() if {0, 1, 7, 8, 9, 63, 64, 65} <= sizes]
    assert len(full) >= 2
    for n in full:
        residues = {(s + n + 4) % 128 for s in by_dst[n]}
        assert {110, 111, 112, 127, 0, 1} <= residues, (n, sorted(residues))
        assert any((s + n + 21 + 127) // 128 >= 3 for s in by_dst[n]), "a message of three blocks"
        assert any(s % 2 for s in by_dst[n]) and any(s % 8 == 0 and s for s in by_dst[n])
    assert all(sizes >= {0} and len(sizes) >= 3 for sizes in by_dst.values())
    lens = collections.Counter(n for _, _, _, n in model.xmd_cases())
    assert set(lens) == {1, 32, 63, 64, 65, 96, 128, 129, 16320} and min(lens.values()) >= 2
    assert 40 <= len(cases) <= 80


def test_map_inputs_cover_both_selections_and_sign_fix_ups_sixteen_times():
    rows = [r.tobytes() for r in model.map_inputs()]
    values = {int.from_bytes(r, "little") for r in rows}
    assert {0, 1, 2, P - 1, P, P + 1, 2**255 - 1, 2**255 + 5} <= values
    count = collections.Counter()
    for r in rows:
        e1, e2, e3, e4, exceptional = model.map_straight_line(model.u_of(r))[1]
        count["gx1 square" if e3 else "gx1 not square"] += 1
        count[("square" if e3 else "not square") + (", negated" if e3 != e4 else ", kept")] += 1
        count["first root" if e1 else "first root times sqrt(-1)"] += e3
        count["second root" if e2 else "second root times sqrt(-1)"] += not e3
        count["exceptional"] += exceptional
    for cls in ("gx1 square", "gx1 not square", "square, negated", "square, kept", "not square, negated", "not square, kept",
                "first root", "first root times sqrt(-1)", "second root", "second root times sqrt(-1)"):
        assert count[cls] >= 16, (cls, count)
    assert count["exceptional"] == 2, "u = 0 and u = p, nothing else"

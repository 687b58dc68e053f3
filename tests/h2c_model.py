"""Hashing to edwards25519 and ristretto255 (RFC 9380, RFC 9497) in Python big integers and hashlib, written in the RFCs' order:
expand_message_xmd over SHA-512 (RFC 9380 section 5.3.1), hash_to_field (5.2), the Elligator 2 map in its generic form (6.7.1) with
the rational map to the Edwards curve (6.8.2), the two edwards25519 suites (8.5), hash_to_ristretto255 (appendix B) and RFC 9497's
HashToGroup / HashToScalar for ristretto255-SHA512 (section 4.1) -- and the rules of the c25519_ExpandMessageXmd_*, ed25519_MapToCurve_*,
ed25519_HashToCurve_*, ed25519_EncodeToCurve_*, ristretto255_HashToGroup_* and ed25519_HashToScalar_* calls (include/curve25519_amd.h,
"Hashing to the groups") on top of them.  tests/test_h2c_model.py pins the model to the RFCs' published vectors; the host-emulation and
GPU tests compare the lane code with it byte for byte on the case set below.  map_straight_line is appendix G.2.1 / G.2.2's
branch-free form, kept beside the generic one to label the cases (which selection, which sign fix-up); nothing here reads the device
code or its constants."""
import functools
import hashlib

import numpy as np

import group_model
import ristretto_model
from vectors import D_ED, L, P, ed_add, ed_enc

MASK255 = (1 << 255) - 1
MONT_J = 486662                                  # curve25519: K t^2 = s^3 + J s^2 + s with K = 1
ELL2_Z = 2
B_IN_BYTES, S_IN_BYTES = 64, 128                 # SHA-512
MAX_LEN_IN_BYTES = 255 * B_IN_BYTES
IDENTITY = (0, 1)


def _inv0(x: int) -> int:
    return pow(x, P - 2, P)


def _sgn0(x: int) -> int:
    return x % P & 1


def _is_square(x: int) -> bool:
    return pow(x, (P - 1) // 2, P) in (0, 1)


def _sqrt(x: int) -> int:
    r = pow(x, (P + 3) // 8, P)
    if r * r % P != x % P:
        r = r * ristretto_model.SQRT_M1 % P
    assert r * r % P == x % P
    return r


SQRT_M486664 = _sqrt(-486664 % P)
if _sgn0(SQRT_M486664):
    SQRT_M486664 = P - SQRT_M486664              # RFC 9380 6.8.2: sgn0(c1) == 0


# ---- RFC 9380 section 5 -------------------------------------------------------------------------------------------------------
def expand_message_xmd(msg: bytes, dst: bytes, len_in_bytes: int) -> bytes:
    ell = -(-len_in_bytes // B_IN_BYTES)
    assert 1 <= len_in_bytes <= MAX_LEN_IN_BYTES and ell <= 255 and 1 <= len(dst) <= 255
    dst_prime = dst + bytes([len(dst)])
    z_pad = bytes(S_IN_BYTES)
    l_i_b_str = len_in_bytes.to_bytes(2, "big")
    b_0 = hashlib.sha512(z_pad + msg + l_i_b_str + b"\x00" + dst_prime).digest()
    b = [hashlib.sha512(b_0 + b"\x01" + dst_prime).digest()]
    for i in range(2, ell + 1):
        b.append(hashlib.sha512(bytes(x ^ y for x, y in zip(b_0, b[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(b)[:len_in_bytes]


def hash_to_field(msg: bytes, dst: bytes, count: int):
    """m = 1, L = 48: each element is 48 expander bytes, big-endian, mod p"""
    uniform = expand_message_xmd(msg, dst, 48 * count)
    return [int.from_bytes(uniform[48 * i:48 * i + 48], "big") % P for i in range(count)]


# ---- RFC 9380 section 6.7.1 and 6.8.2 -----------------------------------------------------------------------------------------
def map_to_curve_elligator2(u: int):
    """(s, t) on curve25519 (K = 1, so s = x and t = y), section 6.7.1"""
    x1 = -MONT_J * _inv0(1 + ELL2_Z * u * u) % P
    if x1 == 0:
        x1 = -MONT_J % P
    gx1 = (x1 ** 3 + MONT_J * x1 * x1 + x1) % P
    x2 = (-x1 - MONT_J) % P
    gx2 = (x2 ** 3 + MONT_J * x2 * x2 + x2) % P
    if _is_square(gx1):
        x, y = x1, _sqrt(gx1)
        if _sgn0(y) != 1:
            y = P - y
    else:
        x, y = x2, _sqrt(gx2)
        if _sgn0(y) != 0:
            y = (P - y) % P
    return x, y


def montgomery_to_edwards(s: int, t: int):
    """the rational map of section 6.8.2; both exceptional denominators give the identity"""
    if t == 0 or (s + 1) % P == 0:
        return IDENTITY
    return SQRT_M486664 * s * _inv0(t) % P, (s - 1) * _inv0(s + 1) % P


def map_to_curve(u: int):
    """map_to_curve_elligator2_edwards25519(u): an affine point, no cofactor cleared"""
    return montgomery_to_edwards(*map_to_curve_elligator2(u % P))


def map_straight_line(u: int):
    """the same point by appendix G.2.1 and G.2.2, and (e1, e2, e3, e4, exceptional): which root was the first try's, the second
    try's, whether gx1 was a square (the selection), the sign of y before the fix-up, and whether the denominators vanished"""
    u %= P
    c2, c3 = pow(2, (P + 3) // 8, P), ristretto_model.SQRT_M1
    tv1 = 2 * u * u % P
    xd = (tv1 + 1) % P
    x1n = -MONT_J % P
    tv2 = xd * xd % P
    gxd = tv2 * xd % P
    gx1 = ((MONT_J * tv1 * x1n + tv2) * x1n) % P
    tv3 = gxd * gxd % P
    tv2 = tv3 * tv3 % P
    tv3 = tv3 * gxd * gx1 % P
    tv2 = tv2 * tv3 % P
    y11 = pow(tv2, (P - 5) // 8, P) * tv3 % P
    y12 = y11 * c3 % P
    e1 = y11 * y11 * gxd % P == gx1
    y1 = y11 if e1 else y12
    x2n = x1n * tv1 % P
    y21 = y11 * u * c2 % P
    y22 = y21 * c3 % P
    gx2 = gx1 * tv1 % P
    e2 = y21 * y21 * gxd % P == gx2
    y2 = y21 if e2 else y22
    e3 = y1 * y1 * gxd % P == gx1
    xn, y = (x1n, y1) if e3 else (x2n, y2)
    e4 = _sgn0(y) == 1
    if e3 != e4:
        y = -y % P
    xn_e, xd_e, yn, yd = xn * SQRT_M486664 % P, xd * y % P, (xn - xd) % P, (xn + xd) % P
    exceptional = xd_e * yd % P == 0
    if exceptional:
        xn_e, xd_e, yn, yd = 0, 1, 1, 1
    return (xn_e * _inv0(xd_e) % P, yn * _inv0(yd) % P), (e1, e2, e3, e4, exceptional)


def u_of(b: bytes) -> int:
    """u of ed25519_MapToCurve: 32 bytes little-endian, bit 255 masked, mod p"""
    return (int.from_bytes(b, "little") & MASK255) % P


def on_curve(A) -> bool:
    x, y = A
    return (-x * x + y * y - 1 - D_ED * x * x * y * y) % P == 0


def clear_cofactor(A):
    return group_model.mul(8, A)


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def map_to_curve_bytes(u32: bytes) -> bytes:
    return ed_enc(map_to_curve(u_of(u32)))


def hash_to_curve_point(msg: bytes, dst: bytes):
    u0, u1 = hash_to_field(msg, dst, 2)
    return clear_cofactor(ed_add(map_to_curve(u0), map_to_curve(u1)))


def encode_to_curve_point(msg: bytes, dst: bytes):
    return clear_cofactor(map_to_curve(hash_to_field(msg, dst, 1)[0]))


def hash_to_curve(msg: bytes, dst: bytes) -> bytes:
    """edwards25519_XMD:SHA-512_ELL2_RO_ with the caller's DST, as the 32-byte Ed25519 encoding"""
    return ed_enc(hash_to_curve_point(msg, dst))


def encode_to_curve(msg: bytes, dst: bytes) -> bytes:
    """edwards25519_XMD:SHA-512_ELL2_NU_"""
    return ed_enc(encode_to_curve_point(msg, dst))


def hash_to_group(msg: bytes, dst: bytes) -> bytes:
    """hash_to_ristretto255 of RFC 9380 appendix B: 64 expander bytes into RFC 9496's one-way map"""
    return ristretto_model.from_hash(expand_message_xmd(msg, dst, 64))


def hash_to_scalar(msg: bytes, dst: bytes) -> bytes:
    """RFC 9497 section 4.1, ristretto255-SHA512: 64 expander bytes, little-endian, mod L"""
    return (int.from_bytes(expand_message_xmd(msg, dst, 64), "little") % L).to_bytes(32, "little")


# ---- RFC 9497 (OPRF mode) on top of them ------------------------------------------------------------------------------------------
def oprf_context_string(mode: int = 0) -> bytes:
    return b"OPRFV1-" + bytes([mode]) + b"-ristretto255-SHA512"


def oprf_derive_key_pair(seed: bytes, info: bytes, mode: int = 0) -> bytes:
    derive_input = seed + len(info).to_bytes(2, "big") + info
    for counter in range(256):
        sk = hash_to_scalar(derive_input + bytes([counter]), b"DeriveKeyPair" + oprf_context_string(mode))
        if any(sk):
            return sk
    raise ValueError("DeriveKeyPairError")


def oprf_hash_to_group(x: bytes, mode: int = 0) -> bytes:
    return hash_to_group(x, b"HashToGroup-" + oprf_context_string(mode))


def oprf_finalize(x: bytes, unblinded: bytes) -> bytes:
    return hashlib.sha512(len(x).to_bytes(2, "big") + x + len(unblinded).to_bytes(2, "big") + unblinded + b"Finalize").digest()


# ---- the case set ------------------------------------------------------------------------------------------------------------
DST_LENGTHS = (1, 16, 45, 46, 61, 62, 173, 174, 255)      # the b_i input is dst_len + 66 bytes: both sides of every block edge
FULL_SWEEP_DST_LENGTHS = (16, 62)                         # the DSTs that take every message length below
BASE_MSG_LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65)
EDGE_RESIDUES = (110, 111, 112, 127, 0, 1)                # of msg_size + dst_len + 4 mod 128: around the padding's block edge
THREE_BLOCK_MSG = 300
OTHER_MSG_LENGTHS = (0, 13, 32)
ROWS_PER_CASE = 3
XMD_LENGTHS = (1, 32, 63, 64, 65, 96, 128, 129, MAX_LEN_IN_BYTES)


def _rows(rows, width):
    if not len(rows):
        return np.zeros((0, width), np.uint8)
    return np.stack([np.frombuffer(bytes(r), np.uint8) for r in rows]).reshape(len(rows), width)


def make_dst(n: int) -> bytes:
    """n bytes that name themselves: a readable head and a seeded rest"""
    head = b"QUUX-V01-CS02-h2c-case-%03d-" % n
    rest = np.random.default_rng(0x9380 + n).integers(0, 256, n, dtype=np.uint8).tobytes()
    return (head + rest)[:n]


def edge_msg_lengths(dst_len: int):
    """the six lengths in [128, 256) that put msg_size + dst_len + 4 at each of EDGE_RESIDUES mod 128"""
    return tuple(128 + (r - dst_len - 4) % 128 for r in EDGE_RESIDUES)


def msg_lengths_for(dst_len: int):
    if dst_len in FULL_SWEEP_DST_LENGTHS:
        return BASE_MSG_LENGTHS + edge_msg_lengths(dst_len) + (THREE_BLOCK_MSG,)
    return OTHER_MSG_LENGTHS


@functools.lru_cache(maxsize=None)
def _cases():
    out = []
    for dst_len in DST_LENGTHS:
        dst = make_dst(dst_len)
        for msg_size in msg_lengths_for(dst_len):
            rng = np.random.default_rng((dst_len << 16) ^ msg_size ^ 0x5A5A)
            msgs = tuple(rng.integers(0, 256, msg_size, dtype=np.uint8).tobytes() for _ in range(ROWS_PER_CASE))
            out.append((dst, msg_size, msgs))
    return tuple(out)


def case_set():
    """[(dst bytes, msg_size, msgs uint8[ROWS_PER_CASE, msg_size])]: one call's worth each -- a call has one DST and one length"""
    return [(dst, size, _rows(msgs, size)) for dst, size, msgs in _cases()]


def xmd_cases():
    """[(dst, msg_size, msgs, len_in_bytes)]: every length of XMD_LENGTHS on two cases, and 64 and 129 bytes on every case"""
    cases = case_set()
    out = []
    wide = {(16, 9), (174, 13)}
    for dst, size, msgs in cases:
        lens = XMD_LENGTHS if (len(dst), size) in wide else (64, 129)
        out += [(dst, size, msgs, n) for n in lens]
    return out


@functools.lru_cache(maxsize=None)
def _map_inputs(n_random=96, seed=0x6821):
    rng = np.random.default_rng(seed)
    vals = [0, 1, 2, P - 1, P, P + 1, 2**255 - 1, 2**255 + 5]
    rows = [int(v).to_bytes(32, "little") for v in vals]
    rows += [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n_random)]
    return tuple(rows)


def map_inputs():
    """uint8[n, 32]: u in {0, 1, 2, p - 1, p, p + 1, 2^255 - 1, bit 255 set on 5} and seeded random strings"""
    return _rows(_map_inputs(), 32)


@functools.lru_cache(maxsize=None)
def _expected(call: str, dst: bytes, msgs: tuple, extra=None):
    fn = {"hash_to_curve": hash_to_curve, "encode_to_curve": encode_to_curve, "hash_to_group": hash_to_group,
          "hash_to_scalar": hash_to_scalar}.get(call)
    if call == "xmd":
        return tuple(expand_message_xmd(m, dst, extra) for m in msgs)
    return tuple(fn(m, dst) for m in msgs)


def expected(call: str, dst: bytes, msgs, len_in_bytes=None):
    """uint8[n, width] of the model for one case; call is "xmd", "hash_to_curve", "encode_to_curve", "hash_to_group" or
    "hash_to_scalar".  Computed once per process and case."""
    rows = _expected(call, bytes(dst), tuple(bytes(m) for m in msgs), len_in_bytes)
    return _rows(rows, len_in_bytes if call == "xmd" else 32)


@functools.lru_cache(maxsize=None)
def _expected_map():
    return tuple(map_to_curve_bytes(u) for u in _map_inputs())


def expected_map():
    return _rows(_expected_map(), 32)

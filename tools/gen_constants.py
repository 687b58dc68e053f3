#!/usr/bin/env python3
"""Derives the curve constants the device code needs from their definitions (big-int arithmetic) and
writes curve25519_amd/csrc/curve_constants.cuh.  Nothing is copied from the reference; tests compare
the device results (which depend on every one of these) with the reference's outputs.

    p  = 2^255 - 19                    d  = -121665/121666 mod p
    I  = sqrt(-1) = 2^((p-1)/4)        B  = (x, 4/5) with x even
    L  = 2^252 + 27742317777372353535851937790883648493
"""
import os

p = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
inv = lambda a: pow(a, p - 2, p)
d = (-121665 * inv(121666)) % p
I = pow(2, (p - 1) // 4, p)
By = (4 * inv(5)) % p


def recover_x(y, sign):
    u, v = (y * y - 1) % p, (d * y * y + 1) % p
    x = (u * pow(v, 3, p) * pow(u * pow(v, 7, p), (p - 5) // 8, p)) % p
    if (v * x * x - u) % p:
        x = x * I % p
    assert (v * x * x - u) % p == 0
    return x if (x & 1) == sign else p - x


Bx = recover_x(By, 0)
assert (-Bx * Bx + By * By - 1 - d * Bx * Bx * By * By) % p == 0


def ed_add(P1, P2):
    (x1, y1), (x2, y2) = P1, P2
    k = d * x1 * x2 * y1 * y2 % p
    return ((x1 * y2 + x2 * y1) * inv(1 + k) % p, (y1 * y2 + x1 * x2) * inv(1 - k) % p)


def ed_mul(k, P1):
    r = (0, 1)
    while k:
        if k & 1:
            r = ed_add(r, P1)
        P1 = ed_add(P1, P1)
        k >>= 1
    return r


def order8_point():
    """L times the first decodable y >= 2 whose point has a component of order 8"""
    y = 2
    while True:
        u, v = (y * y - 1) % p, (d * y * y + 1) % p
        x = (u * pow(v, 3, p) * pow(u * pow(v, 7, p), (p - 5) // 8, p)) % p
        if (v * x * x - u) % p:
            x = x * I % p
        if (v * x * x - u) % p == 0:
            t = ed_mul(L, (x, y))
            if ed_mul(4, t) != (0, 1):
                return t
        y += 1


T8 = order8_point()
# the y of every point of small order (k * T8, k = 0..7: 1, p - 1, 0, y8, p - y8), and p, p + 1: the 255-bit y whose y mod p is one
SMALL_Y = sorted({ed_mul(k, T8)[1] for k in range(8)})
assert len(SMALL_Y) == 5 and ed_mul(8, T8) == (0, 1)
SMALL_Y_255 = SMALL_Y + [p, p + 1]


def naf(k):
    """signed binary non-adjacent form of k: (mask of the non-zero digits, mask of the negative ones)"""
    nz = neg = i = 0
    while k:
        if k & 1:
            digit = 2 - (k & 3)                       # +1 or -1: what leaves k a multiple of 4
            nz |= 1 << i
            if digit < 0:
                neg |= 1 << i
            k -= digit
        k >>= 1
        i += 1
    return nz, neg


# [L]A for a variable point A (ed_keys.cuh): the walk adds +-A at the non-zero digits of L's non-adjacent form
L_NAF_NZ, L_NAF_NEG = naf(L)
assert sum((-1 if (L_NAF_NEG >> i) & 1 else 1) << i for i in range(256) if (L_NAF_NZ >> i) & 1) == L
assert L_NAF_NZ & (L_NAF_NZ >> 1) == 0 and L_NAF_NEG & ~L_NAF_NZ == 0
assert L_NAF_NZ >> 252 == 1 and not (L_NAF_NEG >> 252) & 1 and (L_NAF_NZ & ((1 << 252) - 1)) < 1 << 127


def sqrt_mod(v):
    r = pow(v, (p + 3) // 8, p)
    if (r * r - v) % p:
        r = r * I % p
    assert (r * r - v) % p == 0
    return r


# ristretto255 (RFC 9496 section 4.1; ristretto255.cuh), from d: a - d = -1 - d, a d - 1 = -d - 1.  The RFC lists the even
# ("non-negative") root of 1 / (a - d) and the ODD root of a d - 1: the even one maps a hash to the negated point.
even = lambda r: r if r % 2 == 0 else p - r                 # noqa: E731
INVSQRT_A_MINUS_D = even(inv(sqrt_mod((-1 - d) % p)))
SQRT_AD_MINUS_ONE = p - even(sqrt_mod((-d - 1) % p))
ONE_MINUS_D_SQ = (1 - d * d) % p
D_MINUS_ONE_SQ = (d - 1) ** 2 % p
assert INVSQRT_A_MINUS_D == 54469307008909316920995813868745141605393597292927456921205312896311721017578
assert SQRT_AD_MINUS_ONE == 25063068953384623474111414158702152701244531502492656460079210482610430750235
assert ONE_MINUS_D_SQ == 1159843021668779879193775521855586647937357759715417654439879720876111806838
assert D_MINUS_ONE_SQ == 40440834346308536858101042469323190826248399146238708352240133220865137265952
assert INVSQRT_A_MINUS_D ** 2 * (-1 - d) % p == 1 and SQRT_AD_MINUS_ONE ** 2 % p == (-d - 1) % p and SQRT_AD_MINUS_ONE & 1


# inversion mod L by division steps (sc_invert.cuh): L in the 30-bit limbs of safegcd25519.cuh and L^-1 mod 2^30.  L = 2^252 + c with
# c < 2^125, so limbs 0..4 hold c, limbs 5..7 are zero and limb 8 is 2^(252 - 240): six multiply-adds per number and batch.
L_LIMBS30 = [(L >> (30 * i)) & (2**30 - 1) for i in range(9)]
L_INV30 = pow(L, -1, 2**30)
assert sum(v << (30 * i) for i, v in enumerate(L_LIMBS30)) == L and L >> 270 == 0
assert all(L_LIMBS30[i] for i in (0, 1, 2, 3, 4)) and L_LIMBS30[5:8] == [0, 0, 0] and L_LIMBS30[8] == 1 << 12
assert L * L_INV30 % 2**30 == 1 and L_INV30 == 0x2DAB81E5


# hashing to the curve (RFC 9380; h2c25519.cuh).  The Elligator 2 map to curve25519 (J = 486662, Z = 2) in appendix G.2.1's
# straight-line form needs -J, c2 = 2^((p + 3) / 8) (which turns a root of gx1 times u into a root of gx2 = 2 u^2 gx1) and sqrt(-1);
# the rational map to the Edwards curve (6.8.2) needs sqrt(-486664) with sgn0 = 0, the even root.
MONT_J = 486662
H2C_NEG_J = p - MONT_J
H2C_C2 = pow(2, (p + 3) // 8, p)
H2C_SQRT_M486664 = even(sqrt_mod(-(MONT_J + 2) % p))
assert H2C_SQRT_M486664 == 0x0F26EDF460A006BBD27B08DC03FC4F7EC5A1D3D14B7D1A82CC6E04AAFF457E06
assert H2C_SQRT_M486664 ** 2 % p == -(MONT_J + 2) % p and H2C_SQRT_M486664 % 2 == 0
assert H2C_C2 ** 4 % p == p - 4 and pow(-MONT_J % p, (p - 1) // 2, p) == p - 1          # -J is no square: u = 0 maps to (0, 0)
assert pow((MONT_J - 1) * inv(2) % p, (p - 1) // 2, p) == p - 1                          # (J - 1) / 2 neither: no u gives x = -1


# SHA-512's constants from their definition (FIPS 180-4 section 4.2.3, 5.3.5: the fractional parts of the cube and square roots of
# the first primes) and its compression function, to give the state after Z_pad, the 128 zero bytes every b_0 of expand_message_xmd
# starts with (RFC 9380 section 5.3.1): a constant of the suite, so no lane compresses that block.
def _iroot(n, k):
    lo, hi = 0, 1 << (n.bit_length() // k + 1)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if mid ** k <= n else (lo, mid - 1)
    return lo


M64 = 2**64 - 1
_primes = [q for q in range(2, 410) if all(q % r for r in range(2, q))][:80]
SHA512_K = [_iroot(q << 192, 3) & M64 for q in _primes]
SHA512_IV = [_iroot(q << 128, 2) & M64 for q in _primes[:8]]
assert SHA512_K[0] == 0x428A2F98D728AE22 and SHA512_K[79] == 0x6C44198C4A475817 and SHA512_IV[0] == 0x6A09E667F3BCC908


def sha512_compress(state, block):
    rotr = lambda x, n: (x >> n | x << (64 - n)) & M64      # noqa: E731
    w = [int.from_bytes(block[8 * i:8 * i + 8], "big") for i in range(16)]
    for i in range(16, 80):
        s0 = rotr(w[i - 15], 1) ^ rotr(w[i - 15], 8) ^ w[i - 15] >> 7
        s1 = rotr(w[i - 2], 19) ^ rotr(w[i - 2], 61) ^ w[i - 2] >> 6
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & M64)
    a, b, c, dd, e, f, g, h = state
    for i in range(80):
        t1 = (h + (rotr(e, 14) ^ rotr(e, 18) ^ rotr(e, 41)) + (e & f ^ ~e & g) + SHA512_K[i] + w[i]) & M64
        t2 = ((rotr(a, 28) ^ rotr(a, 34) ^ rotr(a, 39)) + (a & b ^ a & c ^ b & c)) & M64
        a, b, c, dd, e, f, g, h = (t1 + t2) & M64, a, b, c, (dd + t1) & M64, e, f, g
    return [(x + y) & M64 for x, y in zip(state, (a, b, c, dd, e, f, g, h))]


def _sha512_check():
    import hashlib
    msg = b"abc"
    block = msg + b"\x80" + bytes(128 - 1 - 16 - len(msg)) + (8 * len(msg)).to_bytes(16, "big")
    got = b"".join(x.to_bytes(8, "big") for x in sha512_compress(SHA512_IV, block))
    assert got == hashlib.sha512(msg).digest()
    mid = sha512_compress(SHA512_IV, bytes(128))
    tail = b"\x80" + bytes(128 - 1 - 16) + (8 * 128).to_bytes(16, "big")
    assert b"".join(x.to_bytes(8, "big") for x in sha512_compress(mid, tail)) == hashlib.sha512(bytes(128)).digest()
    return mid


SHA512_ZPAD_MID = _sha512_check()


def words(v):
    return ", ".join("0x%08xu" % ((v >> (32 * i)) & 0xFFFFFFFF) for i in range(8))


consts = [
    ("K_D", d, "d = -121665/121666"),
    ("K_2D", 2 * d % p, "2d"),
    ("K_DI", inv(d), "1/d"),
    ("K_SQRTM1", I, "sqrt(-1)"),
    ("K_BX", Bx, "base point x"),
    ("K_BY", By, "base point y = 4/5"),
    ("K_BT2D", 2 * d * Bx * By % p, "2d * Bx * By"),
    ("K_INVSQRT_A_MINUS_D", INVSQRT_A_MINUS_D, "ristretto255: 1/sqrt(a - d), the even root"),
    ("K_SQRT_AD_MINUS_ONE", SQRT_AD_MINUS_ONE, "ristretto255: sqrt(a d - 1), the odd root"),
    ("K_ONE_MINUS_D_SQ", ONE_MINUS_D_SQ, "ristretto255: 1 - d^2"),
    ("K_D_MINUS_ONE_SQ", D_MINUS_ONE_SQ, "ristretto255: (d - 1)^2"),
    ("K_H2C_NEG_J", H2C_NEG_J, "hash to curve: -J = -486662, the first x of Elligator 2 on curve25519"),
    ("K_H2C_C2", H2C_C2, "hash to curve: 2^((p + 3) / 8)"),
    ("K_H2C_SQRT_M486664", H2C_SQRT_M486664, "hash to curve: sqrt(-486664), the even root"),
]
out = ["// GENERATED by tools/gen_constants.py -- do not edit.  256-bit little-endian 32-bit words.",
       "#pragma once", "#include <stdint.h>", "namespace c25519 {"]
for name, v, doc in consts:
    out.append("// %s = 0x%064x" % (doc, v))
    out.append("__device__ constexpr uint32_t %s[8] = { %s };" % (name, words(v)))
out.append("// group order L and 16*c = -2^256 mod L (c = L - 2^252)")
out.append("__device__ constexpr uint32_t K_L[8] = { %s };" % words(L))
out.append("__device__ constexpr uint32_t K_MINUS_R[5] = { %s };" % ", ".join(
    "0x%08xu" % (((16 * (L - 2**252)) >> (32 * i)) & 0xFFFFFFFF) for i in range(5)))
out.append("// multiples of L that keep sc_reduce512's two folds non-negative: L << 134 (13 words, > 2^385) and L << 9 (9 words, > 2^260)")
out.append("__device__ constexpr uint32_t K_L_SHL134[13] = { %s };" % ", ".join("0x%08xu" % (((L << 134) >> (32 * i)) & 0xFFFFFFFF) for i in range(13)))
out.append("__device__ constexpr uint32_t K_L_SHL9[9] = { %s };" % ", ".join("0x%08xu" % (((L << 9) >> (32 * i)) & 0xFFFFFFFF) for i in range(9)))
out.append("// L as nine 30-bit limbs (limbs 5..7 are zero, limb 8 is 2^12) and L^-1 mod 2^30: the modulus of sc_invert.cuh's division steps")
out.append("__device__ constexpr int32_t K_L_LIMBS30[9] = { %s };" % ", ".join("0x%08x" % v for v in L_LIMBS30))
out.append("constexpr uint32_t K_L_INV30 = 0x%08xu;" % L_INV30)
out.append("// p = 2^255 - 19, and the 255-bit y whose y mod p is the y of a point of small order: 0, 1, the two y of the points of")
out.append("// order 8, p - 1, p, p + 1 (strict25519.cuh)")
out.append("__device__ constexpr uint32_t K_P[8] = { %s };" % words(p))
out.append("__device__ constexpr uint32_t K_SMALL_Y[%d][8] = {" % len(SMALL_Y_255))
out += ["    { %s }," % words(v) for v in SMALL_Y_255]
out.append("};")
out.append("// L in signed binary non-adjacent form, L = sum of +-2^i: bit i of K_L_NAF_NZ is set where digit i is not zero (%d digits, the top"
           % bin(L_NAF_NZ).count("1"))
out.append("// one at bit 252, the others below bit %d), bit i of K_L_NAF_NEG where it is -1 (ed_keys.cuh: the walk [L]A)"
           % (L_NAF_NZ & ((1 << 252) - 1)).bit_length())
out.append("__device__ constexpr uint32_t K_L_NAF_NZ[8] = { %s };" % words(L_NAF_NZ))
out.append("__device__ constexpr uint32_t K_L_NAF_NEG[8] = { %s };" % words(L_NAF_NEG))
out.append("// SHA-512's state after the 128 zero bytes of Z_pad (RFC 9380 section 5.3.1): where every b_0 starts")
out.append("__device__ constexpr uint64_t K_SHA512_ZPAD_MID[8] = { %s };" % ", ".join("0x%016xull" % v for v in SHA512_ZPAD_MID))
out.append("}  // namespace c25519")
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "curve25519_amd", "csrc", "curve_constants.cuh")
open(path, "w").write("\n".join(out) + "\n")
print("wrote", os.path.normpath(path))

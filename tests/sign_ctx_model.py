"""Big-integer model of the signer context of ed25519_Sign_Init_* and of a signature under it (ed25519_SignMessage_indexed_*), for
the tests: the 128-byte layout of include/curve25519_amd.h built with hashlib, and R = r*B, S = (h*a + r) mod L on the Edwards curve
for ANY context bytes (a read as a full 256-bit integer, the prefix and pk as given, bytes 96..127 ignored).  Slow and simple."""
import hashlib

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
BY = 4 * pow(5, P - 2, P) % P
BX = None


def _recover_x(y, sign):
    x2 = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * pow(2, (P - 1) // 4, P) % P
    if x & 1 != sign:
        x = P - x
    return x


BX = _recover_x(BY, 0)
B = (BX, BY, 1, BX * BY % P)


def _add(p, q):
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 - x2) % P
    b = (y1 + x1) * (y2 + x2) % P
    c = 2 * D * t1 * t2 % P
    d = 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def _mult(k, p=B):
    q = (0, 1, 1, 0)
    while k:
        if k & 1:
            q = _add(q, p)
        p = _add(p, p)
        k >>= 1
    return q


def _encode(p):
    x, y, z, _ = p
    zi = pow(z, P - 2, P)
    x, y = x * zi % P, y * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def clamp(a: bytes) -> bytes:
    a = bytearray(a)
    a[0] &= 248
    a[31] &= 127
    a[31] |= 64
    return bytes(a)


def sign_ctx(priv: bytes) -> bytes:
    """ed25519_Sign_Init of one 64-byte privKey (seed || pk): a || prefix || pk (as given) || 32 zero bytes"""
    priv = bytes(priv)
    dg = hashlib.sha512(priv[:32]).digest()
    return clamp(dg[:32]) + dg[32:] + priv[32:64] + bytes(32)


def sign_with_ctx(ctx: bytes, msg: bytes) -> bytes:
    """the 64-byte signature of `msg` under a 128-byte context, whatever its bytes"""
    ctx, msg = bytes(ctx), bytes(msg)
    a = int.from_bytes(ctx[:32], "little")
    prefix, pk = ctx[32:64], ctx[64:96]
    r = int.from_bytes(hashlib.sha512(prefix + msg).digest(), "little") % L
    enc_r = _encode(_mult(r))
    h = int.from_bytes(hashlib.sha512(enc_r + pk + msg).digest(), "little") % L
    return enc_r + ((h * a + r) % L).to_bytes(32, "little")

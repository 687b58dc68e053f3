"""Python big-integer model of the 1600-byte X25519 peer context (curve25519_dh_Peer_Init, include/curve25519_amd.h) for the
indexed X25519 tests (tests/test_host_emul_peer_ctx.py, tests/test_gpu_peer_indexed.py):

    bytes 0..31     the key as given          bytes 32..35  uint32 eligibility (1 / 0)      bytes 36..63  zero
    bytes 64..1599  16 rows of 96 bytes: row k = sum over the set bits i of k of 2^(64 i) * Q, Q = 8 P, affine,
                    as Y+X | Y-X | 2d*X*Y in canonical little-endian bytes; row 0 = (1, 1, 0)

P is the Edwards image of u = key mod 2^256 mod p, y = (u - 1) / (u + 1), x the even root.  A key on the twist, and u = -1, have
eligibility 0 and zero rows."""
import numpy as np

import one_peer_cases as cases

P = cases.P
D = -121665 * pow(121666, -1, P) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
CTX_SIZE = 1600


def edwards_add(a, b):
    (x1, y1), (x2, y2) = a, b
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * pow(1 + t, -1, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, -1, P) % P)


def edwards_point(u: int):
    """the point ge_calc_x_checked(.., parity 0) decodes for u's y, or None when the key is not eligible"""
    if not cases.eligible(u):
        return None
    u %= P
    y = (u - 1) * pow(u + 1, -1, P) % P
    x2 = (y * y - 1) * pow(D * y * y + 1, -1, P) % P
    x = pow(x2, (P + 3) // 8, P)
    if x * x % P != x2:
        x = x * SQRT_M1 % P
    assert x * x % P == x2
    if x & 1:
        x = P - x
    return (x, y)


def row_bytes(pt) -> bytes:
    x, y = pt
    return b"".join(v.to_bytes(32, "little") for v in ((y + x) % P, (y - x) % P, 2 * D * x * y % P))


def context(pk: bytes) -> bytes:
    """the 1600 bytes curve25519_dh_Peer_Init writes for the 32-byte key pk"""
    pt = edwards_point(int.from_bytes(pk, "little"))
    head = bytes(pk) + (1 if pt else 0).to_bytes(4, "little") + bytes(28)
    if pt is None:
        return head + bytes(16 * 96)
    for _ in range(3):
        pt = edwards_add(pt, pt)                   # Q = 8 P
    base = [pt]
    for _ in range(3):
        b = base[-1]
        for _ in range(64):
            b = edwards_add(b, b)
        base.append(b)                             # 2^64 Q, 2^128 Q, 2^192 Q
    rows = []
    for k in range(16):
        acc = (0, 1)
        for i in range(4):
            if (k >> i) & 1:
                acc = edwards_add(acc, base[i])
        rows.append(row_bytes(acc))
    return head + b"".join(rows)


def contexts(pks) -> np.ndarray:
    return np.array([np.frombuffer(context(bytes(pk)), np.uint8) for pk in pks]).reshape(-1, CTX_SIZE)

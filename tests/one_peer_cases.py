"""The peer keys of the one-peer X25519 tests (tests/test_host_emul_one_peer.py, tests/test_gpu_one_peer.py) and the Python
big-integer model they are judged by: the RFC 7748 ladder with u read UNMASKED (all 256 bits mod p, as the reference reads
it), and which u lie on the curve, on its twist, or carry a torsion component."""
import json
import os
import random

P = 2 ** 255 - 19
A = 486662
L = 2 ** 252 + 27742317777372353535851937790883648493

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# u of the points of order 1, 2, 4 and 8 (0, 1, the two of order 8), some of them as non-canonical 256-bit encodings
ORDER8 = (325606250916557431795983626356110631294008115727848805560023387167927233504,
          39382357235489614581723060781553021112529911719440698176882885853963445705823)
SMALL_ORDER = (0, 1, *ORDER8, P, P + 1, ORDER8[0] + P, ORDER8[1] + P)
TWIST = (2, 3, 5)                      # on the quadratic twist
MINUS_ONE = (P - 1, 2 * P - 1)         # u = -1: no Edwards image


def clamp(k: int) -> int:
    return (k & ~7 & ~(1 << 255)) | (1 << 254)


def ladder_xz(u: int, k: int):
    """(X : Z) of k * (u, .) by the Montgomery ladder over all 255 bits of k (RFC 7748 5, without masking u)"""
    x1 = u % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in reversed(range(255)):
        kt = (k >> t) & 1
        swap ^= kt
        if swap:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b, c, d = x2 + z2, x2 - z2, x3 + z3, x3 - z3
        aa, bb, da, cb = a * a, b * b, d * a, c * b
        e = aa - bb
        x3, z3 = (da + cb) ** 2 % P, x1 * (da - cb) ** 2 % P
        x2, z2 = aa * bb % P, e * (aa + 121665 * e) % P
    if swap:
        x2, z2 = x3, z3
    return x2, z2


def ladder(u: int, k: int) -> int:
    x2, z2 = ladder_xz(u, k)
    return x2 * pow(z2, P - 2, P) % P


def shared(pk: bytes, sk: bytes) -> bytes:
    return ladder(int.from_bytes(pk, "little"), clamp(int.from_bytes(sk, "little"))).to_bytes(32, "little")


def on_curve(u: int) -> bool:
    """u^3 + A u^2 + u is a square mod p (0 included)"""
    u %= P
    r = (u * u * u + A * u * u + u) % P
    return r == 0 or pow(r, (P - 1) // 2, P) == 1


def eligible(u: int) -> bool:
    """the one-peer comb may stand in for the ladder: u on the curve and u != -1 (mod p)"""
    return on_curve(u) and u % P != P - 1


def has_torsion(u: int) -> bool:
    """L * P != O for an on-curve u: P is not in the prime-order subgroup"""
    return ladder_xz(u, L)[1] % P != 0 if u % P else True


def to_bytes(u: int) -> bytes:
    return u.to_bytes(32, "little")


def kat_peers():
    recs = json.load(open(os.path.join(GOLD, "kat.json")))["x25519"]
    seen, out = set(), []
    for r in recs:
        if r["pk"] not in seen:
            seen.add(r["pk"])
            out.append(bytes.fromhex(r["pk"]))
    return out


def fixed_peers():
    """(name, 32 bytes) of every fixed class: the KAT keys, small order, twist, u = -1, bit 255 set"""
    out = [(f"kat{i}", pk) for i, pk in enumerate(kat_peers())]
    out += [(f"small{i}", to_bytes(u)) for i, u in enumerate(SMALL_ORDER)]
    out += [(f"twist{u}", to_bytes(u)) for u in TWIST]
    out += [(f"minus_one{i}", to_bytes(u)) for i, u in enumerate(MINUS_ONE)]
    on = next(j for j in range(100) if eligible(2 ** 255 + j))
    off = next(j for j in range(100) if not on_curve(2 ** 255 + j))
    out += [("bit255_on", to_bytes(2 ** 255 + on)), ("bit255_off", to_bytes(2 ** 255 + off)),
            ("bit255_rfc", bytes.fromhex(kat_peers()[0].hex()[:-2] + "cc"))]
    return out


def random_peers(count: int, seed: int):
    """(name, 32 bytes): `count` public keys of random secrets (x(s * 9), prime order) and `count` random byte strings"""
    rng = random.Random(seed)
    out = [(f"pub{i}", shared(to_bytes(9), rng.randbytes(32))) for i in range(count)]
    out += [(f"raw{i}", rng.randbytes(32)) for i in range(count)]
    return out

"""The ZIP-215 rule WITHOUT decoding R, as ed25519_Verify_Check_zip215_* decides it (curve25519_amd/csrc/verify_ctx_zip215.cuh), in
Python big integers.  With T = [S]B - [k]A, rule 4 -- [8](T - R) = O -- says that R lies in the coset T + E[8]; so rules 3 and 4 hold
exactly when, for one of the eight points C = T + t with t of small order,  y_R = y_C  and  (x_C = 0 or parity(x_C) = the sign bit),
where y_R = (the low 255 bits of R's string) mod p.  No square root of R is taken.

Two forms of that comparison live here: coset_affine enumerates T + t with the group law over the eight torsion points (decoded from
tests/vectors.py's small_order_encodings), and coset_projective is the device's algebra on (X : Y : Z) -- one inversion of
Z (Z^2 + kXY)(Z^2 - kXY), the four candidates that share Z and the four that come from a point of order 8.  The tests
(tests/test_check_zip215_model.py) hold both against tests/zip215_cases.py's zip215_verdict, which does decode R and multiplies by 8.
Nothing here comes from the device code: the constants below are derived, and the device header's are checked against them."""
import functools
import hashlib
import random

import numpy as np

from vectors import D_ED, ED_B, L, P, ed_add, ed_decode, ed_enc, ed_mul, ed_order8_point, small_order_encodings
from zip215_cases import MASK255, zip215_decode

SQRTM1 = pow(2, (P - 1) // 4, P)
T8 = ed_order8_point()
X8, Y8 = T8
K8 = D_ED * X8 * Y8 % P                      # 1 +- c = (Z^2 +- K8 XY) / Z^2 for c = d x y x8 y8


def words(v):
    """the 8 little-endian 32-bit words of a 256-bit value, as the device headers spell their constants"""
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


@functools.lru_cache(maxsize=None)
def torsion_points():
    """E[8]: the eight points of small order, decoded from every string that decodes to one"""
    pts = {zip215_decode(e) for e, _ in small_order_encodings()}
    assert len(pts) == 8 and all(ed_mul(8, t) == (0, 1) for t in pts)
    return sorted(pts)


def split_r(Rb):
    v = int.from_bytes(bytes(Rb), "little")
    return (v & MASK255) % P, v >> 255


def matches(cand, y_r, sign):
    x, y = cand
    return y == y_r and (x == 0 or (x & 1) == sign)


def coset_affine(T, Rb):
    """rules 3 and 4 for affine T: some T + t encodes, in ZIP-215's sense, to R's string"""
    y_r, sign = split_r(Rb)
    return int(any(matches(ed_add(T, t), y_r, sign) for t in torsion_points()))


def coset_prep(X, Y, Z):
    """what the coset prep kernel leaves for the shared inversion: Z (Z^2 + kXY)(Z^2 - kXY)"""
    zz, kxy = Z * Z % P, K8 * X * Y % P
    return Z * (zz + kxy) * (zz - kxy) % P


def coset_candidates(X, Y, Z, w_inv):
    """the eight candidates from (X : Y : Z) and w_inv = 1 / coset_prep(X, Y, Z), as four (x, y) whose negatives are the other four"""
    zz, kxy = Z * Z % P, K8 * X * Y % P
    dp, dm = (zz + kxy) % P, (zz - kxy) % P
    z_inv = w_inv * dp * dm % P
    wz = w_inv * Z % P
    zdp, zdm = wz * dm * Z % P, wz * dp * Z % P              # Z / (Z^2 + kXY), Z / (Z^2 - kXY)
    x, y = X * z_inv % P, Y * z_inv % P
    a, b, c, e = X * Y8 % P, Y * X8 % P, Y * Y8 % P, X * X8 % P
    return [(x, y), (SQRTM1 * y % P, SQRTM1 * x % P), ((a + b) * zdp % P, (c + e) * zdm % P), ((a - b) * zdm % P, (c - e) * zdp % P)]


def coset_projective(X, Y, Z, Rb):
    """rules 3 and 4 for projective T, the device's way; a zero product (Z = 0, or a point that is not on the curve) gives 0"""
    w = coset_prep(X, Y, Z)
    if w == 0:
        return 0
    y_r, sign = split_r(Rb)
    for x, y in coset_candidates(X, Y, Z, pow(w, P - 2, P)):
        if matches((x, y), y_r, sign) or matches(((P - x) % P, (P - y) % P), y_r, sign):
            return 1
    return 0


def key_on_curve_from_row1(ypx, ymx, y_key):
    """rule 2 from a Verify_Init context: row 1 holds -A as (y + x, y - x, 2dxy, 2); the key decodes exactly when that (x, y) is on
    the curve, and its y is the key's y mod p"""
    half = pow(2, P - 2, P)
    x, y = (ypx - ymx) * half % P, (ypx + ymx) * half % P
    return int((y * y - x * x - 1 - D_ED * x * x % P * y * y) % P == 0 and y == y_key)


def hram(Rb, pk, msg):
    return int.from_bytes(hashlib.sha512(bytes(Rb) + bytes(pk) + bytes(msg)).digest(), "little") % L


def walk_point(sig, pk, msg):
    """T = [S]B - [k]A for a key that decodes (None otherwise), S the raw 256 bits as the context kernels take them"""
    return _walk_point(bytes(sig), bytes(pk), bytes(msg))


def _ext_add(p, q):
    """the unified addition in extended coordinates (complete on this curve): no inversion per step, unlike vectors.ed_add"""
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a, b = (y1 - x1) * (y2 - x2) % P, (y1 + x1) * (y2 + x2) % P
    c, d = 2 * D_ED * t1 * t2 % P, 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def fast_mul(k, pt):
    """k * pt, affine: vectors.ed_mul's value (tests/test_check_zip215_model.py compares them) with one inversion instead of two
    per addition"""
    r, q = (0, 1, 1, 0), (pt[0], pt[1], 1, pt[0] * pt[1] % P)
    while k:
        if k & 1:
            r = _ext_add(r, q)
        q = _ext_add(q, q)
        k >>= 1
    zi = pow(r[2], P - 2, P)
    return (r[0] * zi % P, r[1] * zi % P)


@functools.lru_cache(maxsize=None)
def _walk_point(sig, pk, msg):
    A = zip215_decode(pk)
    if A is None:
        return None
    S = int.from_bytes(bytes(sig[32:]), "little")
    kA = fast_mul(hram(sig[:32], pk, msg), A)
    return ed_add(fast_mul(S, ED_B), ((P - kA[0]) % P, kA[1]))


def check_verdict(sig, pk, msg, z=None):
    """the verdict of ed25519_Verify_Check_zip215_* for a Verify_Init context of `pk`.  z: run the projective algebra on (xz : yz : z)"""
    sig, pk, msg = bytes(sig), bytes(pk), bytes(msg)
    if int.from_bytes(sig[32:], "little") >= L:               # rule 1
        return 0
    T = walk_point(sig, pk, msg)
    if T is None:                                             # rule 2
        return 0
    if z is None:
        return coset_affine(T, sig[:32])
    return coset_projective(T[0] * z % P, T[1] * z % P, z % P, sig[:32])


def undecodable_strings(count, seed=0x215):
    """`count` 32-byte strings whose y has no square root for x (either sign bit)"""
    rnd = random.Random(seed)
    out = []
    while len(out) < count:
        y = rnd.getrandbits(255) % P
        if ed_decode(y, 0) is None:
            out.append((y | (rnd.getrandbits(1) << 255)).to_bytes(32, "little"))
    return out


def encodings_of(pt):
    """every string ZIP-215 decodes to `pt`: canonical, y + p where that fits 255 bits, either sign bit on x = 0"""
    x, y = pt
    ys = [y] + ([y + P] if y + P < 2**255 else [])
    signs = [0, 1] if x == 0 else [x & 1]
    return [(yy | (s << 255)).to_bytes(32, "little") for yy in ys for s in signs]


@functools.lru_cache(maxsize=None)
def generated_set(keys=2, seed=0x2150, msg_len=16):
    """(sig, pk, msg, label): for keys a*B + t and each of the eight torsion shifts j of R = r*B + j*T8 with S = r + k*a -- valid
    under ZIP-215 whatever t and j --: every encoding of R, the sign bit flipped, one y bit flipped, S + 1, S + L, an undecodable
    R, an undecodable key; plus R of small order (where the non-canonical encodings exist) under keys of small order"""
    rnd = random.Random(seed)
    tors = torsion_points()
    und = undecodable_strings(8 * keys + keys, seed)
    sigs, pks, msgs, labels = [], [], [], []

    def put(Rb, S, pk, m, label):
        sigs.append(bytes(Rb) + (S % 2**256).to_bytes(32, "little")); pks.append(bytes(pk)); msgs.append(m); labels.append(label)

    for kk in range(keys):
        a = rnd.getrandbits(252) % L
        pk = ed_enc(ed_add(fast_mul(a, ED_B), tors[(3 * kk + 1) % 8]))
        for j in range(8):
            m = rnd.getrandbits(8 * msg_len).to_bytes(msg_len, "little")
            r = rnd.getrandbits(252) % L
            Rpt = ed_add(fast_mul(r, ED_B), tors[j])

            def s_for(Rb, key=pk):
                return (r + hram(Rb, key, m) * a) % L

            for Rb in encodings_of(Rpt):
                put(Rb, s_for(Rb), pk, m, "valid")
            Rb = ed_enc(Rpt)
            flip = bytes(Rb[:31]) + bytes([Rb[31] ^ 0x80])
            put(flip, s_for(flip), pk, m, "sign_flipped")
            bit = rnd.randrange(255)
            ybit = (int.from_bytes(Rb, "little") ^ (1 << bit)).to_bytes(32, "little")
            put(ybit, s_for(ybit), pk, m, "y_bit_flipped")
            put(Rb, s_for(Rb) + 1, pk, m, "s_plus_1")
            put(Rb, s_for(Rb) + L, pk, m, "s_plus_l")
            bad_r = und[8 * kk + j]
            put(bad_r, s_for(bad_r), pk, m, "r_undecodable")
        bad_key = und[8 * keys + kk]
        Rb = ed_enc(fast_mul(rnd.getrandbits(252) % L, ED_B))
        put(Rb, rnd.getrandbits(252) % L, bad_key, b"k" * msg_len, "key_undecodable")
    # small-order R in every encoding (y + p and the sign bit on x = 0 exist only there) under a mixed-order key with S = k*a, and
    # under a small-order key with S = 0
    a = rnd.getrandbits(252) % L
    mixed = ed_enc(ed_add(fast_mul(a, ED_B), tors[5]))
    small = ed_enc(tors[6])
    for i, (Rb, _) in enumerate(small_order_encodings()):
        m = bytes([i]) * msg_len
        put(Rb, hram(Rb, mixed, m) * a % L, mixed, m, "small_r_valid")
        put(Rb, hram(Rb, mixed, m) * a % L + 1, mixed, m, "small_r_s_plus_1")
        put(Rb, 0, small, m, "small_r_small_key")
    f = lambda rows: np.stack([np.frombuffer(x, np.uint8) for x in rows])  # noqa: E731
    return f(sigs), f(pks), f(msgs), labels


def model_verdicts(sig, pk, msg):
    return np.array([check_verdict(sig[i], pk[i], msg[i]) for i in range(len(sig))], np.int32)

"""ECVRF-EDWARDS25519-SHA512-ELL2 (RFC 9381, suite string 0x04) as ed25519_VRF_Prove_*, ed25519_VRF_Verify_* and
ed25519_VRF_ProofToHash_* state it (include/curve25519_amd.h), in Python big integers and in the RFC's order, and the case set the CPU
and GPU tests of those calls share.  Built on tests/h2c_model.py's encode_to_curve, tests/group_model.py's mul, tests/key_model.py's
decoder and hashlib; tests/test_vrf_model.py pins it to the RFC's three examples.  A walk costs ~2 ms, a proof three of them and a
verification five: the set is a few dozen distinct rows, memoised, and cycled to fill larger calls (scalar_model.cycled)."""
import functools
import hashlib

import numpy as np

import group_model
import h2c_model
import key_model
from key_model import NEUTRAL, clamp
from vectors import ED_B, L, P, ed_add, ed_enc, ed_order8_point

SUITE = b"\x04"
DST = b"ECVRF_" + b"edwards25519_XMD:SHA-512_ELL2_NU_" + SUITE
PROOF_SIZE, OUTPUT_SIZE, C_LEN = 80, 64, 16
ZERO_BETA = bytes(OUTPUT_SIZE)

# the RFC's examples 16, 17 and 18 (appendix B.3): SK, alpha, PK, pi, beta; the first with its H, U and V
EXAMPLES = (
    dict(sk="9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60", alpha="",
         pk="d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a",
         H="b8066ebbb706c72b64390324e4a3276f129569eab100c26b9f05011200c1bad9",
         U="762f5c178b68f0cddcc1157918edf45ec334ac8e8286601a3256c3bbf858edd9",
         V="4652eba1c4612e6fce762977a59420b451e12964adbe4fbecd58a7aeff5860af",
         pi="7d9c633ffeee27349264cf5c667579fc583b4bda63ab71d001f89c10003ab46f14adf9a3cd8b8412d9038531e865c341"
            "cafa73589b023d14311c331a9ad15ff2fb37831e00f0acaa6d73bc9997b06501",
         beta="9d574bf9b8302ec0fc1e21c3ec5368269527b87b462ce36dab2d14ccf80c53cccf6758f058c5b1c856b116388152bbe5"
              "09ee3b9ecfe63d93c3b4346c1fbc6c54"),
    dict(sk="4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb", alpha="72",
         pk="3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c",
         pi="47b327393ff2dd81336f8a2ef10339112401253b3c714eeda879f12c509072ef055b48372bb82efbdce8e10c8cb9a2f9"
            "d60e93908f93df1623ad78a86a028d6bc064dbfc75a6a57379ef855dc6733801",
         beta="38561d6b77b71d30eb97a062168ae12b667ce5c28caccdf76bc88e093e4635987cd96814ce55b4689b3dd2947f80e59a"
              "ac7b7675f8083865b46c89b2ce9cc735"),
    dict(sk="c5aa8df43f9f837bedb7442f31dcb7b166d38535076f094b85ce3a2e0b4458f7", alpha="af82",
         pk="fc51cd8e6218a1a38da47ed00230f0580816ed13ba3303ac5deb911548908025",
         pi="926e895d308f5e328e7aa159c06eddbe56d06846abf5d98c2512235eaa57fdce35b46edfc655bc828d44ad09d1150f31"
            "374e7ef73027e14760d42e77341fe05467bb286cc2c9d7fde29120a0b2320d04",
         beta="121b7f9b9aaaa29099fc04a94ba52784d44eac976dd1a3cca458733be5cd090a7b5fbd148444f17f8daf1fb55cb04b1a"
              "e85a626e30a54b4b0f8abf4a43314a58"),
)

# alpha lengths of the honest proofs: the word straddle behind the 32 key bytes; msg_size + dst_len + 4 = 110, 111, 112, 127, 0, 1
# mod 128 (msg_size = 32 + alpha, a 40-byte DST), the padding's block edge; several blocks
ALPHA_LENGTHS = (0, 1, 7, 8, 9, 34, 35, 36, 51, 52, 53, 300)
assert [(32 + a + len(DST) + 4) % 128 for a in ALPHA_LENGTHS[5:11]] == [110, 111, 112, 127, 0, 1]
REJECT_ALPHA = 9                                  # the alpha length of the rejection rows
ROWS_PER_LENGTH = 2


# ---- the construction ------------------------------------------------------------------------------------------------------
def _le(v: int, n: int = 32) -> bytes:
    return int(v).to_bytes(n, "little")


def _neg(A):
    return ((P - A[0]) % P, A[1])


@functools.lru_cache(maxsize=None)
def _mul(k: int, A):
    return group_model.mul(k, A)


def secret_scalar(seed: bytes):
    """(x, the hash prefix) of a 32-byte seed (section 5.4.5's first steps, RFC 8032's key expansion)"""
    h = hashlib.sha512(seed).digest()
    return int.from_bytes(clamp(h[:32]), "little"), h[32:]


def public_key(seed: bytes) -> bytes:
    return ed_enc(_mul(secret_scalar(seed)[0], ED_B))


def private_key(seed: bytes) -> bytes:
    """the 64-byte private key the calls take: seed || public key"""
    return seed + public_key(seed)


def decode_point(b: bytes):
    """RFC 8032's decoding (string_to_point): the point, or None where the bytes do not decode or are not the canonical encoding --
    ed25519_ClassifyKey's DECODES and CANONICAL"""
    A, y, sign = key_model.decode(b)
    if A is None or y >= P or (A[0] == 0 and sign == 1):
        return None
    return A


@functools.lru_cache(maxsize=None)
def hash_point(pk_string: bytes, alpha: bytes):
    """H = ECVRF_encode_to_curve_h2c_suite(encode_to_curve_salt = PK_string, alpha_string) (5.4.1.2)"""
    return h2c_model.encode_to_curve_point(pk_string + alpha, DST)


def challenge(*points) -> int:
    """ECVRF_challenge_generation (5.4.3) over the five encoded points"""
    return int.from_bytes(hashlib.sha512(SUITE + b"\x02" + b"".join(points) + b"\x00").digest()[:C_LEN], "little")


def nonce(prefix: bytes, h_string: bytes) -> int:
    """ECVRF_nonce_generation_RFC8032 (5.4.2.2)"""
    return int.from_bytes(hashlib.sha512(prefix + h_string).digest(), "little") % L


def prove_parts(priv: bytes, alpha: bytes):
    """every value of ECVRF_prove (5.1) for a 64-byte private key whose second half is read as given"""
    seed, y_string = priv[:32], priv[32:]
    x, prefix = secret_scalar(seed)
    H = hash_point(y_string, alpha)
    h_string = ed_enc(H)
    gamma = _mul(x, H)
    k = nonce(prefix, h_string)
    U, V = _mul(k, ED_B), _mul(k, H)
    c = challenge(y_string, h_string, ed_enc(gamma), ed_enc(U), ed_enc(V))
    s = (k + c * x) % L
    return dict(x=x, k=k, c=c, s=s, H=h_string, Gamma=ed_enc(gamma), U=ed_enc(U), V=ed_enc(V),
                pi=ed_enc(gamma) + _le(c, C_LEN) + _le(s))


@functools.lru_cache(maxsize=None)
def prove(priv: bytes, alpha: bytes) -> bytes:
    return prove_parts(priv, alpha)["pi"]


def decode_proof(pi: bytes):
    """(Gamma, c, s) of ECVRF_decode_proof (5.4.4), or None"""
    gamma = decode_point(pi[:32])
    s = int.from_bytes(pi[48:80], "little")
    if gamma is None or s >= L:
        return None
    return gamma, int.from_bytes(pi[32:48], "little"), s


def _beta(gamma) -> bytes:
    return hashlib.sha512(SUITE + b"\x03" + ed_enc(_mul(8, gamma)) + b"\x00").digest()


@functools.lru_cache(maxsize=None)
def proof_to_hash(pi: bytes):
    """(beta, ok) of ed25519_VRF_ProofToHash for one proof (5.2)"""
    d = decode_proof(pi)
    return (ZERO_BETA, 0) if d is None else (_beta(d[0]), 1)


@functools.lru_cache(maxsize=None)
def verify(pk: bytes, pi: bytes, alpha: bytes, validate_key: bool = True):
    """(beta, ok) of ECVRF_verify (5.3); the calls run it with validate_key = TRUE"""
    Y = decode_point(pk)
    if Y is None or (validate_key and _mul(8, Y) == NEUTRAL):
        return ZERO_BETA, 0
    d = decode_proof(pi)
    if d is None:
        return ZERO_BETA, 0
    gamma, c, s = d
    H = hash_point(pk, alpha)
    U = ed_add(_mul(s, ED_B), _neg(_mul(c, Y)))
    V = ed_add(_mul(s, H), _neg(_mul(c, gamma)))
    if challenge(pk, ed_enc(H), pi[:32], ed_enc(U), ed_enc(V)) != c:
        return ZERO_BETA, 0
    return _beta(gamma), 1


# ---- the case set ----------------------------------------------------------------------------------------------------------
def _bytes(n: int, tag: str) -> bytes:
    out = b""
    i = 0
    while len(out) < n:
        out += hashlib.sha512(f"vrf case {tag} {i}".encode()).digest()
        i += 1
    return out[:n]


def _rows(rows, width):
    if not rows:
        return np.zeros((0, width), np.uint8)
    return np.stack([np.frombuffer(bytes(r), np.uint8) for r in rows]).reshape(len(rows), width).copy()


def _frozen(**arrays):
    for a in arrays.values():
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def honest(alpha_len: int):
    """ROWS_PER_LENGTH honest rows at one alpha length: priv [n, 64], pk [n, 32], alpha [n, alpha_len], pi [n, 80], beta [n, 64]
    (read-only)"""
    privs = [private_key(_bytes(32, f"seed {alpha_len} {j}")) for j in range(ROWS_PER_LENGTH)]
    alphas = [_bytes(alpha_len, f"alpha {alpha_len} {j}") for j in range(ROWS_PER_LENGTH)]
    pis = [prove(p, a) for p, a in zip(privs, alphas)]
    return _frozen(priv=_rows(privs, 64), pk=_rows([p[32:] for p in privs], 32), alpha=_rows(alphas, alpha_len),
                   pi=_rows(pis, PROOF_SIZE), beta=_rows([proof_to_hash(pi)[0] for pi in pis], OUTPUT_SIZE))


def small_order_keys():
    """the canonical encodings of the eight points of small order, with the order of each"""
    T8 = ed_order8_point()
    out = []
    for j in range(8):
        A = _mul(j, T8)
        order = next(m for m in (1, 2, 4, 8) if _mul(m, A) == NEUTRAL)
        out.append((ed_enc(A), order))
    return out


@functools.lru_cache(maxsize=None)
def crafted_small_order_proof(pk: bytes, order: int, alpha: bytes) -> bytes:
    """a proof that satisfies both of ECVRF_verify's equations under a key of small order: Gamma = O, U = [k]B, V = [k]H, s = k,
    with k counted up until c is a multiple of the key's order ([c]Y = O, [c]Gamma = O: U = [s]B - [c]Y, V = [s]H - [c]Gamma).
    Only validate_key rejects it."""
    H = hash_point(pk, alpha)
    k = int.from_bytes(_bytes(32, "small order nonce"), "little") % L
    while True:
        c = challenge(pk, ed_enc(H), ed_enc(NEUTRAL), ed_enc(_mul(k, ED_B)), ed_enc(_mul(k, H)))
        if c % order == 0:
            return ed_enc(NEUTRAL) + _le(c, C_LEN) + _le(k)
        k += 1


@functools.lru_cache(maxsize=None)
def mixed_order_rows(alpha: bytes):
    """two private keys whose public half is [x]B + T8 (of order 8 L: flags DECODES | CANONICAL), each with the honest proof under
    its scalar: [s]B - [c]Y = U - [c]T8, so the first (c a multiple of 8) verifies and the second (c odd) does not.  The seeds
    are counted up until c falls that way."""
    T8 = ed_order8_point()
    want, out, j = [lambda c: c % 8 == 0, lambda c: c % 2 == 1], [], 0
    while want:
        seed = _bytes(32, f"mixed order seed {j}")
        j += 1
        priv = seed + ed_enc(ed_add(_mul(secret_scalar(seed)[0], ED_B), T8))
        if want[0](prove_parts(priv, alpha)["c"]):
            out.append(priv)
            want.pop(0)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rejections():
    """The verification rows at alpha length REJECT_ALPHA, each derived from an honest row: pk [n, 32], pi [n, 80], alpha [n, 9], and
    the model's ok [n] and beta [n, 64] for Verify, ok_hash [n] and beta_hash [n, 64] for ProofToHash, with labels (read-only)."""
    h = honest(REJECT_ALPHA)
    pk, pi, alpha = h["pk"][0].tobytes(), h["pi"][0].tobytes(), h["alpha"][0].tobytes()
    other_pk = h["pk"][1].tobytes()
    rows = [("honest", pk, pi, alpha), ("honest, second key", other_pk, h["pi"][1].tobytes(), h["alpha"][1].tobytes())]

    def flip(b, bit):
        v = bytearray(b)
        v[bit // 8] ^= 1 << (bit % 8)
        return bytes(v)

    rows.append(("a bit of Gamma flipped", pk, flip(pi, 8 * 5 + 3), alpha))
    rows.append(("a bit of c flipped", pk, flip(pi, 8 * 32 + 1), alpha))
    rows.append(("the top bit of c flipped", pk, flip(pi, 8 * 47 + 7), alpha))
    rows.append(("a bit of s flipped", pk, flip(pi, 8 * 48), alpha))
    s = int.from_bytes(pi[48:], "little")
    rows.append(("s + L", pk, pi[:48] + _le(s + L), alpha))
    rows.append(("s = L", pk, pi[:48] + _le(L), alpha))
    rows.append(("s with bit 255", pk, pi[:48] + _le(s | 1 << 255), alpha))
    for y in key_model.off_curve_y(2):
        rows.append(("Gamma off the curve", pk, _le(y) + pi[32:], alpha))
    rows.append(("Gamma not canonical: y = p + 1", pk, _le(P + 1) + pi[32:], alpha))
    rows.append(("Gamma not canonical: y = p", pk, _le(P) + pi[32:], alpha))
    rows.append(("Gamma not canonical: x = 0 with the sign bit", pk, _le(1 | 1 << 255) + pi[32:], alpha))
    rows.append(("Gamma negated", pk, pi[:31] + bytes([pi[31] ^ 0x80]) + pi[32:], alpha))
    rows.append(("the wrong alpha", pk, pi, flip(alpha, 17)))
    rows.append(("the wrong key", other_pk, pi, alpha))
    rows.append(("the key off the curve", _le(key_model.off_curve_y(2)[0]), pi, alpha))
    rows.append(("the key not canonical", _le(P + 1), pi, alpha))
    for key, order in small_order_keys():
        rows.append((f"a key of order {order} and a proof crafted for it", key, crafted_small_order_proof(key, order, alpha), alpha))
    good, bad = mixed_order_rows(alpha)
    rows.append(("a key of mixed order, c a multiple of 8", good[32:], prove(good, alpha), alpha))
    rows.append(("a key of mixed order, c odd", bad[32:], prove(bad, alpha), alpha))
    ver = [verify(k, p, a) for _, k, p, a in rows]
    pth = [proof_to_hash(p) for _, _, p, _ in rows]
    out = _frozen(pk=_rows([r[1] for r in rows], 32), pi=_rows([r[2] for r in rows], PROOF_SIZE), alpha=_rows([r[3] for r in rows], REJECT_ALPHA),
                  ok=np.array([v[1] for v in ver], np.int32), beta=_rows([v[0] for v in ver], OUTPUT_SIZE),
                  ok_hash=np.array([v[1] for v in pth], np.int32), beta_hash=_rows([v[0] for v in pth], OUTPUT_SIZE))
    out["labels"] = tuple(r[0] for r in rows)
    return out


def mixed_order_privs():
    """priv [2, 64] of mixed_order_rows at the rejection rows' alpha, with that alpha [2, 9] and the proofs [2, 80]: Prove reads the
    public half as given"""
    alpha = honest(REJECT_ALPHA)["alpha"][0].tobytes()
    privs = mixed_order_rows(alpha)
    return _rows(privs, 64), _rows([alpha] * 2, REJECT_ALPHA), _rows([prove(p, alpha) for p in privs], PROOF_SIZE)


def example_rows():
    """the RFC's three examples as (priv [64], pk, alpha, pi, beta) bytes"""
    out = []
    for e in EXAMPLES:
        sk, pk = bytes.fromhex(e["sk"]), bytes.fromhex(e["pk"])
        out.append((sk + pk, pk, bytes.fromhex(e["alpha"]), bytes.fromhex(e["pi"]), bytes.fromhex(e["beta"])))
    return out

"""Adversarial unit-test inputs shared by the CPU (host-emulated device source) and GPU suites, with the expected
results computed by Python big integers.  The cases follow the reference's own unit checks
(test/curve25519_selftest.c:624-741): field identities mod p, and mod-L reductions around the n*L +- 1 and
b*R +- 1 boundaries where eco_ReduceHiWord / eco_Mod take their borrow paths."""
import functools

import numpy as np

from curve25519_amd import synth

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
R = (1 << 256) % L                      # 2^256 mod L
MINUS_R = (1 << 256) - 16 * (L - 2**252)  # what one top-word fold subtracts per unit: 2^256 - 16c ... see sc25519.cuh


def le(x: int, nbytes: int) -> np.ndarray:
    return np.frombuffer(int(x).to_bytes(nbytes, "little"), np.uint8)


def field_cases():
    """(pairs, a[n,32], b[n,32]) of 256-bit patterns: every special value against every other, plus seeded random."""
    special = [0, 1, 2, 19, 38, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 2**255 - 1, 2**255, 2**256 - 1,
               2**256 - 38, 2**256 - 39, 2**26 - 1, 2**26, 2**51 - 1, 2**51, (1 << 255) - 20,
               int("3ffffff" * 9 + "ff", 16) % 2**256, int("aa" * 32, 16), int("55" * 32, 16),
               121665, 121666, pow(2, (P - 1) // 4, P)]
    rnd = synth.random_bytes((400, 32), 0xFE01)
    vals = special + [int.from_bytes(r.tobytes(), "little") for r in rnd]
    pairs = [(a, b) for a in special for b in special] + list(zip(vals, reversed(vals)))
    a = np.stack([le(x, 32) for x, _ in pairs])
    b = np.stack([le(y, 32) for _, y in pairs])
    return pairs, a, b


FIELD_OPS = {
    0: lambda x, y: x * y, 1: lambda x, y: x * x, 2: lambda x, y: x + y, 3: lambda x, y: x - y,
    4: lambda x, y: pow(x, P - 2, P), 5: lambda x, y: pow(x, (P - 5) // 8, P), 6: lambda x, y: x,
    7: lambda x, y: (x - y) * (x + y), 8: lambda x, y: x * x - y, 9: lambda x, y: 2 * x * x + x,
    10: lambda x, y: x + 121665 * y, 11: lambda x, y: 9 * x,
    12: lambda x, y: pow(x, P - 2, P), 13: lambda x, y: pow(x, P - 2, P), 14: lambda x, y: pow(x, P - 2, P),
}
# ops 8 and 9 take a reduced second operand (the contract of fe_sqr_sub / fe_sqr2_add_sub)
FIELD_OPS_B_REDUCED = {8, 9}


def inversion_cases():
    """256-bit patterns for the inversions (op 4: what the kernels run, 12: the reference's exponentiation, 13: division steps, 14: division steps on a quad of lanes):
    every power of two and its neighbours, the same below p, below 2p and below 2^256 (non-canonical inputs are reduced first),
    small values, values of the form (p +- 1) / 2^k, seeded random.  The division steps' path depends on the bit patterns of p and
    the input (runs of zeros, of ones, values whose quotient sequence is long), so this is wider than field_cases()."""
    vals = set(range(0, 40))
    for k in range(0, 256):
        for d in (-1, 0, 1):
            for base in (0, P, 2 * P, 2**256):
                for sgn in (1, -1):
                    v = base + sgn * (1 << k) + d
                    if 0 <= v < 2**256:
                        vals.add(v)
    for k in range(1, 64):
        vals.add(((P + 1) >> 1) * pow(2, -k + 1, P) % P)
        vals.add((P - 1) // 2 >> k)
        vals.add(pow(3, k * 5, P))
        vals.add(P - pow(3, k * 7, P))
    vals = sorted(vals)
    rnd = synth.random_bytes((700, 32), 0xFE02)
    vals += [int.from_bytes(r.tobytes(), "little") for r in rnd]
    pairs = [(v, 0) for v in vals]
    a = np.stack([le(x, 32) for x, _ in pairs])
    return pairs, a, np.zeros_like(a)


def scalar_cases():
    """(a512 ints, b256 ints, a[n,64], b[n,32]): values that force the borrow / add-back paths of the mod-L code."""
    a512, b256 = [], []
    edge256 = [0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 15 * L - 1, 15 * L, 15 * L + 1, 2**252 - 1, 2**252,
               2**252 + 1, 2**253 - 1, 2**255 - 1, 2**255, 2**256 - 1, R - 1, R, R + 1, 2**256 - R, 16 * (L - 2**252),
               16 * (L - 2**252) - 1, 16 * (L - 2**252) + 1]
    for n in range(0, 16):
        for d in (-1, 0, 1):
            v = n * L + d
            if 0 <= v < 2**256:
                edge256.append(v)
    for k in (1, 2, 3, 7, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff):
        for d in (-1, 0, 1):
            edge256.append((k * R + d) % 2**256)
            edge256.append((k * 16 * (L - 2**252) + d) % 2**256)
    edge256 = sorted(set(edge256))
    hi_words = [0, 1, 2, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff]
    for lo in edge256:
        for hi in hi_words:
            a512.append(lo + (hi << 256))
            b256.append(edge256[(len(a512) * 7) % len(edge256)])
    # full 512-bit patterns: all-ones, multiples of L near 2^512, digests
    big = [2**512 - 1, 2**512 - L, (2**512 // L) * L, (2**512 // L) * L - 1, (2**512 // L) * L + 1, 2**511, 2**256,
           2**256 - 1, (2**256 - 1) << 256]
    for k in range(1, 40):
        big.append(((2**512 // L) - k) * L + (k % 3) - 1)
    for v in big:
        a512.append(v % 2**512)
        b256.append(edge256[(v % 9973) % len(edge256)])
    rnd = synth.random_bytes((600, 96), 0x5C01)
    for r in rnd:
        a512.append(int.from_bytes(r[:64].tobytes(), "little"))
        b256.append(int.from_bytes(r[64:].tobytes(), "little"))
    a = np.stack([le(x, 64) for x in a512])
    b = np.stack([le(y, 32) for y in b256])
    return a512, b256, a, b


M256 = 2**256 - 1
# op -> (expected exact value, canonical?)   see include/curve25519_amd.h c25519_amd_sc_selftest
SCALAR_OPS = {
    0: (lambda a, b: a, True),
    1: (lambda a, b: a, False),
    2: (lambda a, b: a & M256, True),
    3: (lambda a, b: (a & M256) * b, False),
    4: (lambda a, b: (a & M256) + b, False),
    5: (lambda a, b: (a & M256) + (((a >> 256) & 0xffffffff) << 256), False),
    6: (lambda a, b: (a & M256) * b + (a >> 256), True),
}


def check_scalar(op, out, a512, b256):
    f, canonical = SCALAR_OPS[op]
    for i, (x, y) in enumerate(zip(a512, b256)):
        got = int.from_bytes(out[i].tobytes(), "little")
        exp = f(x, y) % L
        if canonical:
            assert got == exp, (op, i, hex(x), hex(y), hex(got), hex(exp))
        else:
            assert got % L == exp and got < 2**256, (op, i, hex(x), hex(y), hex(got))


def check_field(op, out, pairs):
    f = FIELD_OPS[op]
    for i, (x, y) in enumerate(pairs):
        got = int.from_bytes(out[i].tobytes(), "little")
        if op in FIELD_OPS_B_REDUCED:
            y %= P
        assert got == f(x, y) % P, (op, hex(x), hex(y), hex(got))


# ---- Ed25519 verification corner cases (for the lattice fast path, curve25519_amd/csrc/verify_fast.cuh) -----------------
# A tiny affine Edwards implementation, only to BUILD inputs: keys and R's with torsion components, small-order keys.
# Expected verdicts always come from the oracle / the reference, never from here.
D_ED = (-121665 * pow(121666, P - 2, P)) % P
N8L = 8 * L


def ed_add(p, q):
    x1, y1 = p
    x2, y2 = q
    k = D_ED * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + k, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - k, P - 2, P) % P)


def ed_mul(k, p):
    r = (0, 1)
    while k:
        if k & 1:
            r = ed_add(r, p)
        p = ed_add(p, p)
        k >>= 1
    return r


def ed_enc(p):
    return (p[1] | ((p[0] & 1) << 255)).to_bytes(32, "little")


@functools.lru_cache(maxsize=1024)       # (a model that decodes one key for every row of a set pays for the square root once)
def ed_decode(y, sign):
    u, v = (y * y - 1) % P, (D_ED * y * y + 1) % P
    x = pow(u * pow(v, P - 2, P) % P, (P + 3) // 8, P)
    if (x * x * v - u) % P:
        x = x * pow(2, (P - 1) // 4, P) % P
    if (x * x * v - u) % P:
        return None
    return (P - x if (x & 1) != sign else x, y)


ED_B = ed_decode(4 * pow(5, P - 2, P) % P, 0)


def ed_order8_point():
    y = 2
    while True:
        pt = ed_decode(y, 0)
        y += 1
        if pt is None:
            continue
        t = ed_mul(L, pt)
        if ed_mul(4, t) != (0, 1):
            return t


def torsion_signature_cases(count=15, seed=9):
    """(sig[n,64], pk[n,32], msg[n,32]): keys A = a*B + t*T8 with a torsion component and, for each, the eight
    signatures (r*B + j*T8, r + h*a): exactly those with j + h*t = 0 mod 8 satisfy the cofactorless equation the
    reference checks; a cofactored check would accept all eight."""
    import hashlib
    import random
    rnd = random.Random(seed)
    T8 = ed_order8_point()
    sigs, pks, msgs = [], [], []
    for _ in range(count):
        a, t = rnd.getrandbits(252) % L, rnd.choice([1, 2, 3, 4, 5, 6, 7])
        pk = ed_enc(ed_add(ed_mul(a, ED_B), ed_mul(t, T8)))
        m = rnd.getrandbits(256).to_bytes(32, "little")
        r = rnd.getrandbits(252) % L
        for j in range(8):
            Rb = ed_enc(ed_add(ed_mul(r, ED_B), ed_mul(j, T8)))
            h = int.from_bytes(hashlib.sha512(Rb + pk + m).digest(), "little") % L
            sigs.append(Rb + ((r + h * a) % L).to_bytes(32, "little"))
            pks.append(pk)
            msgs.append(m)
    f = lambda rows: np.stack([np.frombuffer(x, np.uint8) for x in rows])  # noqa: E731
    return f(sigs), f(pks), f(msgs)


def small_order_keys():
    T8 = ed_order8_point()
    return np.stack([np.frombuffer(ed_enc(ed_mul(k, T8)), np.uint8) for k in range(8)])


def special_r_encodings():
    """R byte strings an encoder never produces or that are special points: x = 0 with the sign bit, y >= p, the
    neutral element, (0, -1), all-ones."""
    vals = [1 | (1 << 255), P + 1, 1, P - 1, 2**255 - 1, 2**256 - 1, P, 0, (P - 1) | (1 << 255)]
    return np.stack([le(v, 32) for v in vals])


def lattice_inputs():
    import random
    rnd = random.Random(7)
    hs = [0, 1, 2, 3, L - 1, L - 2, 2**128, 2**128 - 1, 2**127, 2**252, (L - 1) // 2, 2**129 + 1]
    hs += [rnd.getrandbits(253) % L for _ in range(6000)]
    hs += [rnd.getrandbits(k) for k in range(1, 253)]
    hs += [(N8L * a // b) % L for a in range(1, 20) for b in range(a + 1, 21)]
    return hs


def small_order_encodings():
    """Every 32-byte string the reference decodes to one of the eight small-order points: the canonical encodings, x = 0
    with the sign bit set, and y + p where that still fits 255 bits (y = 0, 1), with either sign bit.  [(bytes, k)] with
    the point being k * T8."""
    T8 = ed_order8_point()
    out = []
    for k in range(8):
        x, y = ed_mul(k, T8)
        encs = [y | ((x & 1) << 255)]
        if x == 0:
            encs.append(y | (1 << 255))
        if y + P < 2**255:
            encs.append((y + P) | ((x & 1) << 255))
            if x == 0:
                encs.append((y + P) | (1 << 255))
        out += [(e.to_bytes(32, "little"), k) for e in encs]
    return out


def degenerate_signature_cases():
    """Inputs (sig[n,64], pk[n,32], msg[n,8], label[n]) on which a verifier that validates its inputs and the reference --
    which does not (ed25519_verify.c:179-197, :287-313: no key / R validation, S taken as a 256-bit integer, byte compare
    of enc(T) with R) -- may differ: small-order keys in every encoding the reference decodes, R a small-order point in
    every encoding, S in {0, L, 2L, 15L, 1}, the message searched so that the group equation S*B = R + h*A holds (and
    one where it does not); and mixed-order keys a*B + t*T8 with small-order R and S = h*a, S + L.  Expected verdicts
    are the REFERENCE's (tests/golden/degenerate_verify.npz, written by gen_golden.py); nothing here decides them."""
    import hashlib
    T8 = ed_order8_point()
    encs = small_order_encodings()
    sigs, pks, msgs, labels = [], [], [], []

    def hash_mod_l(Rb, Ab, m):
        return int.from_bytes(hashlib.sha512(Rb + Ab + m).digest(), "little") % L

    def find_msg(Rb, Ab, want, tag):
        """first 8-byte counter message for which want(h) holds (None after 256 tries: unsolvable residue)"""
        for c in range(256):
            m = (tag * 65536 + c).to_bytes(8, "little")
            if want(hash_mod_l(Rb, Ab, m)):
                return m
        return None

    def put(Rb, S, Ab, m, label):
        sigs.append(Rb + S.to_bytes(32, "little"))
        pks.append(Ab)
        msgs.append(m)
        labels.append(label)

    tag = 0
    for Ab, a in encs:
        for Rb, r in encs:
            tag += 1
            # the reference checks S*B + h*(-A) == R: with S = 0 mod L that is h*a + r = 0 mod 8 for A = a*T8, R = r*T8
            sat = find_msg(Rb, Ab, lambda h: (h * a + r) % 8 == 0, tag)
            unsat = find_msg(Rb, Ab, lambda h: (h * a + r) % 8 != 0, tag)
            if sat is not None:
                for S in (0, L, 2 * L, 15 * L):
                    put(Rb, S, Ab, sat, 0)
            if unsat is not None:
                put(Rb, 0, Ab, unsat, 1)
            if r == 0 or a == 0:
                put(Rb, 1, Ab, sat if sat is not None else unsat, 2)         # S = 1: never a torsion point
    import random
    rnd = random.Random(11)
    for t in range(1, 8):
        a = rnd.getrandbits(252) % L
        Ab = ed_enc(ed_add(ed_mul(a, ED_B), ed_mul(t, T8)))
        for j in range(8):
            tag += 1
            Rb = ed_enc(ed_mul(j, T8))
            # S*B = R + h*A with R = j*T8, A = a*B + t*T8:  S = h*a mod L and j + h*t = 0 mod 8
            # (the reference negates A when it decodes it: the sign convention is settled by its verdicts, both residues go in)
            for sign, lab in ((1, 3), (-1, 4)):
                m = find_msg(Rb, Ab, lambda h: (j + sign * h * t) % 8 == 0, tag)
                if m is None:
                    continue
                h = hash_mod_l(Rb, Ab, m)
                for S in ((h * a) % L, (h * a) % L + L, (-h * a) % L):
                    put(Rb, S, Ab, m, lab)
    f = lambda rows: np.stack([np.frombuffer(x, np.uint8) for x in rows])  # noqa: E731
    return f(sigs), f(pks), f(msgs), np.array(labels, np.int32)


def reference_differential(engine):
    """The seeded inputs of test_oracle_golden.test_against_reference_build through `engine` (the oracle, or the real
    reference, whose outputs tests/golden/reference_diff.npz holds): X25519 shared keys (2^256-1 peer keys included) and
    public keys, Ed25519 key pairs, signatures of 0..200-byte messages, verdicts on corrupted signatures and on unvalidated
    garbage, the 8-fold base table and Verify_Init tables (reduced mod p, 32 little-endian bytes per value).
    Returns {name: uint8 / int32 array}."""
    n = 384
    sk = synth.random_bytes((n, 32), 0xD1FF01)
    pk = synth.random_bytes((n, 32), 0xD1FF02)
    pk[:8] = 0xff                                   # 2^256-1 rows
    out = {}
    out["x_shared"], out["x_sk_clamped"] = engine.x25519_shared(pk, sk)
    for fast in (False, True):
        out["x_public" + ("_fast" if fast else "")] = engine.x25519_public(sk, fast=fast)[0]
    pub, priv = engine.ed25519_keypair(sk)
    out["ed_pub"], out["ed_priv"] = pub, priv
    for mlen in (0, 1, 32, 100, 200):
        msg = synth.random_bytes((n, mlen), 0xD1FF03 + mlen)
        sig = engine.ed25519_sign(priv, msg)
        out[f"ed_sig_{mlen}"] = sig
        bad = sig.copy()
        bad[::3, 7] ^= 4
        out[f"ed_verify_{mlen}"] = np.asarray(engine.ed25519_verify(bad, pub, msg), np.int32)
    # garbage keys and signatures: no validation anywhere, verdicts must still agree
    gs, gp = synth.random_bytes((n, 64), 11), synth.random_bytes((n, 32), 12)
    msg = synth.random_bytes((n, 32), 13)
    out["garbage_verify"] = np.asarray(engine.ed25519_verify(gs, gp, msg), np.int32)
    out["base_table"] = engine.base_table()
    # Verify_Init tables, valid keys and unvalidated garbage (off-curve "points": the values then depend on the
    # exact order of doublings / additions, so this pins the operation sequence, not just the group element)
    keys = np.concatenate([pub[:6], gp[:10], np.zeros((1, 32), np.uint8), np.full((1, 32), 0xff, np.uint8)])
    out["verify_init_table"] = np.array([[[le(v, 32) for v in row] for row in tab] for tab in engine.verify_init_table(keys)],
                                        np.uint8)
    return {k: np.asarray(v) for k, v in out.items()}

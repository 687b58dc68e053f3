"""RFC 9497's OPRF (mode 0x00) and VOPRF (mode 0x01) for ristretto255-SHA512 as ristretto255_OPRF_Blind_*, ristretto255_OPRF_Finalize_*,
ristretto255_OPRF_BlindEvaluate_*, ristretto255_VOPRF_BlindEvaluate_* and ristretto255_VOPRF_VerifyProof_* state them
(include/curve25519_amd.h), in Python big integers and in the RFC's order (2.2.1 GenerateProof with ComputeCompositesFast, 2.2.2
VerifyProof with ComputeComposites, 3.3.1, 3.3.2), and the case set the CPU and GPU tests of those calls share.  Built on
tests/h2c_model.py (expand_message_xmd, HashToGroup, HashToScalar), tests/ristretto_model.py (DECODE, ENCODE) and tests/group_model.py's
mul; tests/test_oprf_model.py pins it to the published vectors.  A walk costs ~2 ms: the rows are multiples [a]B of the generator for
a few dozen known a, memoised, so that a request's composite is ONE multiplication, M = [sum a_i d_i]B."""
import functools
import hashlib

import numpy as np

import group_model
import h2c_model
import ristretto_model
from vectors import ED_B, L, ed_add

ZERO32, ZERO64 = bytes(32), bytes(64)
MAX_ROWS = 65535                                     # of one proof: the row index is I2OSP(i, 2)
NO_OWNER = -1
IDENTITY = (0, 1)


def ctx(mode: int) -> bytes:
    return h2c_model.oprf_context_string(mode)


def _le(v: int, n: int = 32) -> bytes:
    return int(v).to_bytes(n, "little")


def _int(b: bytes) -> int:
    return int.from_bytes(b, "little")


def _lp(b: bytes) -> bytes:
    return len(b).to_bytes(2, "big") + b


@functools.lru_cache(maxsize=None)
def _mul(k: int, A):
    return group_model.mul(k, A)


@functools.lru_cache(maxsize=None)
def _enc(A) -> bytes:
    return ristretto_model.encode(A)


@functools.lru_cache(maxsize=None)
def _dec(b: bytes):
    return ristretto_model.decode(b)


def base_mult(k: int) -> bytes:
    return _enc(_mul(k % L, ED_B))


def hash_to_scalar(msg: bytes, mode: int = 1) -> int:
    return _int(h2c_model.hash_to_scalar(msg, b"HashToScalar-" + ctx(mode)))


# ---- the calls, one row ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blind(inp: bytes, blind_bytes: bytes, mode: int):
    """(blinded, ok): blind read as 256 bits mod L; ok = 0 and zeros where the result is the identity"""
    element = _dec(h2c_model.oprf_hash_to_group(inp, mode))
    out = _enc(_mul(_int(blind_bytes) % L, element))
    return (out, 1) if any(out) else (ZERO32, 0)


@functools.lru_cache(maxsize=None)
def finalize(inp: bytes, blind_bytes: bytes, evaluated: bytes):
    """(output, ok, why)"""
    Z = _dec(evaluated)
    b = _int(blind_bytes) % L
    if Z is None:
        return ZERO64, 0, "evaluated does not decode"
    if not any(evaluated):
        return ZERO64, 0, "evaluated is the identity"
    if b == 0:
        return ZERO64, 0, "blind is zero"
    n = _enc(_mul(pow(b, L - 2, L), Z))
    return hashlib.sha512(_lp(inp) + _lp(n) + b"Finalize").digest(), 1, "valid"


@functools.lru_cache(maxsize=None)
def evaluate_row(sks: bytes, blinded: bytes):
    """(evaluated, ok, why) of one row under the key: skS read as 256 bits mod L"""
    C = _dec(blinded)
    if C is None:
        return ZERO32, 0, "row does not decode"
    if not any(blinded):
        return ZERO32, 0, "row is the identity"
    out = _enc(_mul(_int(sks) % L, C))
    return (out, 1, "valid") if any(out) else (ZERO32, 0, "result is the identity")


# ---- the proof (RFC 9497 section 2.2) --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def composite_seed(pks: bytes) -> bytes:
    return hashlib.sha512(_lp(pks) + _lp(b"Seed-" + ctx(1))).digest()


def composite_scalar(seed: bytes, i: int, c_i: bytes, d_i: bytes) -> int:
    return hash_to_scalar(_lp(seed) + i.to_bytes(2, "big") + _lp(c_i) + _lp(d_i) + b"Composite")


def _sum(points):
    acc = IDENTITY
    for Q in points:
        acc = ed_add(acc, Q)
    return acc


def composites(pks: bytes, cs, ds, logs=None, sk=None):
    """(M, Z) as points.  logs: the known a_i with C_i = [a_i]B (then M = [sum a_i d_i]B, one multiplication); sk: the key (then
    Z = [sk]M, ComputeCompositesFast)"""
    seed = composite_seed(pks)
    di = [composite_scalar(seed, i, c, d) for i, (c, d) in enumerate(zip(cs, ds))]
    if logs is not None:
        M = _mul(sum(a * d for a, d in zip(logs, di)) % L, ED_B)
    else:
        M = _sum(_mul(d, _dec(c)) for d, c in zip(di, cs))
    if sk is not None:
        Z = _mul(sk, M)
    else:
        Z = _sum(_mul(d, _dec(e)) for d, e in zip(di, ds))
    return M, Z


def challenge(pks: bytes, M, Z, t2, t3) -> int:
    return hash_to_scalar(_lp(pks) + b"".join(_lp(_enc(A)) for A in (M, Z, t2, t3)) + b"Challenge")


def generate_proof(sk: int, pks: bytes, cs, ds, r: int, logs=None) -> bytes:
    M, Z = composites(pks, cs, ds, logs, sk)
    t2 = _mul(r, ED_B)
    t3 = _mul(r, M)
    c = challenge(pks, M, Z, t2, t3)
    return _le(c) + _le((r - c * sk) % L)


def verify_proof(pks: bytes, cs, ds, proof: bytes, logs=None, dlogs=None) -> int:
    """1 iff the proof holds for rows that decode and are not the identity (the caller has checked them)"""
    c, s = _int(proof[:32]), _int(proof[32:])
    Y = _dec(pks)
    if c >= L or s >= L or Y is None or not any(pks):
        return 0
    seed = composite_seed(pks)
    di = [composite_scalar(seed, i, a, b) for i, (a, b) in enumerate(zip(cs, ds))]
    if logs is not None and dlogs is not None:
        M = _mul(sum(a * d for a, d in zip(logs, di)) % L, ED_B)
        Z = _mul(sum(a * d for a, d in zip(dlogs, di)) % L, ED_B)
    else:
        M = _sum(_mul(d, _dec(a)) for d, a in zip(di, cs))
        Z = _sum(_mul(d, _dec(b)) for d, b in zip(di, ds))
    t2 = ed_add(_mul(s, ED_B), _mul(c, Y))
    t3 = ed_add(_mul(s, M), _mul(c, Z))
    return 1 if challenge(pks, M, Z, t2, t3) == c else 0


# ---- the batched calls -----------------------------------------------------------------------------------------------------------
def owners(offsets, m: int, n: int):
    """the request that owns each row, as the device finds it: a bisection over offsets[1 .. m] for the first request that ends
    behind the row, kept where that request is well formed (1 .. 65 535 rows inside [0, n]) and holds the row.  For offsets that
    rise from 0 to n this is the request the row lies in; for any other array it is still one definite answer."""
    off = [int(x) for x in offsets]
    out = []
    for i in range(n):
        lo, hi = 0, m
        while lo < hi:
            mid = (lo + hi) // 2
            if off[mid + 1] <= i:
                lo = mid + 1
            else:
                hi = mid
        j = lo
        good = j < m and request_well_formed(off, j, n) and off[j] <= i < off[j + 1]
        out.append(j if good else NO_OWNER)
    return out


def request_well_formed(off, j: int, n: int) -> bool:
    return off[j] < off[j + 1] and off[j + 1] - off[j] <= MAX_ROWS and off[j + 1] <= n


def oprf_blind_evaluate(sks: bytes, blinded):
    rows = [evaluate_row(sks, bytes(b)) for b in blinded]
    return [r[0] for r in rows], [r[1] for r in rows]


def voprf_blind_evaluate(sks: bytes, proof_rand, blinded, offsets, logs=None):
    """(evaluated, proofs, ok, req_ok) of ristretto255_VOPRF_BlindEvaluate for m = len(proof_rand) requests over n = len(blinded) rows;
    logs: the rows' known discrete logarithms (None where not known), for the shortcut of composites()"""
    m, n = len(proof_rand), len(blinded)
    off = [int(x) for x in offsets]
    sk = _int(sks) % L
    pks = base_mult(sk)
    own = owners(off, m, n)
    evaluated, ok = [ZERO32] * n, [0] * n
    for i in range(n):
        if own[i] != NO_OWNER:
            evaluated[i], ok[i], _ = evaluate_row(sks, bytes(blinded[i]))
    proofs, req_ok = [ZERO64] * m, [0] * m
    for j in range(m):
        r = _int(bytes(proof_rand[j])) % L
        if not request_well_formed(off, j, n) or r == 0 or sk == 0:
            continue
        rows = range(off[j], off[j + 1])
        if any(own[i] != j or not ok[i] for i in rows):
            continue
        lg = None if logs is None or any(logs[i] is None for i in rows) else [logs[i] for i in rows]
        proofs[j] = generate_proof(sk, pks, [bytes(blinded[i]) for i in rows], [evaluated[i] for i in rows], r, lg)
        req_ok[j] = 1
    return evaluated, proofs, ok, req_ok


def voprf_verify(pks: bytes, blinded, evaluated, proofs, offsets, logs=None, dlogs=None):
    """req_ok of ristretto255_VOPRF_VerifyProof"""
    m, n = len(proofs), len(blinded)
    off = [int(x) for x in offsets]
    own = owners(off, m, n)

    def row_ok(i):
        return all(_dec(bytes(a[i])) is not None and any(bytes(a[i])) for a in (blinded, evaluated))
    req_ok = [0] * m
    for j in range(m):
        if not request_well_formed(off, j, n):
            continue
        rows = range(off[j], off[j + 1])
        if any(own[i] != j or not row_ok(i) for i in rows):
            continue
        known = logs is not None and dlogs is not None and all(logs[i] is not None and dlogs[i] is not None for i in rows)
        req_ok[j] = verify_proof(bytes(pks), [bytes(blinded[i]) for i in rows], [bytes(evaluated[i]) for i in rows], bytes(proofs[j]),
                                 [logs[i] for i in rows] if known else None, [dlogs[i] for i in rows] if known else None)
    return req_ok


# ---- the case set ------------------------------------------------------------------------------------------------------------
HASH_TO_GROUP_DST_LEN = len(b"HashToGroup-" + ctx(0))
BASE_INPUT_LENGTHS = (0, 1, 17)
FINALIZE_TAIL = 44                                   # Finalize hashes len(input) + 2 + 2 + 32 + 8 bytes


def input_lengths():
    """0, 1, 17; the six lengths below 128 that put Finalize's len + 44 bytes at each of h2c_model.EDGE_RESIDUES mod 128 (110, 111, 112:
    the padding still fits the block, just, not; 127, 0, 1: the string ends at the block's edge) -- HashToGroup hashes len + 40-byte
    DST + 4 bytes behind Z_pad, the same 44, so they are its edges too; and three blocks"""
    edges = tuple((r - FINALIZE_TAIL) % 128 for r in h2c_model.EDGE_RESIDUES)
    assert HASH_TO_GROUP_DST_LEN + 4 == FINALIZE_TAIL
    return BASE_INPUT_LENGTHS + edges + (h2c_model.THREE_BLOCK_MSG,)


INPUT_LENGTHS = input_lengths()
REQUEST_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257)
ROWS_PER_LENGTH = 3
N_LOGS = 37                                          # distinct a with C = [a]B: a request of 63 and more repeats rows


def _rows(rows, width):
    if not len(rows):
        return np.zeros((0, width), np.uint8)
    return np.stack([np.frombuffer(bytes(r), np.uint8) for r in rows]).reshape(len(rows), width)


def _seeded(n: int, tag: str) -> bytes:
    out = b""
    k = 0
    while len(out) < n:
        out += hashlib.sha512(b"oprf case %s %d" % (tag.encode(), k)).digest()
        k += 1
    return out[:n]


def _scalar(tag: str) -> int:
    return _int(_seeded(64, tag)) % L


SKS = _le(_scalar("skS"))
KEY = _int(SKS)


@functools.lru_cache(maxsize=None)
def log_rows():
    """(a_k, [a_k]B bytes, [skS a_k]B bytes) for N_LOGS seeded a_k"""
    logs = [_scalar("log %d" % k) for k in range(N_LOGS)]
    return tuple((a, base_mult(a), base_mult(a * KEY)) for a in logs)


@functools.lru_cache(maxsize=None)
def honest(length: int, mode: int):
    """ROWS_PER_LENGTH rows of one input length under one mode: input, blind, blinded, evaluated under SKS, output"""
    inp = [_seeded(length, "input %d %d" % (length, r)) for r in range(ROWS_PER_LENGTH)]
    bl = [_le(_scalar("blind %d %d" % (length, r))) for r in range(ROWS_PER_LENGTH)]
    bl[-1] = _le(_int(bl[-1]) + L)                    # one blind above L: read mod L
    blinded = [blind(i, b, mode)[0] for i, b in zip(inp, bl)]
    evaluated = [evaluate_row(SKS, b)[0] for b in blinded]
    output = [finalize(i, b, e)[0] for i, b, e in zip(inp, bl, evaluated)]
    return dict(input=_rows(inp, length), blind=_rows(bl, 32), blinded=_rows(blinded, 32), evaluated=_rows(evaluated, 32),
                output=_rows(output, 64))


def request_offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return np.array(off, np.uint64)


@functools.lru_cache(maxsize=None)
def request_case(shuffled: bool):
    """one call of len(REQUEST_SIZES) requests, in that order or shuffled: rows [a]B with known a, the model's evaluation and proofs"""
    sizes = list(REQUEST_SIZES)
    if shuffled:
        np.random.default_rng(0x9497).shuffle(sizes)
    off = request_offsets(sizes)
    n, m = int(off[-1]), len(sizes)
    lr = log_rows()
    pick = [(7 * i + (3 if shuffled else 0)) % N_LOGS for i in range(n)]
    logs = [lr[k][0] for k in pick]
    blinded = [lr[k][1] for k in pick]
    rand = [_le(_scalar("proof rand %d %d" % (shuffled, j))) for j in range(m)]
    rand[1] = _le(_int(rand[1]) + L)                  # read mod L
    evaluated, proofs, ok, req_ok = voprf_blind_evaluate(SKS, rand, blinded, off, logs)
    assert ok == [1] * n and req_ok == [1] * m
    return dict(sizes=tuple(sizes), offsets=off, logs=tuple(logs), dlogs=tuple(a * KEY % L for a in logs), blinded=_rows(blinded, 32),
                proof_rand=_rows(rand, 32), evaluated=_rows(evaluated, 32), proof=_rows(proofs, 64), pks=base_mult(KEY))


def _flip(b: bytes, bit: int) -> bytes:
    v = bytearray(b)
    v[bit // 8] ^= 1 << (bit % 8)
    return bytes(v)


REJECT_SIZES = (3, 2, 4, 1)                          # the requests of the server's rejection calls


@functools.lru_cache(maxsize=None)
def row_rejections():
    """labelled rows for the per-row calls: (blinded-or-evaluated bytes, blind, label).  The undecodable rows, the identity, blind
    as 0 and as L"""
    lr = log_rows()
    good_blind = _le(_scalar("reject blind"))
    rows = [(b, good_blind, "undecodable: " + why) for b, why in ristretto_model.FIXED_REJECTS]
    rows.append((ZERO32, good_blind, "identity"))
    rows.append((lr[0][1], ZERO32, "blind 0"))
    rows.append((lr[1][1], _le(L), "blind L"))
    rows.append((lr[2][1], good_blind, "valid"))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def server_rejections():
    """labelled calls of the VOPRF server over REJECT_SIZES (or the offsets the label names): dict(label, sks, proof_rand, blinded,
    offsets, logs) with the model's answer under `want`"""
    lr = log_rows()
    off = request_offsets(REJECT_SIZES)
    n, m = int(off[-1]), len(REJECT_SIZES)
    base_logs = [lr[(5 * i + 1) % N_LOGS][0] for i in range(n)]
    base_rows = [lr[(5 * i + 1) % N_LOGS][1] for i in range(n)]
    rand = [_le(_scalar("reject rand %d" % j)) for j in range(m)]
    cases = []

    def add(label, sks=SKS, rnd=None, rows=None, logs=None, offsets=off):
        rnd, rows = list(rnd or rand), list(rows or base_rows)
        logs = list(logs or base_logs)
        logs = [a if base_rows[i] == rows[i] else None for i, a in enumerate(logs)] if len(rows) == n else [None] * len(rows)
        want = voprf_blind_evaluate(sks, rnd, rows, offsets, logs)
        cases.append(dict(label=label, sks=sks, proof_rand=_rows(rnd, 32), blinded=_rows(rows, 32), offsets=np.array(offsets, np.uint64),
                          want=dict(evaluated=_rows(want[0], 32), proof=_rows(want[1], 64), ok=list(want[2]), req_ok=list(want[3]))))
    add("honest")
    for k, (b, why) in enumerate(ristretto_model.FIXED_REJECTS):
        rows = list(base_rows)
        rows[3 + k % 2] = b                           # a row of the second request
        add("undecodable row: %s (%d)" % (why, k), rows=rows)
    rows = list(base_rows)
    rows[5] = ZERO32                                  # a row of the third request
    add("identity row", rows=rows)
    for name, v in (("0", 0), ("L", L)):
        add("skS " + name, sks=_le(v))
        rnd = list(rand)
        rnd[2] = _le(v)
        add("proof_rand " + name, rnd=rnd)
    return tuple(cases)


def malformed_offsets():
    """(label, offsets, requests that must fail) over the n = 10 rows and m = 4 requests of REJECT_SIZES: what the device forms answer
    with req_ok = 0 and the host forms refuse as a bad argument"""
    n = sum(REJECT_SIZES)
    return (("an empty request", [0, 3, 3, 9, n], (1,)),
            ("a decreasing pair", [0, 5, 3, 9, n], (1,)),
            ("past n", [0, 3, 5, 9, n + 2], (3,)),
            ("does not begin at 0", [1, 3, 5, 9, n], ()),
            ("does not end at n", [0, 3, 5, 9, n - 1], ()))


@functools.lru_cache(maxsize=None)
def verify_rejections():
    """labelled calls of VerifyProof over the honest REJECT_SIZES call: dict(label, pks, blinded, evaluated, proof, offsets, want)"""
    honest_call = server_rejections()[0]
    off = honest_call["offsets"]
    blinded = [bytes(r) for r in honest_call["blinded"]]
    evaluated = [bytes(r) for r in honest_call["want"]["evaluated"]]
    proofs = [bytes(r) for r in honest_call["want"]["proof"]]
    pks = base_mult(KEY)
    n = len(blinded)
    cases = []

    def add(label, expect, pk=pks, bl=None, ev=None, pr=None, offsets=off):
        bl, ev, pr = list(bl or blinded), list(ev or evaluated), list(pr or proofs)
        want = voprf_verify(pk, bl, ev, pr, offsets)
        assert want == expect, (label, want, expect)
        cases.append(dict(label=label, pks=pk, blinded=_rows(bl, 32), evaluated=_rows(ev, 32), proof=_rows(pr, 64),
                          offsets=np.array(offsets, np.uint64), want=want))
    add("honest", [1, 1, 1, 1])
    for k, (b, why) in enumerate(ristretto_model.FIXED_REJECTS):
        rows = list(blinded if k % 2 else evaluated)
        rows[3] = b
        add("undecodable row: %s (%d)" % (why, k), [1, 0, 1, 1], **({"bl": rows} if k % 2 else {"ev": rows}))
    rows = list(evaluated)
    rows[0] = ZERO32
    add("identity row", [0, 1, 1, 1], ev=rows)
    c, s = proofs[2][:32], proofs[2][32:]
    for label, p in (("c + L", _le(_int(c) + L) + s), ("s + L", c + _le(_int(s) + L)), ("a flipped bit of c", _flip(c, 77) + s),
                     ("a flipped bit of s", c + _flip(s, 200))):
        pr = list(proofs)
        pr[2] = p
        add(label, [1, 1, 0, 1], pr=pr)
    rows = list(evaluated)
    rows[6] = _flip(rows[6], 9)                       # may or may not decode: the request fails either way
    add("a flipped bit of an evaluated row", [1, 1, 0, 1], ev=rows)
    add("a wrong pkS", [0, 0, 0, 0], pk=base_mult(KEY + 1))
    add("an undecodable pkS", [0, 0, 0, 0], pk=ristretto_model.FIXED_REJECTS[3][0])
    add("the identity as pkS", [0, 0, 0, 0], pk=ZERO32)
    bl, ev = list(blinded), list(evaluated)
    bl[5], bl[6] = bl[6], bl[5]
    ev[5], ev[6] = ev[6], ev[5]
    add("two rows of a request swapped", [1, 1, 0, 1], bl=bl, ev=ev)
    moved = [int(x) for x in off]
    moved[1] -= 1                                     # the last row of the first request given to the second
    add("the last row of a request given to the next", [0, 0, 1, 1], offsets=moved)
    assert n == sum(REJECT_SIZES)
    return tuple(cases)


# ---- the published vectors: RFC 9497 A.1.2 (mode 0x01), the values the issue that added these calls states -----------------------
VOPRF_SEED, VOPRF_INFO = bytes([0xA3]) * 32, b"test key"
VOPRF_SKS = "e6f73f344b79b379f1a0dd37e07ff62e38d9f71345ce62ae3a9bc60b04ccd909"
VOPRF_PKS = "c803e2cc6b05fc15064549b5920659ca4a77b2cca6f04f6b357009335476ad4e"
B1 = "64d37aed22a27f5191de1c1d69fadb899d8862b58eb4220029e036ec4c1f6706"
B2 = "222a5e897cf59db8145db8d16e597e8facb80ae7d4e26d9881aa6f61d645fc0e"
INPUT_1, INPUT_2 = b"\x00", bytes([0x5A]) * 17
VECTORS = (
    dict(inputs=(INPUT_1,), blinds=(B1,), r=B2,
         blinded=("863f330cc1a1259ed5a5998a23acfd37fb4351a793a5b3c090b642ddc439b945",),
         evaluated=("aa8fa048764d5623868679402ff6108d2521884fa138cd7f9c7669a9a014267e",),
         proof="ddef93772692e535d1a53903db24367355cc2cc78de93b3be5a8ffcc6985dd06"
               "6d4346421d17bf5117a2a1ff0fcb2a759f58a539dfbe857a40bce4cf49ec600d",
         outputs=("b58cfbe118e0cb94d79b5fd6a6dafb98764dff49c14e1770b566e42402da1a7d"
                  "a4d8527693914139caee5bd03903af43a491351d23b430948dd50cde10d32b3c",)),
    dict(inputs=(INPUT_2,), blinds=(B1,), r=B2,
         blinded=("cc0b2a350101881d8a4cba4c80241d74fb7dcbfde4a61fde2f91443c2bf9ef0c",),
         evaluated=("60a59a57208d48aca71e9e850d22674b611f752bed48b36f7a91b372bd7ad468",),
         proof="401a0da6264f8cf45bb2f5264bc31e109155600babb3cd4e5af7d181a2c9dc0a"
               "67154fabf031fd936051dec80b0b6ae29c9503493dde7393b722eafdf5a50b02",
         outputs=("8a9a2f3c7f085b65933594309041fc1898d42d0858e59f90814ae90571a6df60"
                  "356f4610bf816f27afdd84f47719e480906d27ecd994985890e5f539e7ea74b6",)),
    dict(inputs=(INPUT_1, INPUT_2), blinds=(B1, B2), r="419c4f4f5052c53c45f3da494d2b67b220d02118e0857cdbcf037f9ea84bbe0c",
         blinded=("863f330cc1a1259ed5a5998a23acfd37fb4351a793a5b3c090b642ddc439b945",
                  "90a0145ea9da29254c3a56be4fe185465ebb3bf2a1801f7124bbbadac751e654"),
         evaluated=("aa8fa048764d5623868679402ff6108d2521884fa138cd7f9c7669a9a014267e",
                    "cc5ac221950a49ceaa73c8db41b82c20372a4c8d63e5dded2db920b7eee36a2a"),
         proof="cc203910175d786927eeb44ea847328047892ddf8590e723c37205cb74600b0a"
               "5ab5337c8eb4ceae0494c2cf89529dcf94572ed267473d567aeed6ab873dee08",
         outputs=("b58cfbe118e0cb94d79b5fd6a6dafb98764dff49c14e1770b566e42402da1a7d"
                  "a4d8527693914139caee5bd03903af43a491351d23b430948dd50cde10d32b3c",
                  "8a9a2f3c7f085b65933594309041fc1898d42d0858e59f90814ae90571a6df60"
                  "356f4610bf816f27afdd84f47719e480906d27ecd994985890e5f539e7ea74b6")),
)

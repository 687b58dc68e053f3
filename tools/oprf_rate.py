#!/usr/bin/env python3
"""tools/oprf_rate.py -- the OPRF / VOPRF calls (ristretto255_OPRF_Blind_dev, ristretto255_OPRF_Finalize_dev,
ristretto255_OPRF_BlindEvaluate_dev, ristretto255_VOPRF_BlindEvaluate_dev, ristretto255_VOPRF_VerifyProof_dev) at 2^10 .. 2^20 rows
per call over inputs of 32 bytes, each beside the COMPOSED sequence of existing *_dev calls of the same build on the same inputs in the
same process, WITHOUT the host hashes and host copies between them (hashed strings are random bytes of the right length: the device
work does not depend on their values):
  * Blind: ristretto255_HashToGroup_dev, ristretto255_ScalarMult_dev;
  * Finalize: ed25519_ScalarInvert_dev, ristretto255_ScalarMult_dev -- and, as a row of its own and ONE round, the same with the
    download of N and the per-item hashlib SHA-512 loop a caller had behind it;
  * OPRF_BlindEvaluate: ristretto255_ScalarMult_dev with the key repeated n times;
  * VOPRF_BlindEvaluate: per row ristretto255_ScalarMult_dev (D_i), ed25519_HashToScalar_dev over 145 bytes (d_i), ristretto255_ScalarMult_dev
    (d_i C_i); per request two ristretto255_ScalarMult_dev (Z, t3), ristretto255_ScalarMultBase_dev (t2), ed25519_HashToScalar_dev over 179
    bytes (c), ed25519_ScalarMulAdd_dev (s) -- without the sums of the requests' rows, which have no call of their own;
  * VOPRF_VerifyProof: per row ed25519_HashToScalar_dev and two ristretto255_ScalarMult_dev; per request three ristretto255_ScalarMult_dev,
    ristretto255_ScalarMultBase_dev, two ristretto255_PointAdd_dev, ed25519_HashToScalar_dev -- again without the sums.
The proof calls run with requests of 64 rows in the sweep, and at the largest size with requests of 1, 64, 4096 and 65535 rows.
HIP events in one process, inputs resident in HBM, the calls in turn in interleaved rounds after a warm-up round, every figure
`launches` calls back to back: best and spread (slowest less fastest round) per call.  Writes profiles/oprf_rate.txt (--out)."""
import argparse
import ctypes as C
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from curve25519_amd import _lib, api, oprf, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="10,12,14,16,18,20")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--launches", type=int, default=2)
ap.add_argument("--input-size", type=int, default=32)
ap.add_argument("--request", type=int, default=64)
ap.add_argument("--request-sizes", default="1,64,4096,65535")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oprf_rate.txt"))
args = ap.parse_args()

L = _lib.load()
dev = torch.device("cuda", 0)
NS = [1 << int(s) for s in args.sizes.split(",")]
NMAX = max(NS)
ISZ = args.input_size
DST_GROUP = b"HashToGroup-OPRFV1-\x01-ristretto255-SHA512"
DST_SCALAR = b"HashToScalar-OPRFV1-\x01-ristretto255-SHA512"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
u8 = lambda n, w=32: torch.empty((n, w), dtype=torch.uint8, device=dev)  # noqa: E731
i32 = lambda n: torch.empty((n, 1), dtype=torch.int32, device=dev)  # noqa: E731


def scalars(n, seed):
    s = synth.random_bytes((n, 32), seed)
    s[:, 31] &= 0x0f                                           # below 2^252: canonical and not zero
    s[:, 0] |= 1
    return s


def offsets_for(n, size):
    off = np.arange(0, n + 1, size, dtype=np.int64)
    if off[-1] != n:
        off = np.append(off, n)
    return off.reshape(-1, 1)


inputs = synth.random_bytes((NMAX, ISZ), 0x9497)
blinds, rands, sks = scalars(NMAX, 0x9498), scalars(NMAX, 0x9499), scalars(1, 0x949A)
d_in, d_bl, d_rand, d_sk = to_dev(inputs), to_dev(blinds), to_dev(rands), to_dev(sks)
d_sk_rep = to_dev(np.repeat(sks, NMAX, axis=0))
d_msg145, d_msg179 = to_dev(synth.random_bytes((NMAX, 145), 0x949B)), to_dev(synth.random_bytes((NMAX, 179), 0x949C))
d_blinded, d_ev, d_out = u8(NMAX), u8(NMAX), u8(NMAX, 64)
d_ok = i32(NMAX)
d_pk = u8(1)
api.ristretto255_ScalarMultBase_dev(d_pk, d_sk)

# what is timed is what is tested: the protocol round-trips on the first rows, and a wrong key is refused
oprf.ristretto255_OPRF_Blind_dev(d_blinded, d_ok, d_in, d_bl, 1)
off0 = to_dev(offsets_for(NMAX, args.request))
m0 = off0.shape[0] - 1
d_proof, d_rok = u8(NMAX, 64), i32(NMAX)
oprf.ristretto255_VOPRF_BlindEvaluate_dev(d_ev, d_proof[:m0], d_ok, d_rok[:m0], d_sk, d_rand[:m0], d_blinded, off0)
torch.cuda.synchronize()
assert bool((d_ok == 1).all()) and bool((d_rok[:m0] == 1).all())
oprf.ristretto255_VOPRF_VerifyProof_dev(d_rok[:m0], d_pk, d_blinded, d_ev, d_proof[:m0], off0)
oprf.ristretto255_OPRF_Finalize_dev(d_out, d_ok, d_in, d_bl, d_ev)
torch.cuda.synchronize()
assert bool((d_rok[:m0] == 1).all()) and bool((d_ok == 1).all())
unblinded, ok = api.ristretto255_ScalarMult(sks.repeat(4, axis=0), api.ristretto255_HashToGroup(inputs[:4], DST_GROUP))
want = [hashlib.sha512(len(i).to_bytes(2, "big") + i.tobytes() + b"\x00\x20" + n.tobytes() + b"Finalize").digest() for i, n in zip(inputs[:4], unblinded)]
assert ok.all() and [bytes(r) for r in d_out[:4].cpu().numpy()] == want, "Finalize(Blind, BlindEvaluate) is Hash(input, skS * HashToGroup(input))"
oprf.ristretto255_VOPRF_VerifyProof_dev(d_rok[:m0], d_blinded[:1], d_blinded, d_ev, d_proof[:m0], off0)
torch.cuda.synchronize()
assert not bool(d_rok[:m0].any()), "another key's proofs are refused"


def ev_ms(f, launches=None):
    launches = launches or args.launches
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def check(rc, what):
    _lib.check(rc, what)


def proof_calls(n, size):
    """(server, verifier, composed server, composed verifier) over n rows in requests of `size`"""
    off = to_dev(offsets_for(n, size))
    m = off.shape[0] - 1
    q_ev, q_pr, q_ok, q_rok, t32, t32b, t32c, s32 = u8(n), u8(m, 64), i32(n), i32(m), u8(n), u8(m), u8(m), u8(n)
    st = stream
    oprf.ristretto255_VOPRF_BlindEvaluate_dev(d_ev[:n], d_proof[:m], d_ok[:n], d_rok[:m], d_sk, d_rand[:m], d_blinded[:n], off)
    proofs = d_proof[:m].clone()
    torch.cuda.synchronize()
    assert bool((d_rok[:m] == 1).all())

    def server():
        check(L.ristretto255_VOPRF_BlindEvaluate_dev(p(q_ev), p(q_pr), p(q_ok), p(q_rok), p(d_sk), p(d_rand), p(d_blinded), p(off), m, n, st()), "server")

    def verifier():
        check(L.ristretto255_VOPRF_VerifyProof_dev(p(q_rok), p(d_pk), p(d_blinded), p(d_ev), p(proofs), p(off), m, n, st()), "verifier")

    def composed_server():
        check(L.ristretto255_ScalarMult_dev(p(q_ev), p(q_ok), p(d_sk_rep), p(d_blinded), n, st()), "D")
        check(L.ed25519_HashToScalar_dev(p(s32), p(d_msg145), 145, DST_SCALAR, len(DST_SCALAR), n, st()), "d")
        check(L.ristretto255_ScalarMult_dev(p(t32), p(q_ok), p(s32), p(d_blinded), n, st()), "dC")
        check(L.ristretto255_ScalarMult_dev(p(t32b), p(q_rok), p(d_sk_rep), p(t32), m, st()), "Z")
        check(L.ristretto255_ScalarMult_dev(p(t32c), p(q_rok), p(d_rand), p(t32), m, st()), "t3")
        check(L.ristretto255_ScalarMultBase_dev(p(t32c), p(d_rand), m, st()), "t2")
        check(L.ed25519_HashToScalar_dev(p(t32b), p(d_msg179), 179, DST_SCALAR, len(DST_SCALAR), m, st()), "c")
        check(L.ed25519_ScalarMulAdd_dev(p(t32c), p(t32b), p(d_sk_rep), p(d_rand), m, st()), "s")

    def composed_verifier():
        check(L.ed25519_HashToScalar_dev(p(s32), p(d_msg145), 145, DST_SCALAR, len(DST_SCALAR), n, st()), "d")
        check(L.ristretto255_ScalarMult_dev(p(t32), p(q_ok), p(s32), p(d_blinded), n, st()), "dC")
        check(L.ristretto255_ScalarMult_dev(p(q_ev), p(q_ok), p(s32), p(d_ev), n, st()), "dD")
        check(L.ristretto255_ScalarMult_dev(p(t32b), p(q_rok), p(d_rand), p(t32), m, st()), "sM")
        check(L.ristretto255_ScalarMult_dev(p(t32c), p(q_rok), p(d_bl), p(q_ev), m, st()), "cZ")
        check(L.ristretto255_PointAdd_dev(p(t32b), p(q_rok), p(t32b), p(t32c), m, st()), "t3")
        check(L.ristretto255_ScalarMult_dev(p(t32c), p(q_rok), p(d_bl), p(d_sk_rep), m, st()), "cY")
        check(L.ristretto255_ScalarMultBase_dev(p(t32b), p(d_rand), m, st()), "sB")
        check(L.ristretto255_PointAdd_dev(p(t32b), p(q_rok), p(t32b), p(t32c), m, st()), "t2")
        check(L.ed25519_HashToScalar_dev(p(t32b), p(d_msg179), 179, DST_SCALAR, len(DST_SCALAR), m, st()), "c")

    keep = (off, proofs, q_ev, q_pr, q_ok, q_rok, t32, t32b, t32c, s32)
    return keep, m, server, verifier, composed_server, composed_verifier


def calls(n):
    q32, q64, q_ok, q_t = u8(n), u8(n, 64), i32(n), u8(n)
    st = stream
    keep, m, server, verifier, composed_server, composed_verifier = proof_calls(n, args.request)

    def composed_blind():
        check(L.ristretto255_HashToGroup_dev(p(q_t), p(d_in), ISZ, DST_GROUP, len(DST_GROUP), n, st()), "h2g")
        check(L.ristretto255_ScalarMult_dev(p(q32), p(q_ok), p(d_bl), p(q_t), n, st()), "mult")

    def composed_finalize():
        check(L.ed25519_ScalarInvert_dev(p(q_t), p(q_ok), p(d_bl), n, st()), "invert")
        check(L.ristretto255_ScalarMult_dev(p(q32), p(q_ok), p(q_t), p(d_ev), n, st()), "mult")

    out = {
        "OPRF_Blind": lambda: check(L.ristretto255_OPRF_Blind_dev(p(q32), p(q_ok), p(d_in), ISZ, p(d_bl), 1, n, st()), "blind"),
        "  composed: HashToGroup + ScalarMult": composed_blind,
        "OPRF_Finalize": lambda: check(L.ristretto255_OPRF_Finalize_dev(p(q64), p(q_ok), p(d_in), ISZ, p(d_bl), p(d_ev), n, st()), "finalize"),
        "  composed: ScalarInvert + ScalarMult": composed_finalize,
        "OPRF_BlindEvaluate": lambda: check(L.ristretto255_OPRF_BlindEvaluate_dev(p(q32), p(q_ok), p(d_sk), p(d_blinded), n, st()), "evaluate"),
        "  composed: ScalarMult, key repeated": lambda: check(L.ristretto255_ScalarMult_dev(p(q32), p(q_ok), p(d_sk_rep), p(d_blinded), n, st()), "mult"),
        f"VOPRF_BlindEvaluate /{args.request}": server,
        "  composed server (no sums)": composed_server,
        f"VOPRF_VerifyProof /{args.request}": verifier,
        "  composed verifier (no sums)": composed_verifier,
    }

    def finalize_with_host_hashes():
        t0 = time.perf_counter()
        composed_finalize()
        torch.cuda.synchronize()
        rows = q32.cpu().numpy()
        for i, r in zip(inputs[:n], rows):
            hashlib.sha512(ISZ.to_bytes(2, "big") + i.tobytes() + b"\x00\x20" + r.tobytes() + b"Finalize").digest()
        return (time.perf_counter() - t0) * 1e3

    return (keep, q32, q64, q_ok, q_t), out, finalize_with_host_hashes


say(f"# tools/oprf_rate.py on {torch.cuda.get_device_name(0)}: n rows per call, inputs of {ISZ} bytes, requests of {args.request} rows; "
    f"{args.rounds} interleaved rounds of {args.launches} launches back to back, every call in turn on the same inputs; best ms per call "
    f"(spread ms) | M rows/s; x = time against the composed sequence of existing calls below it")
at_max = {}
for n in NS:
    keep, vs, with_hashes = calls(n)
    times = {name: [] for name in vs}
    for r in range(args.rounds + 1):                           # (the first round warms up and is not counted)
        for name, f in vs.items():
            t = ev_ms(f)
            if r:
                times[name].append(t)
    say(f"n = 2^{n.bit_length() - 1}")
    names = list(times)
    for k, name in enumerate(names):
        ts = times[name]
        best, spread = min(ts), max(ts) - min(ts)
        ref = min(times[names[k + 1]]) if not name.startswith("  ") else best
        say(f"  {name:>40} {best:9.3f} ms ({spread:6.3f}) {n / best / 1e3:9.2f} M/s" + ("" if name.startswith("  ") else f"  x {best / ref:5.2f}"))
    say(f"  {'  composed Finalize WITH host hashes':>40} {with_hashes():9.1f} ms (one round: device sequence, download, hashlib loop)")
    if n == NMAX:
        at_max = {name: (min(ts), max(ts) - min(ts)) for name, ts in times.items()}
    del keep

say(f"# the proof calls at n = 2^{NMAX.bit_length() - 1} rows by request size (the server's and the verifier's per-request stage is ONE lane per request)")
for size in (int(s) for s in args.request_sizes.split(",")):
    n = NMAX // size * size if size > 1 else NMAX
    keep, m, server, verifier, _, _ = proof_calls(n, size)
    ts = {"VOPRF_BlindEvaluate": [], "VOPRF_VerifyProof": []}
    for r in range(3):
        for name, f in (("VOPRF_BlindEvaluate", server), ("VOPRF_VerifyProof", verifier)):
            t = ev_ms(f, 1)
            if r:
                ts[name].append(t)
    for name, t in ts.items():
        say(f"  {name:>22} {m:8d} requests of {size:5d} rows ({n} rows) {min(t):10.3f} ms ({max(t) - min(t):6.3f}) {n / min(t) / 1e3:9.2f} M rows/s")
    del keep

say(f"# at n = 2^{NMAX.bit_length() - 1}, each call against its composed sequence:")
names = list(at_max)
for k in range(0, len(names), 2):
    (ms, sp), (ref, rsp) = at_max[names[k]], at_max[names[k + 1]]
    verdict = "not slower than" if ms <= ref + max(sp, rsp) else "SLOWER than"
    say(f"#   {names[k]:>26} {ms:8.3f} ms (spread {sp:.3f}) = {ms / ref:5.2f} x composed ({ref:.3f} ms, spread {rsp:.3f}): {verdict} the composed sequence")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", args.out)

#!/usr/bin/env python3
"""tools/h2c_rate.py -- the hashing calls (ristretto255_HashToGroup_dev, ed25519_HashToScalar_dev, ed25519_HashToCurve_dev,
ed25519_EncodeToCurve_dev, ed25519_MapToCurve_dev, c25519_ExpandMessageXmd_dev at 64 bytes) at 2^10 .. 2^20 elements per call, over
messages of 32 bytes and DSTs of 32 and 64 bytes (a one- and a two-block b_i), with ristretto255_FromHash_dev and
ed25519_SignMessage_dev of the same build on the same n beside them as the scale: FromHash is the cost of HashToGroup's map alone
(what a caller paid before, behind a host loop of SHA-512 calls), SignMessage three compressions plus a comb walk.  By operation
count HashToGroup is FromHash plus three compressions and HashToCurve two square-root chains, one inversion and four or five
compressions; the last lines give the measured ratios.  HIP events in one process, inputs resident in HBM, the calls in turn on the
same inputs in interleaved rounds after a warm-up round, every figure `launches` calls back to back: best and spread (slowest less
fastest round) per call.  Writes profiles/h2c_rate.txt (--out)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from curve25519_amd import _lib, api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="10,11,12,13,14,15,16,17,18,19,20")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--launches", type=int, default=4)
ap.add_argument("--msg-size", type=int, default=32)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "h2c_rate.txt"))
args = ap.parse_args()

L = _lib.load()
dev = torch.device("cuda", 0)
NS = [1 << int(s) for s in args.sizes.split(",")]
NMAX = max(NS)
MSG = args.msg_size
DSTS = {32: b"h2c_rate.py-DST-of-32-bytes-----" [:32], 64: (b"h2c_rate.py-DST-of-64-bytes-" + b"-" * 64)[:64]}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


msgs = synth.random_bytes((NMAX, MSG), 0x9380)
hashes = synth.random_bytes((NMAX, 64), 0x9381)
_, priv = api.ed25519_CreateKeyPair(synth.random_bytes((NMAX, 32), 0x9382))
d_msgs, d_hashes, d_priv = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (msgs, hashes, priv))
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

# the device's bytes are the host form's, and HashToGroup is FromHash of the expander's 64 bytes: what is timed is what is tested
check = api.ristretto255_HashToGroup(msgs[:256], DSTS[32])
assert np.array_equal(check, api.ristretto255_FromHash(api.c25519_ExpandMessageXmd(msgs[:256], DSTS[32], 64)))


def ev_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.launches):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.launches


def calls(n):
    q = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    out = {}
    for dl, dst in DSTS.items():
        for name in ("ristretto255_HashToGroup", "ed25519_HashToScalar", "ed25519_HashToCurve", "ed25519_EncodeToCurve"):
            fn = getattr(L, name + "_dev")
            out[f"{name} dst={dl}"] = (lambda fn=fn, dst=dst, name=name: _lib.check(fn(p(q), p(d_msgs), MSG, dst, len(dst), n, stream()), name))
        out[f"c25519_ExpandMessageXmd(64) dst={dl}"] = (lambda dst=dst: _lib.check(
            L.c25519_ExpandMessageXmd_dev(p(q), p(d_msgs), MSG, dst, len(dst), 64, n, stream()), "xmd"))
    out["ed25519_MapToCurve"] = lambda: _lib.check(L.ed25519_MapToCurve_dev(p(q), p(d_hashes), n, stream()), "map")
    out["ristretto255_FromHash"] = lambda: _lib.check(L.ristretto255_FromHash_dev(p(q), p(d_hashes), n, stream()), "fromhash")
    out["ed25519_SignMessage"] = lambda: _lib.check(L.ed25519_SignMessage_dev(p(q), p(d_priv), p(d_msgs), MSG, n, stream()), "sign")
    return q, out


say(f"# tools/h2c_rate.py on {torch.cuda.get_device_name(0)}: n elements per call, messages of {MSG} bytes, DSTs of {sorted(DSTS)} bytes; "
    f"{args.rounds} interleaved rounds of {args.launches} launches back to back, every call in turn on the same inputs; best ms per call "
    f"(spread ms) | M/s; x = rate against ristretto255_FromHash_dev of the same build beside it")
at_max = {}
for n in NS:
    keep, vs = calls(n)
    times = {name: [] for name in vs}
    for r in range(args.rounds + 1):                           # (the first round warms up and is not counted)
        for name, f in vs.items():
            t = ev_ms(f)
            if r:
                times[name].append(t)
    say(f"n = 2^{n.bit_length() - 1}")
    ref = min(times["ristretto255_FromHash"])
    for name, ts in times.items():
        best, spread = min(ts), max(ts) - min(ts)
        say(f"  {name:>40} {best:9.3f} ms ({spread:6.3f}) {n / best / 1e3:9.2f} M/s  x {ref / best:5.2f}")
    if n == NMAX:
        at_max = {name: min(ts) for name, ts in times.items()}

fh_ms, sign_ms = at_max["ristretto255_FromHash"], at_max["ed25519_SignMessage"]
say(f"# at n = 2^{NMAX.bit_length() - 1}, against ristretto255_FromHash_dev ({fh_ms:.3f} ms) and ed25519_SignMessage_dev ({sign_ms:.3f} ms):")
for name, ms in at_max.items():
    if name not in ("ristretto255_FromHash", "ed25519_SignMessage"):
        say(f"#   {name:>40} {ms:8.3f} ms = {ms / fh_ms:5.2f} x FromHash, {ms / sign_ms:5.2f} x SignMessage")
xmd = at_max["c25519_ExpandMessageXmd(64) dst=32"]
say(f"# HashToGroup less FromHash: {at_max['ristretto255_HashToGroup dst=32'] - fh_ms:.3f} ms for three compressions; the expander alone "
    f"(64 bytes out, dst = 32): {xmd:.3f} ms")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", args.out)

#!/usr/bin/env python3
"""tools/ristretto_rate.py -- the ristretto255 calls (ristretto255_ScalarMult_dev at each SCALARMULT_WINDOW, ristretto255_ScalarMultBase_dev,
ristretto255_PointAdd_dev, ristretto255_PointSub_dev, ristretto255_FromHash_dev, ristretto255_IsValidPoint_dev) at one element and at
2^10 .. 2^20 elements per call, with the Edwards group calls of the same build on the same n beside them as the scale
(ed25519_ScalarMult_noclamp_dev at each width, ed25519_ScalarMultBase_noclamp_dev, ed25519_PointAdd_dev): a ristretto255 call is
the Edwards call with the shared inversion replaced by square-root chains in the lane (254 squarings and 11 products each; two for
ScalarMult, one for ScalarMultBase, three for PointAdd and for FromHash, one for IsValidPoint).  HIP events in one process, inputs
resident in HBM, the calls in turn on the same inputs in interleaved rounds after a warm-up round: best and spread (slowest less
fastest round) per call.  The ristretto255 points are FromHash outputs, the Edwards points honest public keys; every lane does the
same work whatever its inputs.  The last lines name the width that is fastest at the largest size and say whether it wins by more
than the rounds' spread: otherwise the ristretto255 default is the group calls' (csrc/engine_ristretto.hip: RIST_WINDOW_DEFAULT).
Writes profiles/ristretto_rate.txt (--out)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from curve25519_amd import _lib, api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="0,10,11,12,13,14,15,16,17,18,19,20")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--single-calls", type=int, default=100)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ristretto_rate.txt"))
args = ap.parse_args()

L = _lib.load()
dev = torch.device("cuda", 0)
NS = [1 << int(s) for s in args.sizes.split(",")]
NMAX = max(NS)
WINDOWS = (2, 3, 4)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


hashes = synth.random_bytes((NMAX, 64), 0x7201)
points = api.ristretto255_FromHash(hashes)
assert api.ristretto255_IsValidPoint(points[:4096]).all()
scalars = synth.random_bytes((NMAX, 32), 0x7202)
pub, _ = api.ed25519_CreateKeyPair(synth.random_bytes((NMAX, 32), 0x7203))
d_hashes, d_points, d_scalars, d_pub = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (hashes, points, scalars, pub))
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731


def ev_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)


def calls(n):
    q = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    okw = torch.empty((n, 1), dtype=torch.int32, device=dev)

    def windowed(fn, pts, w, name):
        def run():
            with _lib.tunable("SCALARMULT_WINDOW", w):
                _lib.check(fn(p(q), p(okw), p(d_scalars), p(pts), n, stream()), name)
        return run

    out = {}
    for w in WINDOWS:
        out[f"ristretto255_ScalarMult W={w}"] = windowed(L.ristretto255_ScalarMult_dev, d_points, w, "ristretto255_ScalarMult_dev")
        out[f"ed25519_ScalarMult_noclamp W={w}"] = windowed(L.ed25519_ScalarMult_noclamp_dev, d_pub, w, "ed25519_ScalarMult_noclamp_dev")
    out.update({
        "ristretto255_ScalarMultBase": lambda: _lib.check(L.ristretto255_ScalarMultBase_dev(p(q), p(d_scalars), n, stream()), "rBase"),
        "ed25519_ScalarMultBase_noclamp": lambda: _lib.check(L.ed25519_ScalarMultBase_noclamp_dev(p(q), p(d_scalars), n, stream()), "eBase"),
        "ristretto255_PointAdd": lambda: _lib.check(L.ristretto255_PointAdd_dev(p(q), p(okw), p(d_points), p(d_points[NMAX - n:]), n, stream()), "rAdd"),
        "ristretto255_PointSub": lambda: _lib.check(L.ristretto255_PointSub_dev(p(q), p(okw), p(d_points), p(d_points[NMAX - n:]), n, stream()), "rSub"),
        "ed25519_PointAdd": lambda: _lib.check(L.ed25519_PointAdd_dev(p(q), p(okw), p(d_pub), p(d_pub[NMAX - n:]), n, stream()), "eAdd"),
        "ristretto255_FromHash": lambda: _lib.check(L.ristretto255_FromHash_dev(p(q), p(d_hashes), n, stream()), "rFromHash"),
        "ristretto255_IsValidPoint": lambda: _lib.check(L.ristretto255_IsValidPoint_dev(p(okw), p(d_points), n, stream()), "rIsValid"),
    })
    return (q, okw), out


SCALE = {"ristretto255_ScalarMultBase": "ed25519_ScalarMultBase_noclamp", "ristretto255_PointAdd": "ed25519_PointAdd",
         "ristretto255_PointSub": "ed25519_PointAdd"}
SCALE.update({f"ristretto255_ScalarMult W={w}": f"ed25519_ScalarMult_noclamp W={w}" for w in WINDOWS})

say(f"# tools/ristretto_rate.py on {torch.cuda.get_device_name(0)}: n elements per call; {args.rounds} interleaved rounds, every call in "
    f"turn on the same inputs; best ms (spread ms) | M/s; x = rate against the Edwards call of the same build beside it")
at_max = {}
for n in NS:
    keep, vs = calls(n)
    times = {name: [] for name in vs}
    for r in range(args.rounds + 1):                           # (the first round warms up and is not counted)
        for name, f in vs.items():
            t = ev_ms(f)
            if r:
                times[name].append(t)
    assert keep[1].cpu().numpy().all()
    say(f"n = 2^{n.bit_length() - 1}")
    for name, ts in times.items():
        best, spread = min(ts), max(ts) - min(ts)
        rel = f"  x {min(times[SCALE[name]]) / best:5.2f}" if name in SCALE else ""
        say(f"  {name:>32} {best:9.3f} ms ({spread:6.3f}) {n / best / 1e3:9.2f} M/s{rel}")
    if n == NMAX:
        at_max = {w: times[f"ristretto255_ScalarMult W={w}"] for w in WINDOWS}

say("# a call of ONE element (device pointers, one synchronise per call, host clock): median | best, microseconds")
_, one = calls(1)
for name, f in one.items():
    ts = []
    for i in range(args.single_calls + 10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts = np.sort(np.array(ts[10:]))
    say(f"  {name:>32} {ts[len(ts) // 2]:9.1f} | {ts[0]:9.1f}")

order = sorted(WINDOWS, key=lambda w: min(at_max[w]))
fastest, second = order[0], order[1]
gap = min(at_max[second]) - min(at_max[fastest])
spread = max(max(at_max[w]) - min(at_max[w]) for w in (fastest, second))
say(f"# at n = 2^{NMAX.bit_length() - 1}: W = {fastest} is fastest, {gap:.3f} ms ahead of W = {second}; the rounds' spread is {spread:.3f} ms: "
    + (f"W = {fastest} wins by more than the spread" if gap > spread else "no win beyond the spread, the group calls' default is taken"))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", args.out)

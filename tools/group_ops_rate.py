#!/usr/bin/env python3
"""tools/group_ops_rate.py -- the group calls (ed25519_ScalarMult_dev at each SCALARMULT_WINDOW, ed25519_ScalarMult_noclamp_dev,
ed25519_ScalarMultBase[_noclamp]_dev, ed25519_PointAdd_dev, ed25519_PointSub_dev) at 2^10 .. 2^20 elements per call, with
curve25519_dh_CreateSharedKey_dev of the same build on the same n beside them as the scale (the variable-base walk is 2,840 / 2,520 /
2,400 field products at W = 2 / 3 / 4, the ladder 2,550), and the latency of a call of ONE element.  HIP events in one process,
inputs resident in HBM, the calls in turn on the same inputs in interleaved rounds after a warm-up round: best and spread (slowest
less fastest round) per call.  The points are honest public keys with one mixed-order key in eight; every lane does the same work
whatever its inputs.  The last lines name the width that is fastest at the largest size and say whether it wins by more than the
rounds' spread: that decides SCALARMULT_WINDOW's built-in value (csrc/engine_group.hip).  Writes profiles/group_ops_rate.txt (--out)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from curve25519_amd import _lib, api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="10,11,12,13,14,15,16,17,18,19,20")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--single-calls", type=int, default=100)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_ops_rate.txt"))
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


pub, _ = api.ed25519_CreateKeyPair(synth.random_bytes((NMAX, 32), 0x6c01))
from key_model import mixed_order_keys  # noqa: E402  (the test model's A + T: inputs only, nothing is judged here)
mixed = np.stack([np.frombuffer(k, np.uint8) for k in mixed_order_keys(pub[:8])])
points = pub.copy()
points[7::8] = mixed[np.arange(len(points[7::8])) % len(mixed)]
scalars = synth.random_bytes((NMAX, 32), 0x6c02)
xpk, ok = api.ed25519_PublicKey_to_X25519(pub)
assert ok.all()
d_points, d_scalars, d_xpk = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (points, scalars, xpk))
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731


def ev_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)


def calls(n):
    q = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    okw = torch.empty((n, 1), dtype=torch.int32, device=dev)
    sk = d_scalars[:n].clone()                               # the ladder clamps its secret in place

    def windowed(w):
        def run():
            with _lib.tunable("SCALARMULT_WINDOW", w):
                _lib.check(L.ed25519_ScalarMult_dev(p(q), p(okw), p(d_scalars), p(d_points), n, stream()), "ScalarMult_dev")
        return run

    out = {f"ScalarMult W={w}": windowed(w) for w in WINDOWS}
    out.update({
        "ScalarMult_noclamp": lambda: _lib.check(L.ed25519_ScalarMult_noclamp_dev(p(q), p(okw), p(d_scalars), p(d_points), n, stream()), "noclamp"),
        "ScalarMultBase": lambda: _lib.check(L.ed25519_ScalarMultBase_dev(p(q), p(d_scalars), n, stream()), "ScalarMultBase_dev"),
        "ScalarMultBase_noclamp": lambda: _lib.check(L.ed25519_ScalarMultBase_noclamp_dev(p(q), p(d_scalars), n, stream()), "Base_noclamp"),
        "PointAdd": lambda: _lib.check(L.ed25519_PointAdd_dev(p(q), p(okw), p(d_points), p(d_points[NMAX - n:]), n, stream()), "PointAdd_dev"),
        "PointSub": lambda: _lib.check(L.ed25519_PointSub_dev(p(q), p(okw), p(d_points), p(d_points[NMAX - n:]), n, stream()), "PointSub_dev"),
        "CreateSharedKey": lambda: _lib.check(L.curve25519_dh_CreateSharedKey_dev(p(q), p(d_xpk), p(sk), n, stream()), "CreateSharedKey_dev"),
    })
    return (q, okw, sk), out


say(f"# tools/group_ops_rate.py on {torch.cuda.get_device_name(0)}: n elements per call, honest points with one mixed-order point in "
    f"eight; {args.rounds} interleaved rounds, every call in turn on the same inputs; best ms (spread ms) | M/s; "
    f"x = rate against curve25519_dh_CreateSharedKey_dev")
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
    ladder = min(times["CreateSharedKey"])
    say(f"n = 2^{n.bit_length() - 1}")
    for name, ts in times.items():
        best, spread = min(ts), max(ts) - min(ts)
        say(f"  {name:>24} {best:9.3f} ms ({spread:6.3f}) {n / best / 1e3:9.2f} M/s  x {ladder / best:5.2f}")
    if n == NMAX:
        at_max = {w: times[f"ScalarMult W={w}"] for w in WINDOWS}

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
    say(f"  {name:>24} {ts[len(ts) // 2]:9.1f} | {ts[0]:9.1f}")

order = sorted(WINDOWS, key=lambda w: min(at_max[w]))
fastest, second = order[0], order[1]
gap = min(at_max[second]) - min(at_max[fastest])
spread = max(max(at_max[w]) - min(at_max[w]) for w in (fastest, second))
say(f"# at n = 2^{NMAX.bit_length() - 1}: W = {fastest} is fastest, {gap:.3f} ms ahead of W = {second}; the rounds' spread is {spread:.3f} ms: "
    + (f"W = {fastest} wins by more than the spread" if gap > spread else f"no win beyond the spread, the smaller width W = {min(fastest, second)} is taken"))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", args.out)

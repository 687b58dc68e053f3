#!/usr/bin/env python3
"""tools/scalar_rate.py -- the scalar calls mod L: ed25519_ScalarInvert_dev at 2^10 .. 2^20 elements per call at every group size K
of its shared inversion (tunable SC_INVERT_K: 1, 2, 4, 8, 16) and at the built-in choice, and ed25519_ScalarMul_dev,
ed25519_ScalarMulAdd_dev and ed25519_ScalarReduce_dev at 2^20.  HIP events in one process, inputs resident in HBM, the calls in turn on
the same inputs in interleaved rounds after a warm-up round; a round's figure for a call is the time of --reps launches back to back
on one stream between two events, divided by their number (a single launch of 30-100 us would measure the launch as much as the
kernel): best and spread (slowest less fastest round) per call.  Every lane does
the same work whatever its inputs.  No pass/fail threshold rests on these figures: per size the last lines name the K that is fastest
and say whether it wins by more than the rounds' spread -- that decides the built-in choice (csrc/engine_scalar.hip: sc_invert_k)
-- and the 2^20 rows fill README.md's row.  Writes profiles/scalar_rate.txt (--out)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from curve25519_amd import _lib, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="10,11,12,13,14,15,16,17,18,19,20")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scalar_rate.txt"))
args = ap.parse_args()

L = _lib.load()
dev = torch.device("cuda", 0)
NS = [1 << int(s) for s in args.sizes.split(",")]
NMAX = max(NS)
KS = (1, 2, 4, 8, 16)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


a, b, c = (synth.random_bytes((NMAX, 32), seed) for seed in (0x5C01, 0x5C02, 0x5C03))
wide = synth.random_bytes((NMAX, 64), 0x5C04)
d_a, d_b, d_c, d_wide = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (a, b, c, wide))
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731


def ev_ms(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    f(1)                                                       # (the knob is set and the shape warm before the window opens)
    torch.cuda.synchronize()
    e0.record(); f(args.reps); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps


def calls(n):
    r = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    okw = torch.empty((n, 1), dtype=torch.int32, device=dev)

    def invert(k):
        def run(reps):
            with _lib.tunable("SC_INVERT_K", k):
                for _ in range(reps):
                    _lib.check(L.ed25519_ScalarInvert_dev(p(r), p(okw), p(d_a), n, stream()), "ed25519_ScalarInvert_dev")
        return run

    def plain(fn, *ptrs):
        def run(reps):
            for _ in range(reps):
                _lib.check(fn(p(r), *ptrs, n, stream()), "scalar call")
        return run

    out = {f"ed25519_ScalarInvert K={k}": invert(k) for k in KS}
    out["ed25519_ScalarInvert built-in"] = invert(-1)
    if n == NMAX:
        out["ed25519_ScalarMul"] = plain(L.ed25519_ScalarMul_dev, p(d_a), p(d_b))
        out["ed25519_ScalarMulAdd"] = plain(L.ed25519_ScalarMulAdd_dev, p(d_a), p(d_b), p(d_c))
        out["ed25519_ScalarReduce"] = plain(L.ed25519_ScalarReduce_dev, p(d_wide))
    return (r, okw), out


say(f"# tools/scalar_rate.py on {torch.cuda.get_device_name(0)}: n elements per call; {args.rounds} interleaved rounds, every call in turn "
    f"on the same inputs, {args.reps} launches back to back per figure; best ms per call (spread ms) | M/s")
verdicts = []
for n in NS:
    keep, vs = calls(n)
    times = {name: [] for name in vs}
    for rnd in range(args.rounds + 1):                         # (the first round warms up and is not counted)
        for name, f in vs.items():
            t = ev_ms(f)
            if rnd:
                times[name].append(t)
    assert keep[1].cpu().numpy().all()
    say(f"n = 2^{n.bit_length() - 1}")
    for name, ts in times.items():
        best, spread = min(ts), max(ts) - min(ts)
        say(f"  {name:>32} {best:9.3f} ms ({spread:6.3f}) {n / best / 1e3:9.2f} M/s")
    order = sorted(KS, key=lambda k: min(times[f"ed25519_ScalarInvert K={k}"]))
    t0, t1 = (times[f"ed25519_ScalarInvert K={k}"] for k in order[:2])
    gap, spread = min(t1) - min(t0), max(max(t0) - min(t0), max(t1) - min(t1))
    verdicts.append(f"# n = 2^{n.bit_length() - 1}: K = {order[0]} is fastest, {gap:.3f} ms ahead of K = {order[1]}; the rounds' spread is "
                    f"{spread:.3f} ms: " + ("a win beyond the spread" if gap > spread else "no win beyond the spread"))
for v in verdicts:
    say(v)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", args.out)

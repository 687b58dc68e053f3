#!/usr/bin/env python3
"""tools/msm_rate.py -- the multiscalar calls (ed25519_MultiScalarMult[_vartime]_dev, ristretto255_MultiScalarMult[_vartime]_dev)
beside what a caller had before, on the same inputs in the same process:
  * shapes with n_groups * m = 2^20 rows, m in {2, 64, 4096, 2^16, 2^18, 2^20}: the plain call; the _vartime call forced onto the
    bucket path (MSM_BUCKET_MIN = 1) at every MSM_WINDOW 7..13 -- where the groups, which that path runs one after the other, are at
    most --max-bucket-groups; and the COMPOSED sequence: *_ScalarMult_noclamp_dev (ed25519) / ristretto255_ScalarMult_dev over all rows,
    then log2 m rounds of *_PointAdd_dev that each add the upper half of what is left to the lower half (for n_groups = 1 that is the
    group's sum, checked against the plain call; for more groups it is the same work);
  * the crossover: n_groups = 1, m = 2^10 .. 2^20, the plain call against the bucket path at every width.
HIP events in one process, inputs resident in HBM, canonical random scalars and distinct valid points, the calls in turn in interleaved
rounds after a warm-up round: best ms and spread (slowest less fastest round) per call.  Writes profiles/msm_rate.txt (--out)."""
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
ap.add_argument("--log-rows", type=int, default=20)
ap.add_argument("--group-sizes", default="1,6,12,16,18,20", help="log2 m of the shapes with n_groups * m = 2^log-rows")
ap.add_argument("--crossover", default="10,11,12,13,14,15,16,17,18,19,20", help="log2 m of the n_groups = 1 sweep")
ap.add_argument("--groups", default="ed25519,ristretto255")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--max-bucket-groups", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_rate.txt"))
args = ap.parse_args()

L = _lib.load()
dev = torch.device("cuda", 0)
N = 1 << args.log_rows
WIDTHS = tuple(range(7, 14))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
u8 = lambda n: torch.empty((n, 32), dtype=torch.uint8, device=dev)  # noqa: E731
i32 = lambda n: torch.empty((n, 1), dtype=torch.int32, device=dev)  # noqa: E731
check = _lib.check


def ev_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def rounds(calls):
    """{name: (best, spread)} over interleaved rounds, the first one not counted"""
    times = {name: [] for name in calls}
    for r in range(args.rounds + 1):
        for name, f in calls.items():
            t = ev_ms(f)
            if r:
                times[name].append(t)
    return {name: (min(ts), max(ts) - min(ts)) for name, ts in times.items()}


scalars = synth.random_bytes((N, 32), 0x3501)
scalars[:, 31] &= 0x0f                                         # below 2^252: canonical, so the composed sequence's low 255 bits are the scalar
d_sc = to_dev(scalars)
base_sc = synth.random_bytes((N, 32), 0x3502)
base_sc[:, 31] &= 0x0f
d_base = to_dev(base_sc)

for group in args.groups.split(","):
    stem = {"ed25519": "ed25519", "ristretto255": "ristretto255"}[group]
    mult = getattr(L, "ed25519_ScalarMult_noclamp_dev" if group == "ed25519" else "ristretto255_ScalarMult_dev")
    add = getattr(L, stem + "_PointAdd_dev")
    plain, vartime = getattr(L, stem + "_MultiScalarMult_dev"), getattr(L, stem + "_MultiScalarMult_vartime_dev")
    d_pt = u8(N)
    base = getattr(L, "ed25519_ScalarMultBase_noclamp_dev" if group == "ed25519" else "ristretto255_ScalarMultBase_dev")
    check(base(p(d_pt), p(d_base), N, stream()), "base")       # N distinct valid points
    t_a, t_b, t_ok, q, ok = u8(N), u8(N), i32(N), u8(N), i32(N)

    def composed(rows, m):
        check(mult(p(t_a), p(t_ok), p(d_sc), p(d_pt), rows, stream()), "mult")
        src, dst, left = t_a, t_b, rows
        for _ in range(m.bit_length() - 1):
            left //= 2
            check(add(p(dst), p(t_ok), p(src), C.c_void_p(src.data_ptr() + 32 * left), left, stream()), "add")
            src, dst = dst, src
        return src

    def bucket_call(m, n_groups, c):
        """the _vartime call on the bucket path at width c (the knobs are host words: setting them is not in the way of the events)"""
        def f():
            with _lib.tunable("MSM_BUCKET_MIN", 1), _lib.tunable("MSM_WINDOW", c):
                check(vartime(p(q), p(ok), p(d_sc), p(d_pt), m, n_groups, stream()), "vartime")
        return f

    # what is timed is what is tested: one group of 2^12 rows three ways
    m0 = 1 << 12
    check(plain(p(q), p(ok), p(d_sc), p(d_pt), m0, 1, stream()), "plain")
    want = q[:1].cpu().numpy().copy()
    got = composed(m0, m0)[:1].cpu().numpy()
    with _lib.tunable("MSM_BUCKET_MIN", 1):
        check(vartime(p(q), p(ok), p(d_sc), p(d_pt), m0, 1, stream()), "vartime")
    torch.cuda.synchronize()
    assert int(ok[0]) == 1 and np.array_equal(want, got) and np.array_equal(want, q[:1].cpu().numpy()), "the three ways agree"

    say(f"# tools/msm_rate.py on {torch.cuda.get_device_name(0)}, {group}: {args.rounds} interleaved rounds after a warm-up round, one call "
        f"per figure; best ms (spread ms) | M rows/s.  bucket cN: the _vartime call with MSM_BUCKET_MIN = 1, MSM_WINDOW = N")
    say(f"## n_groups * m = 2^{args.log_rows} rows")
    for lg in (int(s) for s in args.group_sizes.split(",")):
        m, n_groups = 1 << lg, N >> lg
        calls = {"plain": lambda: check(plain(p(q), p(ok), p(d_sc), p(d_pt), m, n_groups, stream()), "plain"),
                 "composed": lambda: composed(N, m)}
        if n_groups <= args.max_bucket_groups:
            calls.update({f"bucket c{c}": bucket_call(m, n_groups, c) for c in WIDTHS})
        res = rounds(calls)
        say(f"m = 2^{lg}, n_groups = {n_groups}")
        for name, (best, spread) in res.items():
            say(f"  {name:>12} {best:10.3f} ms ({spread:6.3f}) {N / best / 1e3:9.2f} M rows/s")
        if n_groups > args.max_bucket_groups:
            say(f"  {'bucket':>12} not timed: {n_groups} groups run one after the other, nine launches each")
        (pb, ps), (cb, cs) = res["plain"], res["composed"]
        say(f"  plain = {pb / cb:5.2f} x composed: " + ("not slower" if pb <= cb + max(ps, cs) else "SLOWER") + " than the composed sequence")

    say("## crossover: n_groups = 1")
    first_win = None
    for lg in (int(s) for s in args.crossover.split(",")):
        m = 1 << lg
        calls = {"plain": lambda: check(plain(p(q), p(ok), p(d_sc), p(d_pt), m, 1, stream()), "plain")}
        calls.update({f"c{c}": bucket_call(m, 1, c) for c in WIDTHS})
        res = rounds(calls)
        (pb, ps) = res["plain"]
        best_c = min(WIDTHS, key=lambda c: res[f"c{c}"][0])
        bb, bs = res[f"c{best_c}"]
        wins = bb + max(ps, bs) < pb
        first_win = (first_win if first_win is not None else lg) if wins else None
        say(f"  m = 2^{lg:<2} plain {pb:9.3f} ({ps:5.3f})  bucket " + " ".join(f"c{c} {res[f'c{c}'][0]:8.3f}" for c in WIDTHS)
            + f"  best c{best_c} {bb:8.3f} ({bs:5.3f}) = {bb / pb:5.2f} x plain" + ("  bucket wins" if wins else ""))
    say(f"# {group}: the bucket path beats the plain path by more than the rounds' spread from m = "
        + (f"2^{first_win} and at every larger measured m" if first_win is not None else "never (at the largest measured m it does not)"))
    del d_pt, t_a, t_b, t_ok, q, ok

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", args.out)

#!/usr/bin/env python3
"""tools/verify_zip215_rate.py -- ZIP-215 verification (ed25519_VerifySignature_zip215_*) against the plain call of the same build on
the same inputs.

    python tools/verify_zip215_rate.py [--out profiles/verify_zip215_rate.txt] [--reps 7]

Honest inputs (device-made keys and signatures, 32-byte messages): n = 1 through the host-pointer single call (wall-clock us per call,
median), n = 2^10, 2^12, 2^14, 2^16, 2^20 through the *_dev forms in one process (device events; per size a warm-up of both calls so
that the clocks are up, then --reps rounds in which plain and ZIP-215 alternate, each round the median of --reps calls; the table gives
the median round and the spread of the rounds).  At 2^20 two hostile mixes against the honest ZIP-215 time: every second key off the
curve, every R one of the 14 small-order encodings.  Needs the GPU; there is no CPU fallback."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_zip215_rate.txt"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("verify_zip215_rate: no GPU")
    from curve25519_amd import api
    import strict_cases as sc
    from vectors import small_order_encodings
    rng = np.random.default_rng(0x215EED)
    lines = [f"# tools/verify_zip215_rate.py on {torch.cuda.get_device_name(0)}; {a.reps} rounds, plain and ZIP-215 alternating, "
             f"each the median of {a.reps} calls; [min .. max] over the rounds"]

    def dev_ms(fn, *args):
        t = []
        for _ in range(a.reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn(*args)
            e.record()
            e.synchronize()
            t.append(s.elapsed_time(e))
        return float(np.median(t))

    def host_us(fn, *args, calls=200):
        for _ in range(20):
            fn(*args)
        t = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn(*args)
            t.append(time.perf_counter() - t0)
        return float(np.median(t)) * 1e6

    N = 1 << 20
    pub, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (N, 32), dtype=np.uint8))
    msg = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    sig = api.ed25519_SignMessage(priv, msg)

    p1 = host_us(api.ed25519_VerifySignature, sig[:1], pub[:1], msg[:1])
    z1 = host_us(api.ed25519_VerifySignature_zip215, sig[:1], pub[:1], msg[:1])
    p1b = host_us(api.ed25519_VerifySignature, sig[:1], pub[:1], msg[:1])
    lines.append(f"n = 1 (host call, us):   plain {p1:8.1f} / {p1b:8.1f}   ZIP-215 {z1:8.1f}   ZIP-215 - plain {z1 - min(p1, p1b):+6.1f} us")
    lines.append(f"{'n':>8} {'plain ms':>10} {'[min .. max]':>19} {'zip215 ms':>10} {'[min .. max]':>19} {'plain M/s':>10} {'zip215 M/s':>11} "
                 f"{'zip215/plain rate':>18}")

    def tensors(s, p, m):
        return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (s, p, m)]

    def rounds(t, n, reps):
        out = torch.empty((n, 1), dtype=torch.int32, device="cuda")
        for _ in range(3):                                                       # clock ramp-up, on both calls
            api.ed25519_VerifySignature_dev(out, *t)
            api.ed25519_VerifySignature_zip215_dev(out, *t)
        tp, tz = [], []
        for _ in range(reps):
            tp.append(dev_ms(api.ed25519_VerifySignature_dev, out, *t))
            tz.append(dev_ms(api.ed25519_VerifySignature_zip215_dev, out, *t))
        assert int(out.sum()) >= 0
        return tp, tz

    honest_zip = None
    for k in (10, 12, 14, 16, 20):
        n = 1 << k
        tp, tz = rounds(tensors(sig[:n], pub[:n], msg[:n]), n, a.reps)
        mp, mz = float(np.median(tp)), float(np.median(tz))
        lines.append(f"{'2^%d' % k:>8} {mp:10.3f} [{min(tp):7.3f} .. {max(tp):7.3f}] {mz:10.3f} [{min(tz):7.3f} .. {max(tz):7.3f}] "
                     f"{n / mp / 1e3:10.1f} {n / mz / 1e3:11.1f} {mp / mz:18.3f}")
        if k == 20:
            honest_zip = mz
    lines.append("hostile mixes at 2^20 (time relative to the honest inputs' ZIP-215 time):")
    encs = np.stack([np.frombuffer(e, np.uint8) for e, _ in small_order_encodings()])
    hs, hp = sc.hostile(sig, pub, "offcurve")
    rs = sig.copy()
    rs[:, :32] = encs[np.arange(N) % len(encs)]
    for name, (s, p) in (("every second key off the curve", (hs, hp)), ("every R a small-order encoding", (rs, pub))):
        tp, tz = rounds(tensors(s, p, msg), N, 3)
        mp, mz = float(np.median(tp)), float(np.median(tz))
        lines.append(f"  {name}: ZIP-215 {mz:8.3f} ms ({mz / honest_zip:5.2f} x)   plain {mp:8.3f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

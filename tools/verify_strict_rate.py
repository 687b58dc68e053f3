#!/usr/bin/env python3
"""tools/verify_strict_rate.py -- strict verification (ed25519_VerifySignature_strict_*) against the plain call on the same inputs.

    python tools/verify_strict_rate.py [--out profiles/verify_strict_rate.txt] [--reps 7]

Honest inputs (device-made keys and signatures, 32-byte messages): n = 1 through the host-pointer single call (wall-clock us per call,
median), n = 2^10, 2^14, 2^16, 2^20 through the *_dev forms (device events, median of --reps calls; plain and strict alternate).  At 2^20
three hostile mixes, for both calls: every second key off the curve, every S replaced by S + L, every key of small order.  Then
ed25519_Verify_Check_strict against ed25519_Verify_Check on one honest context (n = 1 wall-clock, 2^10, 2^16 and 2^20 device time): the
difference is k_ed25519_verify_check_strict_mask, behind the plain kernels (each workgroup's key check and the per-pair rules).  Needs the GPU; there is no CPU fallback."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_strict_rate.txt"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("verify_strict_rate: no GPU")
    from curve25519_amd import api
    import strict_cases as sc
    rng = np.random.default_rng(0x5EED)
    lines = [f"# tools/verify_strict_rate.py on {torch.cuda.get_device_name(0)}; medians of {a.reps} calls, plain and strict alternating"]

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

    # single call
    p1 = host_us(api.ed25519_VerifySignature, sig[:1], pub[:1], msg[:1])
    s1 = host_us(api.ed25519_VerifySignature_strict, sig[:1], pub[:1], msg[:1])
    p1b = host_us(api.ed25519_VerifySignature, sig[:1], pub[:1], msg[:1])
    lines.append(f"n = 1 (host call, us):   plain {min(p1, p1b):8.1f}   strict {s1:8.1f}   strict - plain {s1 - min(p1, p1b):+6.1f} us")
    lines.append(f"{'n':>8} {'plain ms':>10} {'strict ms':>10} {'plain M/s':>10} {'strict M/s':>11} {'strict/plain rate':>18}")

    def tensors(s, p, m):
        return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (s, p, m)]

    for k in (10, 14, 16, 20):
        n = 1 << k
        t = tensors(sig[:n], pub[:n], msg[:n])
        out = torch.empty((n, 1), dtype=torch.int32, device="cuda")
        for _ in range(2):
            api.ed25519_VerifySignature_dev(out, *t)
            api.ed25519_VerifySignature_strict_dev(out, *t)
        tp, ts = [], []
        for _ in range(a.reps):
            tp.append(dev_ms(api.ed25519_VerifySignature_dev, out, *t))
            ts.append(dev_ms(api.ed25519_VerifySignature_strict_dev, out, *t))
        mp, ms = float(np.median(tp)), float(np.median(ts))
        lines.append(f"{'2^%d' % k:>8} {mp:10.3f} {ms:10.3f} {n / mp / 1e3:10.1f} {n / ms / 1e3:11.1f} {mp / ms:18.3f}")
        if k == 20:
            honest_plain, honest_strict = mp, ms
    lines.append("hostile mixes at 2^20 (time relative to the honest inputs' time of the same call):")
    for kind in ("offcurve", "s_plus_l", "small_key"):
        hs, hp = sc.hostile(sig, pub, kind)
        t = tensors(hs, hp, msg)
        out = torch.empty((N, 1), dtype=torch.int32, device="cuda")
        api.ed25519_VerifySignature_dev(out, *t)
        api.ed25519_VerifySignature_strict_dev(out, *t)
        mp = float(np.median([dev_ms(api.ed25519_VerifySignature_dev, out, *t) for _ in range(3)]))
        ms = float(np.median([dev_ms(api.ed25519_VerifySignature_strict_dev, out, *t) for _ in range(3)]))
        lines.append(f"  {kind:>10}: plain {mp:8.3f} ms ({mp / honest_plain:5.2f} x)   strict {ms:8.3f} ms ({ms / honest_strict:5.2f} x)")

    lines.append("ed25519_Verify_Check_strict vs ed25519_Verify_Check, one honest context:")
    ctx = api.ed25519_Verify_Init(pub[:1])[0]
    csig = api.ed25519_SignMessage(np.repeat(priv[:1], N, 0), msg)
    p1 = host_us(api.ed25519_Verify_Check, ctx, csig[:1], msg[:1])
    s1 = host_us(api.ed25519_Verify_Check_strict, ctx, csig[:1], msg[:1])
    lines.append(f"  n = 1 (host call, us): plain {p1:8.1f}   strict {s1:8.1f}   strict - plain {s1 - p1:+6.1f} us")
    dctx = torch.from_numpy(ctx[None, :].copy()).cuda()

    def check_dev(out, s, m):
        api._lib.check(api._lib.load().ed25519_Verify_Check_dev(out.data_ptr(), dctx.data_ptr(), s.data_ptr(), m.data_ptr(), 32, s.shape[0],
                                                                torch.cuda.current_stream().cuda_stream), "ed25519_Verify_Check_dev")

    for k in (10, 16, 20):
        n = 1 << k
        s, m = (torch.from_numpy(np.ascontiguousarray(x[:n])).cuda() for x in (csig, msg))
        out = torch.empty((n, 1), dtype=torch.int32, device="cuda")
        check_dev(out, s, m)
        api.ed25519_Verify_Check_strict_dev(out, dctx, s, m)
        mp = float(np.median([dev_ms(check_dev, out, s, m) for _ in range(3)]))
        ms = float(np.median([dev_ms(api.ed25519_Verify_Check_strict_dev, out, dctx, s, m) for _ in range(3)]))
        lines.append(f"  2^{k}: plain {mp:8.3f} ms   strict {ms:8.3f} ms   strict - plain {(ms - mp) * 1e3:+7.1f} us")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

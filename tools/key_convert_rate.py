#!/usr/bin/env python3
"""tools/key_convert_rate.py -- ed25519_ClassifyKey_dev, ed25519_PublicKey_to_X25519_dev and ed25519_PrivateKey_to_X25519_dev at
2^10, 2^14, 2^16 and 2^20 keys per call, with ed25519_VerifySignature_dev of the same build on honest signatures beside them as a
scale (the key calls walk [L]A, 252 doublings and 45 additions; verification walks ~134 doublings over window tables), and the
latency of a call of ONE key.  HIP events in one process, inputs resident in HBM, the calls in turn on the same inputs, the best of
a few rounds after a warm-up round.  The keys are honest public keys with one mixed-order key in eight (every lane does the same
work whatever its key: the walk does not depend on the data).  Writes profiles/key_convert_rate.txt (--out)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from curve25519_amd import _lib, api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="10,14,16,20")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--single-calls", type=int, default=200)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_convert_rate.txt"))
args = ap.parse_args()

L = _lib.load()
dev = torch.device("cuda", 0)
NS = [1 << int(s) for s in args.sizes.split(",")]
NMAX = max(NS)
MSG = 32
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


seeds = synth.random_bytes((NMAX, 32), 0x6b01)
msg = synth.random_bytes((NMAX, MSG), 0x6b02)
pub, priv = api.ed25519_CreateKeyPair(seeds)
sig = api.ed25519_SignMessage(priv, msg)
keys = pub.copy()
from key_model import mixed_order_keys  # noqa: E402  (the test model's A + T: inputs only, nothing is judged here)
mixed = np.stack([np.frombuffer(k, np.uint8) for k in mixed_order_keys(pub[:8])])
keys[7::8] = mixed[np.arange(len(keys[7::8])) % len(mixed)]
d_keys, d_pub, d_priv = (torch.from_numpy(a).to(dev) for a in (keys, pub, priv))
d_sig, d_msg = torch.from_numpy(sig).to(dev), torch.from_numpy(msg).to(dev)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731


def ev_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)


def calls(n):
    flags = torch.empty((n, 1), dtype=torch.int32, device=dev)
    ok = torch.empty((n, 1), dtype=torch.int32, device=dev)
    xpk = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    xsk = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    verdict = torch.empty((n, 1), dtype=torch.int32, device=dev)
    keep = (flags, ok, xpk, xsk, verdict)
    return keep, {
        "classify": lambda: _lib.check(L.ed25519_ClassifyKey_dev(p(flags), p(d_keys), n, stream()), "ClassifyKey_dev"),
        "public": lambda: _lib.check(L.ed25519_PublicKey_to_X25519_dev(p(xpk), p(ok), p(d_keys), n, stream()), "PublicKey_to_X25519_dev"),
        "private": lambda: _lib.check(L.ed25519_PrivateKey_to_X25519_dev(p(xsk), p(d_priv), n, stream()), "PrivateKey_to_X25519_dev"),
        "verify": lambda: _lib.check(L.ed25519_VerifySignature_dev(p(verdict), p(d_sig), p(d_pub), p(d_msg), MSG, n, stream()),
                                     "VerifySignature_dev"),
    }


say(f"# tools/key_convert_rate.py on {torch.cuda.get_device_name(0)}: n keys per call, honest keys with one mixed-order key in eight; "
    f"best of {args.rounds} rounds, the four calls in turn on the same inputs; ms per call | M/s; x = rate against VerifySignature_dev")
say(f"{'n':>6} {'ClassifyKey_dev':>22} {'x':>5} {'PublicKey_to_X25519_dev':>24} {'x':>5} {'PrivateKey_to_X25519_dev':>25} "
    f"{'VerifySignature_dev':>22}")
for n in NS:
    keep, vs = calls(n)
    best = {name: 1e9 for name in vs}
    for r in range(args.rounds + 1):                           # (the first round warms up and is not counted)
        for name, f in vs.items():
            t = ev_ms(f)
            if r:
                best[name] = min(best[name], t)
    flags, ok, xpk, xsk, verdict = keep
    f = flags.cpu().numpy().reshape(n)
    want = np.full(n, 11, np.int32)
    want[7::8] = 3
    assert np.array_equal(f, want) and np.array_equal(ok.cpu().numpy().reshape(n), (want == 11).astype(np.int32))
    assert verdict.cpu().numpy().all()
    lg = n.bit_length() - 1
    cell = lambda t: f"{t:8.3f} ms {n / t / 1e3:8.2f}"  # noqa: E731
    say(f"{'2^%d' % lg:>6} {cell(best['classify']):>22} {best['verify'] / best['classify']:5.2f} {cell(best['public']):>24} "
        f"{best['verify'] / best['public']:5.2f} {cell(best['private']):>25} {cell(best['verify']):>22}")

say("# a call of ONE key (device pointers, one synchronise per call, host clock): median | best, microseconds")
import time  # noqa: E402
_, one = calls(1)
for name, label in (("classify", "ed25519_ClassifyKey_dev"), ("public", "ed25519_PublicKey_to_X25519_dev"),
                    ("private", "ed25519_PrivateKey_to_X25519_dev"), ("verify", "ed25519_VerifySignature_dev")):
    ts = []
    for i in range(args.single_calls + 10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one[name]()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts = np.sort(np.array(ts[10:]))
    say(f"{label:>34} {ts[len(ts) // 2]:9.1f} | {ts[0]:9.1f}")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", args.out)

#!/usr/bin/env python3
"""tools/vrf_rate.py -- the ECVRF calls (ed25519_VRF_Prove_dev, ed25519_VRF_Verify_dev, ed25519_VRF_ProofToHash_dev) at 2^10 .. 2^20
elements per call over alpha of 32 bytes, with two scales of the same build on the same inputs in the same process beside them:
  * the COMPOSED device sequence a caller had before -- ed25519_EncodeToCurve_dev on pk || alpha, ed25519_ScalarMult_noclamp_dev twice
    (Gamma, V), ed25519_ScalarMultBase_noclamp_dev (U), ed25519_ScalarMulAdd_dev (s) -- WITHOUT its three host hashes (x, k and c are
    random scalars here: the device work does not depend on their values) and without the copies between host and device those
    hashes would need;
  * ed25519_ScalarMult_noclamp_dev alone: one variable-base walk with its shared inversion.
By operation count Prove is one EncodeToCurve, two variable-base walks over one table, a comb walk and two inversions; Verify one
EncodeToCurve, one full-length and two half-length walks, a comb walk and two inversions at one wave per SIMD.  HIP events in one
process, inputs resident in HBM, the calls in turn in interleaved rounds after a warm-up round, every figure `launches` calls back to
back: best and spread (slowest less fastest round) per call.  Writes profiles/vrf_rate.txt (--out)."""
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
ap.add_argument("--sizes", default="10,12,14,16,18,20")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--launches", type=int, default=2)
ap.add_argument("--alpha-size", type=int, default=32)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vrf_rate.txt"))
args = ap.parse_args()

L = _lib.load()
dev = torch.device("cuda", 0)
NS = [1 << int(s) for s in args.sizes.split(",")]
NMAX = max(NS)
ALPHA = args.alpha_size
DST = b"ECVRF_" + b"edwards25519_XMD:SHA-512_ELL2_NU_" + b"\x04"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


pub, priv = api.ed25519_CreateKeyPair(synth.random_bytes((NMAX, 32), 0x9381))
alpha = synth.random_bytes((NMAX, ALPHA), 0x9382)
scalars = synth.random_bytes((3, NMAX, 32), 0x9383)
scalars[:, :, 31] &= 0x0f                                       # below 2^252: canonical
to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
d_pub, d_priv, d_alpha = to_dev(pub), to_dev(priv), to_dev(alpha)
d_msg = to_dev(np.concatenate([pub, alpha], axis=1))
d_x, d_k, d_c = (to_dev(s) for s in scalars)
d_proof = torch.empty((NMAX, 80), dtype=torch.uint8, device=dev)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

# what is timed is what is tested: the proofs verify, Verify and ProofToHash agree, and another key's proof is refused
api.ed25519_VRF_Prove_dev(d_proof, d_priv, d_alpha)
torch.cuda.synchronize()
chk = d_proof[:256].cpu().numpy()
beta, ok = api.ed25519_VRF_Verify(pub[:256], chk, alpha[:256])
beta2, ok2 = api.ed25519_VRF_ProofToHash(chk)
assert ok.all() and ok2.all() and np.array_equal(beta, beta2)
assert not api.ed25519_VRF_Verify(np.roll(pub[:256], 1, axis=0), chk, alpha[:256])[1].any()


def ev_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.launches):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.launches


def calls(n):
    u8 = lambda w=32: torch.empty((n, w), dtype=torch.uint8, device=dev)  # noqa: E731
    q_h, q_g, q_u, q_v, q_s, q_pi, q_beta = u8(), u8(), u8(), u8(), u8(), u8(80), u8(64)
    q_ok = torch.empty((n, 1), dtype=torch.int32, device=dev)
    st = stream

    def composed():
        _lib.check(L.ed25519_EncodeToCurve_dev(p(q_h), p(d_msg), 32 + ALPHA, DST, len(DST), n, st()), "encode")
        _lib.check(L.ed25519_ScalarMult_noclamp_dev(p(q_g), p(q_ok), p(d_x), p(q_h), n, st()), "gamma")
        _lib.check(L.ed25519_ScalarMultBase_noclamp_dev(p(q_u), p(d_k), n, st()), "u")
        _lib.check(L.ed25519_ScalarMult_noclamp_dev(p(q_v), p(q_ok), p(d_k), p(q_h), n, st()), "v")
        _lib.check(L.ed25519_ScalarMulAdd_dev(p(q_s), p(d_c), p(d_x), p(d_k), n, st()), "s")

    out = {
        "ed25519_VRF_Prove": lambda: _lib.check(L.ed25519_VRF_Prove_dev(p(q_pi), p(d_priv), p(d_alpha), ALPHA, n, st()), "prove"),
        "composed sequence (no host hashes)": composed,
        "ed25519_VRF_Verify": lambda: _lib.check(L.ed25519_VRF_Verify_dev(p(q_beta), p(q_ok), p(d_pub), p(d_proof), p(d_alpha), ALPHA, n, st()),
                                                 "verify"),
        "ed25519_VRF_ProofToHash": lambda: _lib.check(L.ed25519_VRF_ProofToHash_dev(p(q_beta), p(q_ok), p(d_proof), n, st()), "proof_to_hash"),
        "ed25519_ScalarMult_noclamp": lambda: _lib.check(L.ed25519_ScalarMult_noclamp_dev(p(q_g), p(q_ok), p(d_x), p(d_pub), n, st()), "mult"),
    }
    return (q_h, q_g, q_u, q_v, q_s, q_pi, q_beta, q_ok), out


say(f"# tools/vrf_rate.py on {torch.cuda.get_device_name(0)}: n elements per call, alpha of {ALPHA} bytes; {args.rounds} interleaved rounds "
    f"of {args.launches} launches back to back, every call in turn on the same inputs; best ms per call (spread ms) | M/s; "
    f"x = time against the composed sequence of the same build beside it")
at_max, spread_max = {}, {}
for n in NS:
    keep, vs = calls(n)
    times = {name: [] for name in vs}
    for r in range(args.rounds + 1):                           # (the first round warms up and is not counted)
        for name, f in vs.items():
            t = ev_ms(f)
            if r:
                times[name].append(t)
    say(f"n = 2^{n.bit_length() - 1}")
    ref = min(times["composed sequence (no host hashes)"])
    for name, ts in times.items():
        best, spread = min(ts), max(ts) - min(ts)
        say(f"  {name:>36} {best:9.3f} ms ({spread:6.3f}) {n / best / 1e3:9.2f} M/s  x {best / ref:5.2f}")
    if n == NMAX:
        at_max = {name: min(ts) for name, ts in times.items()}
        spread_max = {name: max(ts) - min(ts) for name, ts in times.items()}

comp, mult = at_max["composed sequence (no host hashes)"], at_max["ed25519_ScalarMult_noclamp"]
say(f"# at n = 2^{NMAX.bit_length() - 1}, against the composed sequence ({comp:.3f} ms, spread {spread_max['composed sequence (no host hashes)']:.3f}) "
    f"and ed25519_ScalarMult_noclamp_dev ({mult:.3f} ms):")
for name in ("ed25519_VRF_Prove", "ed25519_VRF_Verify", "ed25519_VRF_ProofToHash"):
    ms = at_max[name]
    say(f"#   {name:>24} {ms:8.3f} ms (spread {spread_max[name]:.3f}) = {ms / comp:5.2f} x composed, {ms / mult:5.2f} x ScalarMult_noclamp, "
        f"{NMAX / ms / 1e3:.1f} M/s")
worst = max(spread_max["ed25519_VRF_Prove"], spread_max["composed sequence (no host hashes)"])
verdict = "not slower than" if at_max["ed25519_VRF_Prove"] <= comp + worst else "SLOWER than"
say(f"# Prove is {verdict} the composed sequence by more than the rounds' spread ({at_max['ed25519_VRF_Prove'] - comp:+.3f} ms, spread {worst:.3f})")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", args.out)

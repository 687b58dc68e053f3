#!/usr/bin/env python3
"""tools/one_peer_rate.py -- many X25519 secrets against ONE peer key (curve25519_dh_CreateSharedKey_one_peer_dev) against the
ladder on the same inputs (curve25519_dh_CreateSharedKey_dev with the key repeated).  Per size, device-resident calls timed with
HIP events in one process (best of several):
  remembered  the peer's comb was built by an earlier call: the walk alone (+ one lane asking whether the key is the kept one)
  fresh       every call builds the comb for a new peer first (ONE_PEER_WIDE = 1, two peers in turn): what ONE_PEER_WIDE weighs
  fallback    a twist peer while another peer's comb is kept: the device says no and the ladder runs (must cost what the ladder does)
  ladder      curve25519_dh_CreateSharedKey_dev
The break-even line at the end is the smallest size from which a fresh comb beats the ladder: ONE_PEER_WIDE's default."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from curve25519_amd import _lib, api, synth  # noqa: E402

L = _lib.load()
dev = torch.device("cuda", 0)
big = 1 << 22
sk_host = synth.random_bytes((big, 32), 0x0ef1)
d_sk = torch.from_numpy(sk_host).to(dev)
d_out = torch.empty_like(d_sk)


def pub(seed):
    return api.curve25519_dh_CalculatePublicKey(synth.random_bytes((1, 32), seed))[0]


peers = [torch.from_numpy(pub(s)).to(dev) for s in (0x0ef2, 0x0ef3, 0x0ef4)]
twist = torch.from_numpy(np.frombuffer((2).to_bytes(32, "little"), np.uint8).reshape(1, 32).copy()).to(dev)
d_rep = peers[0].repeat(big, 1)
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def one_peer(pk, n):
    _lib.check(L.curve25519_dh_CreateSharedKey_one_peer_dev(p(d_out), p(pk), p(d_sk), n, st()), "one_peer_dev")


def ladder(n):
    _lib.check(L.curve25519_dh_CreateSharedKey_dev(p(d_out), p(d_rep), p(d_sk), n, st()), "CreateSharedKey_dev")


def best_ms(f, reps):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


# the inputs are clamped in place by the first call; every later call sees the same (clamped) secrets
ladder(big)
torch.cuda.synchronize()
print(f"# tools/one_peer_rate.py on {torch.cuda.get_device_name(0)}: X25519 with ONE peer key, device-resident calls, best of N; ms per call | M ops/s")
print(f"{'n':>6} {'remembered comb':>24} {'fresh comb':>24} {'fallback (twist)':>24} {'ladder (_dev)':>24} {'x remembered':>12} {'x fresh':>8}")
rows = []
turn = [0]
for n in [1 << lg for lg in range(10, 17)] + [3 << 15] + [1 << lg for lg in range(17, 23)]:
    reps = 20 if n < 1 << 20 else 8
    with _lib.tunable("ONE_PEER_WIDE", 1):
        one_peer(peers[0], n)                                    # build and remember peer 0's comb
        torch.cuda.synchronize()
    rem = best_ms(lambda: one_peer(peers[0], n), reps)
    wide_rem = L.c25519_amd_x25519_one_peer_last_wide()

    def fresh_call():
        turn[0] ^= 1
        one_peer(peers[1 + turn[0]], n)
    with _lib.tunable("ONE_PEER_WIDE", 1):
        fresh = best_ms(fresh_call, reps)
        wide_fresh = L.c25519_amd_x25519_one_peer_last_wide()
        one_peer(peers[0], n)                                    # peer 0's comb kept again for the fallback row
        torch.cuda.synchronize()
    fb = best_ms(lambda: one_peer(twist, n), reps)
    wide_fb = L.c25519_amd_x25519_one_peer_last_wide()
    lad = best_ms(lambda: ladder(n), reps)
    want_rem = 1 if n > 3584 else 0                              # (per-wave sizes run the ladder unless a comb is built)
    assert (wide_rem, wide_fresh, wide_fb) == (want_rem, 1, 0), (n, wide_rem, wide_fresh, wide_fb)
    cell = lambda ms: f"{ms:8.3f} ms {n / ms / 1e3:9.1f} M/s"  # noqa: E731
    print(f"{n if n & (n - 1) else '2^' + str(n.bit_length() - 1):>6} {cell(rem):>24} {cell(fresh):>24} {cell(fb):>24} {cell(lad):>24} {lad / rem:12.2f} {lad / fresh:8.2f}")
    rows.append((n, rem, fresh, fb, lad))
be = next((n for n, _, fresh, _, lad in rows if fresh < lad and all(f < l for m, _, f, _, l in rows if m >= n)), None)
print(f"# break-even: a fresh comb beats the ladder from n = {be} on" if be else "# break-even: none in range")
print("# (remembered at the per-wave sizes, <= 3584, is the ladder: those calls never ask the device)")

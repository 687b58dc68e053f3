#!/usr/bin/env python3
"""tools/peer_indexed_rate.py -- curve25519_dh_CreateSharedKey_indexed_dev (n secrets against K peer contexts in one call, element i
against context ctx_index[i]) against what a caller without it runs: curve25519_dh_CreateSharedKey_dev on the same secrets with the
keys gathered (pk[idx]).  Rows: n = 2^12 .. 2^20 secrets crossed with K = 1, 64, 4096, 65536 contexts, indices uniformly random and
the same indices sorted.  Columns (HIP events in one process, inputs resident in HBM, the variants called in turn on the same inputs
and the best of a few rounds kept): the product call; the same call with PEER_INDEXED_MIN = 0 (always the walk over the contexts'
rows) and with PEER_INDEXED_MIN = 2^30 (always gather + the ladder paths); CreateSharedKey_dev; product / ladder.  The crossover
between the two forced columns sets PEER_INDEXED_MIN.  Last: curve25519_dh_Peer_Init_dev contexts per second."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from curve25519_amd import _lib, api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="12,14,15,16,18,20")
ap.add_argument("--ns", default="", help="explicit call sizes (elements) instead of --sizes")
ap.add_argument("--ks", default="1,64,4096,65536")
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()

L = _lib.load()
dev = torch.device("cuda", 0)
KMAX = max(int(k) for k in args.ks.split(","))
NS = [int(x) for x in args.ns.split(",")] if args.ns else [1 << int(s) for s in args.sizes.split(",")]
NMAX = max(NS)
pub, _ = api.curve25519_dh_CalculatePublicKey(synth.random_bytes((KMAX, 32), 0x2ec0))
d_pub = torch.from_numpy(pub).to(dev)
d_ctxs = torch.empty((KMAX, 1600), dtype=torch.uint8, device=dev)
api.curve25519_dh_Peer_Init_dev(d_ctxs, d_pub)
sk_all = torch.from_numpy(synth.random_bytes((NMAX, 32), 0x2ec1)).to(dev)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731


def ev_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)


def variants(k, d_idx, d_pk, n):
    """name -> (tunable value or None, the call); every call works on a fresh copy of the secrets (they are clamped in place)"""
    out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    sk = torch.empty_like(out)

    def indexed():
        _lib.check(L.curve25519_dh_CreateSharedKey_indexed_dev(p(out), p(d_ctxs), k, p(d_idx), p(sk), n, stream()), "indexed_dev")

    def ladder():
        _lib.check(L.curve25519_dh_CreateSharedKey_dev(p(out), p(d_pk), p(sk), n, stream()), "CreateSharedKey_dev")
    return out, sk, {"indexed": (None, indexed), "walk": (0, indexed), "gather": (1 << 30, indexed), "ladder": (None, ladder)}


print(f"# tools/peer_indexed_rate.py on {torch.cuda.get_device_name(0)}: n secrets against K peer contexts (public keys of random "
      f"secrets); best of {args.rounds} rounds, the four calls in turn on the same inputs; ms per call | M/s")
print(f"{'n':>6} {'K':>6} {'order':>7} {'indexed _dev':>22} {'walk (MIN=0)':>22} {'gather (MIN=2^30)':>22} {'CreateSharedKey_dev':>22} "
      f"{'x':>5}")
for n in NS:
    lg = n.bit_length() - 1
    label = f"2^{lg}" if n == 1 << lg else str(n)
    for k in (int(x) for x in args.ks.split(",")):
        for sort in (False, True):
            idx = np.random.default_rng(0x2ec2 + k + lg).integers(0, k, n).astype(np.uint32)
            if sort:
                idx = np.sort(idx)
            d_idx = torch.from_numpy(idx.view(np.int32).reshape(n, 1)).to(dev)
            d_pk = d_pub[torch.from_numpy(idx.astype(np.int64)).to(dev)].contiguous()
            out, sk, vs = variants(k, d_idx, d_pk, n)
            best = {name: 1e9 for name in vs}
            ref = None
            for r in range(args.rounds + 1):                   # (the first round warms up and is not counted)
                for name, (knob, f) in vs.items():
                    sk.copy_(sk_all[:n])
                    with _lib.tunable("PEER_INDEXED_MIN", knob if knob is not None else -1):
                        t = ev_ms(f)
                    if ref is None:
                        ref = out.clone()
                    assert torch.equal(out, ref), (name, n, k)
                    if r:
                        best[name] = min(best[name], t)
            cell = lambda t: f"{t:8.3f} ms {n / t / 1e3:7.1f}"  # noqa: E731
            print(f"{label:>6} {k:>6} {'sorted' if sort else 'random':>7} {cell(best['indexed']):>22} {cell(best['walk']):>22} "
                  f"{cell(best['gather']):>22} {cell(best['ladder']):>22} {best['ladder'] / best['indexed']:5.2f}", flush=True)

print("# curve25519_dh_Peer_Init_dev: contexts per call | ms | contexts/s")
for k in (4096, 65536):
    if k > KMAX:
        continue
    t = min(ev_ms(lambda: api.curve25519_dh_Peer_Init_dev(d_ctxs[:k], d_pub[:k])) for _ in range(4))
    print(f"{k:>8} {t:8.3f} ms {k / t * 1e3 / 1e6:8.3f} M/s", flush=True)

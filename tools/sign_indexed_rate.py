#!/usr/bin/env python3
"""tools/sign_indexed_rate.py -- ed25519_SignMessage_indexed_* (many Sign_Init contexts in one call, message i under context
ctx_index[i]) against what a caller without it runs: ed25519_SignMessage_* on the gathered private keys priv[idx].
Rows: n = 1, 2^10, 2^12, 2^14, 2^16, 2^20 messages of 32 bytes crossed with K = 1, 64, 4096, 65536 contexts, indices uniformly random.
Columns: the indexed _dev call and SignMessage_dev on the gathered keys (HIP events, inputs resident in HBM, the two calls alternating
in the same process, best of several), their ratio; then the two host-pointer _batch forms (wall clock, best of three): the
indexed one moves 4 + 32 + 64 bytes per element and uploads the K contexts every call (8.4 MB at K = 65536), SignMessage_batch
moves 64 + 32 + 64.  Every output is checked against SignMessage's bytes."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from curve25519_amd import _lib, api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="0,10,12,14,16,20", help="log2 of the call sizes")
ap.add_argument("--ks", default="1,64,4096,65536")
args = ap.parse_args()

L = _lib.load()
dev = torch.device("cuda", 0)
KMAX = max(int(k) for k in args.ks.split(","))
NMAX = 1 << max(int(s) for s in args.sizes.split(","))
_, priv = api.ed25519_CreateKeyPair(synth.random_bytes((KMAX, 32), 0x5ec0))
ctxs = api.ed25519_Sign_Init(priv)
d_ctxs = torch.from_numpy(ctxs).to(dev)
d_priv = torch.from_numpy(priv).to(dev)
msg = synth.random_bytes((NMAX, 32), 0x5ec1)
d_msg_all = torch.from_numpy(msg).to(dev)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731


def ev_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall_ms(f):
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter(); out = f()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, out


print(f"# tools/sign_indexed_rate.py on {torch.cuda.get_device_name(0)}: n messages of 32 bytes under K Sign_Init contexts, random "
      f"indices; ms per call | M signatures/s")
print(f"{'n':>6} {'K':>6} {'indexed _dev':>24} {'SignMessage_dev gathered':>26} {'x':>5} {'indexed _batch':>24} "
      f"{'SignMessage_batch':>24} {'x':>5}")
for lg in (int(s) for s in args.sizes.split(",")):
    n = 1 << lg
    reps = 10 if n >= 1 << 16 else 30
    for k in (int(x) for x in args.ks.split(",")):
        idx = np.random.default_rng(0x5ec2 + k + lg).integers(0, k, n).astype(np.uint32)
        d_idx = torch.from_numpy(idx.view(np.int32)).to(dev)
        d_msg = d_msg_all[:n]
        d_pk = d_priv[torch.from_numpy(idx.astype(np.int64)).to(dev)].contiguous()
        s_idx = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        s_gat = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        f_idx = lambda: _lib.check(L.ed25519_SignMessage_indexed_dev(p(s_idx), p(d_ctxs), k, p(d_idx), p(d_msg), 32, n, stream()),  # noqa: E731
                                   "ed25519_SignMessage_indexed_dev")
        f_gat = lambda: _lib.check(L.ed25519_SignMessage_dev(p(s_gat), p(d_pk), p(d_msg), 32, n, stream()),  # noqa: E731
                                   "ed25519_SignMessage_dev")
        for _ in range(3):
            f_idx(); f_gat()
        torch.cuda.synchronize()
        t_idx = t_gat = 1e9
        for _ in range(reps):
            t_idx = min(t_idx, ev_ms(f_idx))
            t_gat = min(t_gat, ev_ms(f_gat))
        assert torch.equal(s_idx, s_gat), (n, k)
        sub = ctxs[:k]
        t_bi, sig_bi = wall_ms(lambda: api.ed25519_SignMessage_indexed(sub, idx, msg[:n]))
        pk_host = priv[idx]
        t_bs, sig_bs = wall_ms(lambda: api.ed25519_SignMessage(pk_host, msg[:n]))
        assert np.array_equal(sig_bi, sig_bs) and np.array_equal(sig_bs, s_gat.cpu().numpy()), (n, k)
        cell = lambda t: f"{t:8.3f} ms {n / t / 1e3:8.2f} M/s"  # noqa: E731
        print(f"{'2^' + str(lg):>6} {k:>6} {cell(t_idx):>24} {cell(t_gat):>26} {t_gat / t_idx:5.2f} {cell(t_bi):>24} {cell(t_bs):>24} "
              f"{t_bs / t_bi:5.2f}", flush=True)

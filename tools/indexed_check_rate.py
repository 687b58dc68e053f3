#!/usr/bin/env python3
"""tools/indexed_check_rate.py -- ed25519_Verify_Check_indexed_* (many Verify_Init contexts in one call, element i against context
ctx_index[i]) against what a caller without it runs: ed25519_VerifySignature_dev on the same (sig, pk = pub[idx], msg) triples.
Rows: n = 2^12 .. 2^20 pairs crossed with K = 1, 64, 4096, 65536 contexts, indices uniformly random and the same indices sorted.
Columns: the _dev call (HIP events, best of a few calls, inputs resident in HBM), VerifySignature_dev, their ratio, and the
host-pointer _batch call (wall clock, which uploads the K contexts every call: 136 MB at K = 65536).

--ab GATHER.so REPACK.so: the gather / repack A/B instead (tools/build_variants.sh builds both from engine.hip: the product's
direct gather of the rows, and -DC25519_INDEXED_REPACK=1, which copies the call's rows into 128-byte-aligned scratch first); the two
builds are called alternately on the same inputs at n = 2^20 and 2^16 and must give the same verdicts."""
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
ap.add_argument("--ab", nargs=2, metavar=("GATHER_SO", "REPACK_SO"))
ap.add_argument("--sizes", default="12,14,16,18,20")
ap.add_argument("--ks", default="1,64,4096,65536")
args = ap.parse_args()

L = _lib.load()
dev = torch.device("cuda", 0)
KMAX = max(int(k) for k in args.ks.split(","))
NMAX = 1 << max(int(s) for s in args.sizes.split(","))
pub, priv = api.ed25519_CreateKeyPair(synth.random_bytes((KMAX, 32), 0x1dc0))
ctxs = api.ed25519_Verify_Init(pub)
d_ctxs = torch.from_numpy(ctxs).to(dev)
d_pub = torch.from_numpy(pub).to(dev)
msg = synth.random_bytes((NMAX, 32), 0x1dc1)
d_msg_all = torch.from_numpy(msg).to(dev)
p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731


def ev_ms(f, reps):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def inputs(k, n, seed, sort):
    """indices, signatures (all valid) and messages of n pairs over the first k keys"""
    idx = np.random.default_rng(seed).integers(0, k, n).astype(np.uint32)
    if sort:
        idx = np.sort(idx)
    sig = api.ed25519_SignMessage(priv[idx], msg[:n])
    return idx, sig


def indexed_dev(lib, d_ok, k, d_idx, d_sig, d_msg, n):
    _lib.check(lib.ed25519_Verify_Check_indexed_dev(p(d_ok), p(d_ctxs), k, p(d_idx), p(d_sig), p(d_msg), 32, n, stream()),
               "ed25519_Verify_Check_indexed_dev")


def bind(lib):
    vp, sz = C.c_void_p, C.c_size_t
    lib.ed25519_Verify_Check_indexed_dev.argtypes = [vp, vp, sz, vp, vp, vp, sz, sz, vp]
    return lib


if args.ab:
    libs = [bind(C.CDLL(os.path.abspath(s))) for s in args.ab]
    print(f"# tools/indexed_check_rate.py --ab on {torch.cuda.get_device_name(0)}: ed25519_Verify_Check_indexed_dev, random indices, "
          f"32-byte messages; best of 5 calls, the two builds alternating; ms per call | M pairs/s")
    print(f"{'pairs':>8} {'K':>6} {'gather (rows in place)':>26} {'repack (aligned copy first)':>28} {'repack/gather':>14}")
    for lg in (20, 16):
        n = 1 << lg
        for k in (int(x) for x in args.ks.split(",")):
            idx, sig = inputs(k, n, 0x1dc2 + k, False)
            d_idx, d_sig, d_msg = torch.from_numpy(idx.view(np.int32)).to(dev), torch.from_numpy(sig).to(dev), d_msg_all[:n]
            oks = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in libs]
            ms = [1e9, 1e9]
            for _ in range(5):
                for j, lib in enumerate(libs):
                    ms[j] = min(ms[j], ev_ms(lambda: indexed_dev(lib, oks[j], k, d_idx, d_sig, d_msg, n), 1))
            assert bool(oks[0].all()) and torch.equal(oks[0], oks[1]), (n, k)
            cell = lambda t: f"{t:8.3f} ms {n / t / 1e3:8.1f} M/s"  # noqa: E731
            print(f"{'2^' + str(lg):>8} {k:>6} {cell(ms[0]):>26} {cell(ms[1]):>28} {ms[1] / ms[0]:14.2f}")
    sys.exit(0)

bind(L)
print(f"# tools/indexed_check_rate.py on {torch.cuda.get_device_name(0)}: n pairs against K Verify_Init contexts, 32-byte messages, all "
      f"signatures valid; ms per call | M pairs/s")
print(f"{'pairs':>6} {'K':>6} {'order':>7} {'indexed _dev':>24} {'VerifySignature_dev':>24} {'x':>5} {'indexed _batch':>24}")
for lg in (int(s) for s in args.sizes.split(",")):
    n = 1 << lg
    reps = 5 if n >= 1 << 18 else 10
    for k in (int(x) for x in args.ks.split(",")):
        for sort in (False, True):
            idx, sig = inputs(k, n, 0x1dc2 + k, sort)
            d_idx, d_sig, d_msg = torch.from_numpy(idx.view(np.int32)).to(dev), torch.from_numpy(sig).to(dev), d_msg_all[:n]
            d_pk = d_pub[torch.from_numpy(idx.astype(np.int64)).to(dev)].contiguous()
            d_ok = torch.zeros(n, dtype=torch.int32, device=d_sig.device)
            t_idx = ev_ms(lambda: indexed_dev(L, d_ok, k, d_idx, d_sig, d_msg, n), reps)
            assert bool(d_ok.all()), (n, k)
            d_ok.zero_()
            t_vs = ev_ms(lambda: _lib.check(L.ed25519_VerifySignature_dev(p(d_ok), p(d_sig), p(d_pk), p(d_msg), 32, n, stream()),
                                            "ed25519_VerifySignature_dev"), reps)
            assert bool(d_ok.all()), (n, k)
            ok = api.ed25519_Verify_Check_indexed(ctxs[:k], idx, sig, msg[:n])
            t_b = 1e9
            for _ in range(3):
                t0 = time.perf_counter(); ok = api.ed25519_Verify_Check_indexed(ctxs[:k], idx, sig, msg[:n])
                t_b = min(t_b, (time.perf_counter() - t0) * 1e3)
            assert ok.all(), (n, k)
            cell = lambda t: f"{t:8.3f} ms {n / t / 1e3:7.1f} M/s"  # noqa: E731
            print(f"{'2^' + str(lg):>6} {k:>6} {'sorted' if sort else 'random':>7} {cell(t_idx):>24} {cell(t_vs):>24} {t_vs / t_idx:5.2f} "
                  f"{cell(t_b):>24}", flush=True)

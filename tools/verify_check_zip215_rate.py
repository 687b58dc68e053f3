#!/usr/bin/env python3
"""tools/verify_check_zip215_rate.py -- ed25519_Verify_Check_zip215_* (the ZIP-215 verdict against Verify_Init contexts) against its
ceiling and its bar, on honest inputs through the *_dev forms (HIP events, inputs resident in HBM).

    python tools/verify_check_zip215_rate.py [--out profiles/verify_check_zip215_rate.txt] [--rounds 5]

Per cell (n = 2^10 .. 2^20 pairs over K = 1, 256, 4096, 65536 contexts, random indices, 32-byte messages) three calls on the same
triples, alternating in one process for --rounds rounds (each round one timed call per variant behind a warm-up of all three), min ..
max over the rounds:
  (a) ed25519_Verify_Check_indexed_dev              the plain call: the ceiling, it runs the same walk
  (b) ed25519_VerifySignature_zip215_dev            on the gathered keys: the bar, what a caller without the new call runs
  (c) ed25519_Verify_Check_zip215_indexed_dev       with ZIP215_CHECK_MIN = 0: the context path at every size
Then one context, the comb remembered: ed25519_Verify_Check_dev against ed25519_Verify_Check_zip215_dev (ZIP215_CHECK_MIN = 0).

--trace LOG2N: only run (c) a few times at that size, for `rocprofv3 --kernel-trace --stats -- python tools/... --trace 20`.
--plain-lib SO: only time ed25519_Verify_Check_indexed_dev of that library at 2^20 over K = 4096 and print one line -- for an
interleaved A/B of two builds in fresh processes.  Needs the GPU; there is no CPU fallback."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="10,12,14,16,18,20")
    ap.add_argument("--ks", default="1,256,4096,65536")
    ap.add_argument("--one-sizes", default="12,14,16,20")
    ap.add_argument("--trace", type=int)
    ap.add_argument("--plain-lib")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("verify_check_zip215_rate: no GPU")
    from curve25519_amd import _lib, api, synth
    L = _lib.load()
    dev = torch.device("cuda", 0)
    sizes = [int(s) for s in a.sizes.split(",")]
    ks = [int(k) for k in a.ks.split(",")]
    if a.trace:
        sizes, ks = [a.trace], [4096]
    if a.plain_lib:
        sizes, ks = [20], [4096]
    nmax = 1 << max(sizes + [int(s) for s in a.one_sizes.split(",")])
    pub, priv = api.ed25519_CreateKeyPair(synth.random_bytes((max(ks), 32), 0x21c0))
    ctxs = api.ed25519_Verify_Init(pub)
    d_ctxs, d_pub = torch.from_numpy(ctxs).to(dev), torch.from_numpy(pub).to(dev)
    msg = synth.random_bytes((nmax, 32), 0x21c1)
    d_msg_all = torch.from_numpy(msg).to(dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(f):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); f(); e.record(); e.synchronize()
        return s.elapsed_time(e)

    def rounds(fs):
        """per variant [min, max] of a.rounds timed calls, the variants alternating"""
        for _ in range(2):
            for f in fs:
                f()
        torch.cuda.synchronize()
        t = [[] for _ in fs]
        for _ in range(a.rounds):
            for j, f in enumerate(fs):
                t[j].append(timed(f))
        return [(min(x), max(x)) for x in t]

    def cell(n, t):
        return f"{t[0]:7.3f}..{t[1]:7.3f} ms {n / t[0] / 1e3:6.1f} M/s"

    def inputs(k, n):
        idx = np.random.default_rng(0x21c2 + k).integers(0, k, n).astype(np.uint32)
        sig = api.ed25519_SignMessage(priv[idx], msg[:n])
        return (torch.from_numpy(idx.view(np.int32)).to(dev), torch.from_numpy(sig).to(dev), d_msg_all[:n],
                d_pub[torch.from_numpy(idx.astype(np.int64)).to(dev)].contiguous())

    if a.plain_lib:
        lib = C.CDLL(os.path.abspath(a.plain_lib))
        vp, sz = C.c_void_p, C.c_size_t
        lib.ed25519_Verify_Check_indexed_dev.argtypes = [vp, vp, sz, vp, vp, vp, sz, sz, vp]
        n, k = 1 << 20, 4096
        d_idx, d_sig, d_msg, _ = inputs(k, n)
        d_ok = torch.zeros(n, dtype=torch.int32, device=dev)
        t = rounds([lambda: _lib.check(lib.ed25519_Verify_Check_indexed_dev(p(d_ok), p(d_ctxs), k, p(d_idx), p(d_sig), p(d_msg), 32, n, stream()),
                                       "ed25519_Verify_Check_indexed_dev")])[0]
        assert bool(d_ok.all())
        print(f"{a.plain_lib}: ed25519_Verify_Check_indexed_dev 2^20 K=4096 {cell(n, t)}", flush=True)
        return

    say(f"# tools/verify_check_zip215_rate.py on {torch.cuda.get_device_name(0)}: n pairs against K Verify_Init contexts, random indices, "
        f"32-byte messages, all signatures valid; {a.rounds} rounds, the variants alternating; min..max ms per call | M pairs/s at the min")
    say(f"{'pairs':>6} {'K':>6} {'(a) Verify_Check_indexed':>34} {'(b) VerifySignature_zip215':>34} {'(c) Verify_Check_zip215_indexed':>34} {'c/a':>5} {'b/c':>5}")
    with _lib.tunable("ZIP215_CHECK_MIN", 0):
        for lg in sizes:
            n = 1 << lg
            for k in ks:
                d_idx, d_sig, d_msg, d_pk = inputs(k, n)
                oks = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3)]
                fa = lambda: _lib.check(L.ed25519_Verify_Check_indexed_dev(p(oks[0]), p(d_ctxs), k, p(d_idx), p(d_sig), p(d_msg), 32, n, stream()), "a")  # noqa: E731
                fb = lambda: _lib.check(L.ed25519_VerifySignature_zip215_dev(p(oks[1]), p(d_sig), p(d_pk), p(d_msg), 32, n, stream()), "b")  # noqa: E731
                fc = lambda: _lib.check(L.ed25519_Verify_Check_zip215_indexed_dev(p(oks[2]), p(d_ctxs), k, p(d_idx), p(d_sig), p(d_msg), 32, n, stream()), "c")  # noqa: E731
                if a.trace:
                    for _ in range(5):
                        fc()
                    torch.cuda.synchronize()
                    assert bool(oks[2].all())
                    return
                ta, tb, tc = rounds([fa, fb, fc])
                assert all(bool(o.all()) for o in oks), (n, k)
                say(f"{'2^' + str(lg):>6} {k:>6} {cell(n, ta):>34} {cell(n, tb):>34} {cell(n, tc):>34} {ta[0] / tc[0]:5.2f} {tb[0] / tc[0]:5.2f}")
        say("# one context, the comb remembered (a first call of 2^16 pairs builds it): plain ed25519_Verify_Check_dev | ed25519_Verify_Check_zip215_dev")
        say(f"{'pairs':>6} {'Verify_Check_dev':>34} {'Verify_Check_zip215_dev':>34} {'zip215/plain':>12} {'wide':>5}")
        d_idx, d_sig_all, _, _ = inputs(1, nmax)
        d_ctx = d_ctxs[:1]
        warm = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
        _lib.check(L.ed25519_Verify_Check_dev(p(warm), p(d_ctx), p(d_sig_all), p(d_msg_all), 32, 1 << 16, stream()), "warm")
        for lg in (int(s) for s in a.one_sizes.split(",")):
            n = 1 << lg
            oks = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)]
            fp = lambda: _lib.check(L.ed25519_Verify_Check_dev(p(oks[0]), p(d_ctx), p(d_sig_all), p(d_msg_all), 32, n, stream()), "plain")  # noqa: E731
            fz = lambda: _lib.check(L.ed25519_Verify_Check_zip215_dev(p(oks[1]), p(d_ctx), p(d_sig_all), p(d_msg_all), 32, n, stream()), "zip215")  # noqa: E731
            tp, tz = rounds([fp, fz])
            fz()
            wide = L.c25519_amd_verify_check_last_wide()
            assert all(bool(o.all()) for o in oks), n
            say(f"{'2^' + str(lg):>6} {cell(n, tp):>34} {cell(n, tz):>34} {tz[0] / tp[0]:12.2f} {wide:>5}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

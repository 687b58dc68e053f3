#!/usr/bin/env python3
"""tools/verify_batch_rate.py -- ZIP-215 batch verification (ed25519_VerifyBatch_zip215_dev): the batch equation at each window width
against the per-element path of the same build, on the same honest inputs.  Its numbers set the defaults of BATCH_EQ_MIN and of the
built-in window width (csrc/engine_batch_eq.hip).

    python tools/verify_batch_rate.py [--out profiles/verify_batch_rate.txt] [--reps 5] [--parent-lib PATH]
    rocprofv3 --kernel-trace --stats -d DIR -o eq -- python tools/verify_batch_rate.py --kernels 20 [--width 13]
    python tools/rocpd_summary.py stats DIR/.../eq_results.db          # the split of the equation's kernels, appended to the file

Honest inputs (device-made keys and signatures, 32-byte messages), n = 2^10 .. 2^20 through the *_dev form in ONE process, device
events.  Per size, after a warm-up of every variant, --reps rounds; in a round the variants alternate -- (a) BATCH_EQ_MIN = 0: the
per-element ZIP-215 kernels into scratch plus the AND-reduction, (b) BATCH_EQ_MIN = 1 at BATCH_EQ_WINDOW = 8, 10, 13 -- each the median
of --reps calls.  The table gives the median round and [min .. max] over the rounds.  --parent-lib: a libcurve25519_amd.so built from
the PARENT commit; ed25519_VerifySignature_zip215_dev at 2^20 is then measured in fresh child processes, this build and the parent's
alternating, to show that the existing call did not move (the margin is that call's own round-to-round spread).  --kernels K: only run
the equation at 2^K a few times (what the rocprofv3 run traces).  Needs the GPU; there is no CPU fallback."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
WIDTHS = (8, 10, 13)
SEED = bytes(range(32))


def use_library(path):
    """load `path` instead of the tree's library; entry points it lacks (an older build) are dropped from the ctypes table"""
    import ctypes
    from curve25519_amd import _lib, build
    build.LIB = path
    build.is_stale = lambda: False                           # never rebuild over somebody else's library
    have = ctypes.CDLL(path)
    for name in list(_lib.SIGNATURES):
        if not hasattr(have, name):
            del _lib.SIGNATURES[name]


def inputs(api, n, rng):
    pub, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return api.ed25519_SignMessage(priv, msg), pub, msg


def dev_ms(torch, reps, fn):
    t = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        t.append(s.elapsed_time(e))
    return float(np.median(t))


def child_zip215(a):
    """ed25519_VerifySignature_zip215_dev at 2^20 with the library --lib names: one JSON line of round medians"""
    import torch
    if a.lib:
        use_library(a.lib)
    from curve25519_amd import api
    n = 1 << 20
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in inputs(api, n, np.random.default_rng(0xBA7C4ED))]
    out = torch.empty((n, 1), dtype=torch.int32, device="cuda")
    for _ in range(3):
        api.ed25519_VerifySignature_zip215_dev(out, *t)
    rounds = [dev_ms(torch, a.reps, lambda: api.ed25519_VerifySignature_zip215_dev(out, *t)) for _ in range(a.reps)]
    assert int(out.sum()) == n
    print(json.dumps({"rounds_ms": rounds}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch_rate.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--width", type=int, default=-1)
    ap.add_argument("--child-zip215", action="store_true")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("verify_batch_rate: no GPU")
    if a.child_zip215:
        return child_zip215(a)
    from curve25519_amd import _lib, api
    lib = _lib.load()
    rng = np.random.default_rng(0xBA7C4ED)
    N = 1 << (a.kernels or 20)
    sig, pub, msg = inputs(api, N, rng)
    res = torch.full((1, 1), -7, dtype=torch.int32, device="cuda")

    def tensors(n):
        return [torch.from_numpy(np.ascontiguousarray(x[:n])).cuda() for x in (sig, pub, msg)]

    if a.kernels:
        t = tensors(N)
        with _lib.tunable("BATCH_EQ_MIN", 1), _lib.tunable("BATCH_EQ_WINDOW", a.width):
            for _ in range(10):
                api.ed25519_VerifyBatch_zip215_dev(res, *t, SEED)
            torch.cuda.synchronize()
        assert int(res.cpu()[0, 0]) == 1
        return

    variants = [("per element", 0, -1)] + [(f"c = {c}", 1, c) for c in WIDTHS]
    lines = [f"# tools/verify_batch_rate.py on {torch.cuda.get_device_name(0)}; honest inputs; {a.reps} rounds, the variants alternating, "
             f"each the median of {a.reps} calls; ms, [min .. max] over the rounds",
             f"{'n':>6} " + " ".join(f"{name:>12} {'[min .. max]':>19}" for name, _, _ in variants) + f" {'best eq':>8} {'per element / best':>19}"]
    table = {}
    for k in range(10, 21):
        n = 1 << k
        t = tensors(n)

        def call(mn, c):
            with _lib.tunable("BATCH_EQ_MIN", mn), _lib.tunable("BATCH_EQ_WINDOW", c):
                api.ed25519_VerifyBatch_zip215_dev(res, *t, SEED)

        for _, mn, c in variants * 2:                                            # clock ramp-up, on every variant
            call(mn, c)
        rounds = {name: [] for name, _, _ in variants}
        for _ in range(a.reps):
            for name, mn, c in variants:
                rounds[name].append(dev_ms(torch, a.reps, lambda: call(mn, c)))
                assert int(res.cpu()[0, 0]) == 1
        med = {name: float(np.median(v)) for name, v in rounds.items()}
        best = min((name for name, _, _ in variants[1:]), key=med.get)
        table[k] = (med, rounds, best)
        lines.append(f"{'2^%d' % k:>6} " + " ".join(f"{med[name]:12.3f} [{min(rounds[name]):7.3f} .. {max(rounds[name]):7.3f}]" for name, _, _ in variants)
                     + f" {best:>8} {med['per element'] / med[best]:19.3f}")
    # the defaults the numbers give: the smallest size FROM WHICH the best equation beats the per-element path by more than the
    # rounds' spread (of either), at every larger measured size too
    wins = {}
    for k, (med, rounds, best) in table.items():
        spread = max(max(rounds[x]) - min(rounds[x]) for x in ("per element", best))
        wins[k] = med["per element"] - med[best] > spread
    from_k = None
    for k in sorted(table, reverse=True):
        if not wins[k]:
            break
        from_k = k
    lines.append("")
    lines.append("BATCH_EQ_MIN from these numbers: " + (f"2^{from_k} = {1 << from_k}" if from_k else "never (0): the equation wins at no measured size"))
    lines.append("fastest width per size: " + ", ".join(f"2^{k}: {table[k][2]}" for k in sorted(table)))
    lines.append(f"scratch at 2^20: ed25519_VerifyBatch_scratch_bytes = {lib.ed25519_VerifyBatch_scratch_bytes(1 << 20)} "
                 f"({lib.ed25519_VerifyBatch_scratch_bytes(1 << 20) / (1 << 20):.0f} B per element, built-in width), "
                 f"ed25519_VerifySignature_scratch_bytes = {lib.ed25519_VerifySignature_scratch_bytes(1 << 20)} "
                 f"({lib.ed25519_VerifySignature_scratch_bytes(1 << 20) / (1 << 20):.0f} B per element)")
    if a.parent_lib:
        runs = {"this build": [], "parent": []}
        for _ in range(2):
            for name, path in (("this build", None), ("parent", a.parent_lib)):
                cmd = [sys.executable, os.path.abspath(__file__), "--child-zip215", "--reps", str(a.reps)] + (["--lib", path] if path else [])
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, check=True).stdout
                runs[name] += json.loads(out.strip().splitlines()[-1])["rounds_ms"]
        lines.append("")
        lines.append("ed25519_VerifySignature_zip215_dev at 2^20, fresh processes, this build and the parent commit's alternating (2 x "
                     f"{a.reps} rounds each, each the median of {a.reps} calls):")
        for name, v in runs.items():
            lines.append(f"  {name:>10}: median {np.median(v):7.3f} ms  [{min(v):7.3f} .. {max(v):7.3f}]  spread {max(v) - min(v):.3f} ms")
        d = float(np.median(runs["this build"]) - np.median(runs["parent"]))
        margin = max(max(v) - min(v) for v in runs.values())
        lines.append(f"  this build - parent: {d:+.3f} ms; margin (the call's own round-to-round spread): {margin:.3f} ms -> "
                     + ("did not move" if d <= margin else "SLOWER THAN THE PARENT"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

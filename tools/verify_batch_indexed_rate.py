#!/usr/bin/env python3
"""tools/verify_batch_indexed_rate.py -- ZIP-215 batch verification with coalesced keys (ed25519_VerifyBatch_zip215_indexed_dev) against
the un-indexed equation and the per-element call on the gathered keys, on the same honest inputs.  Its numbers set the default of
BATCH_EQ_INDEXED_MIN and say whether the built-in window width should differ from the un-indexed call's (csrc/engine_batch_eq.hip).

    python tools/verify_batch_indexed_rate.py [--out profiles/verify_batch_indexed_rate.txt] [--reps 5] [--parent-lib PATH]
    rocprofv3 --kernel-trace --stats -d DIR -o keyeq -- python tools/verify_batch_indexed_rate.py --kernels 20 --keys 256
    python tools/rocpd_summary.py stats DIR/.../keyeq_results.db       # the split of the equation's kernels, appended to the file

Honest inputs (device-made keys and signatures, 32-byte messages; element i under a uniformly drawn key, and under key perm(i) at
K = n), n = 2^14 .. 2^20 and K in {1, 256, 4096, 65536, n} (K <= n) through the *_dev forms in ONE process, device events.  Per cell,
after a warm-up of every variant, --reps rounds; in a round the variants alternate -- (a) the indexed equation (BATCH_EQ_INDEXED_MIN
= 1) at c = 10 and at c = 13, (b) ed25519_VerifyBatch_zip215_dev on the gathered keys with BATCH_EQ_MIN = 1, (c)
ed25519_VerifySignature_zip215_dev on the gathered keys -- each the median of --reps calls.  The table gives the median round and
[min .. max] over the rounds; (a) in the ratios is the width the built-in choice takes at that n.  --parent-lib: a
libcurve25519_amd.so built from the PARENT commit; ed25519_VerifyBatch_zip215_dev and ed25519_VerifySignature_zip215_dev at 2^20 are
then measured in fresh child processes, this build and the parent's alternating, to show that the existing calls did not move (the
margin is each call's own round-to-round spread).  --kernels K: only run the indexed equation at 2^K over --keys keys a few times (what
the rocprofv3 run traces).  Needs the GPU; there is no CPU fallback."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from verify_batch_rate import dev_ms, use_library  # noqa: E402

SEED = bytes(range(32))
KEYS = (1, 256, 4096, 65536, None)                          # None: K = n
VARIANTS = ("(a) c=10", "(a) c=13", "(b) equation", "(c) per element")


def builtin_width(n):
    return 10 if n < (1 << 16) else 13


def child(a):
    """the two existing calls at 2^20 with the library --lib names: one JSON line of round medians each"""
    import torch
    if a.lib:
        use_library(a.lib)
    from curve25519_amd import api
    n = 1 << 20
    rng = np.random.default_rng(0xC0A1E5CE)
    pub, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (api.ed25519_SignMessage(priv, msg), pub, msg)]
    out = torch.empty((n, 1), dtype=torch.int32, device="cuda")
    res = torch.full((1, 1), -7, dtype=torch.int32, device="cuda")
    calls = {"VerifyBatch_zip215_dev": lambda: api.ed25519_VerifyBatch_zip215_dev(res, *t, SEED),
             "VerifySignature_zip215_dev": lambda: api.ed25519_VerifySignature_zip215_dev(out, *t)}
    for fn in list(calls.values()) * 3:
        fn()
    rounds = {name: [] for name in calls}
    for _ in range(a.reps):
        for name, fn in calls.items():
            rounds[name].append(dev_ms(torch, a.reps, fn))
    assert int(out.sum()) == n and int(res.cpu()[0, 0]) == 1
    print(json.dumps(rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch_indexed_rate.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--keys", type=int, default=256)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("verify_batch_indexed_rate: no GPU")
    if a.child:
        return child(a)
    from curve25519_amd import _lib, api
    lib = _lib.load()
    rng = np.random.default_rng(0xC0A1E5CD)
    N = 1 << (a.kernels or 20)
    pub, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (N, 32), dtype=np.uint8))
    msg = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    res = torch.full((1, 1), -7, dtype=torch.int32, device="cuda")
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731

    def tensors(n, K):
        """keys[K], idx[n, 1], sig[n], msg[n], gathered pk[n] on the device"""
        idx = rng.permutation(n) if K == n else rng.integers(0, K, n)
        sig = api.ed25519_SignMessage(priv[idx], msg[:n])
        return cuda(pub[:K]), cuda(idx.astype(np.uint32).view(np.int32).reshape(-1, 1)), cuda(sig), cuda(msg[:n]), cuda(pub[idx])

    if a.kernels:
        keys, idx, sig, m, _ = tensors(N, min(a.keys, N))
        with _lib.tunable("BATCH_EQ_INDEXED_MIN", 1):
            for _ in range(10):
                api.ed25519_VerifyBatch_zip215_indexed_dev(res, keys, idx, sig, m, SEED)
            torch.cuda.synchronize()
        assert int(res.cpu()[0, 0]) == 1
        return

    lines = [f"# tools/verify_batch_indexed_rate.py on {torch.cuda.get_device_name(0)}; honest inputs; {a.reps} rounds, the variants "
             f"alternating, each the median of {a.reps} calls; ms, [min .. max] over the rounds; (a) in the ratios: the built-in width's",
             f"{'n':>5} {'K':>6} " + " ".join(f"{name:>16} {'[min .. max]':>19}" for name in VARIANTS) + f" {'(b)/(a)':>8} {'(c)/(a)':>8}"]
    table = {}
    for k in range(14, 21):
        n = 1 << k
        for K in sorted({n if K is None else K for K in KEYS if (K or n) <= n}):
            keys, idx, sig, m, pk = tensors(n, K)
            verdict = torch.empty((n, 1), dtype=torch.int32, device="cuda")

            def indexed(c):
                with _lib.tunable("BATCH_EQ_INDEXED_MIN", 1), _lib.tunable("BATCH_EQ_WINDOW", c):
                    api.ed25519_VerifyBatch_zip215_indexed_dev(res, keys, idx, sig, m, SEED)

            def equation():
                with _lib.tunable("BATCH_EQ_MIN", 1):
                    api.ed25519_VerifyBatch_zip215_dev(res, sig, pk, m, SEED)

            def per_element():
                api.ed25519_VerifySignature_zip215_dev(verdict, sig, pk, m)
                res.fill_(1)

            calls = dict(zip(VARIANTS, (lambda: indexed(10), lambda: indexed(13), equation, per_element)))
            for fn in list(calls.values()) * 2:                                   # clock ramp-up, on every variant
                fn()
            rounds = {name: [] for name in VARIANTS}
            for _ in range(a.reps):
                for name, fn in calls.items():
                    rounds[name].append(dev_ms(torch, a.reps, fn))
                    assert int(res.cpu()[0, 0]) == 1
            assert int(verdict.sum()) == n
            med = {name: float(np.median(v)) for name, v in rounds.items()}
            mine = f"(a) c={builtin_width(n)}"
            table[k, K] = (med, rounds, mine)
            lines.append(f"{'2^%d' % k:>5} {K:>6} " + " ".join(f"{med[name]:16.3f} [{min(rounds[name]):7.3f} .. {max(rounds[name]):7.3f}]" for name in VARIANTS)
                         + f" {med[VARIANTS[2]] / med[mine]:8.3f} {med[VARIANTS[3]] / med[mine]:8.3f}")
    # the defaults the numbers give: the smallest size FROM WHICH (a) beats (c) by more than the rounds' spread (of either) at every
    # measured K <= 65536, at every larger measured size too
    def wins(k, K, over):
        med, rounds, mine = table[k, K]
        return med[over] - med[mine] > max(max(rounds[x]) - min(rounds[x]) for x in (over, mine))

    from_k = None
    for k in range(20, 13, -1):
        if not all(wins(k, K, VARIANTS[3]) for (kk, K) in table if kk == k and K <= 65536):
            break
        from_k = k
    lines.append("")
    lines.append("BATCH_EQ_INDEXED_MIN from these numbers: " + (f"2^{from_k} = {1 << from_k}" if from_k else "never (0): (a) wins at no measured size"))
    lines.append("faster width of (a) per cell (* = by more than the rounds' spread): " + ", ".join(
        f"2^{k}/{K}: c={10 if med['(a) c=10'] < med['(a) c=13'] else 13}"
        + ("*" if abs(med["(a) c=10"] - med["(a) c=13"]) > max(max(rounds[x]) - min(rounds[x]) for x in VARIANTS[:2]) else "")
        for (k, K), (med, rounds, _) in sorted(table.items())))
    lines.append("(a) beats (b) by more than the rounds' spread at 2^20: " + ", ".join(
        f"K = {K}: {'yes' if wins(20, K, VARIANTS[2]) else 'NO'}" for (k, K) in sorted(table) if k == 20))
    lines.append("what K = n costs over (b), the price of the accumulation ((a) - (b), ms): " + ", ".join(
        f"2^{k}: {table[k, 1 << k][0][table[k, 1 << k][2]] - table[k, 1 << k][0][VARIANTS[2]]:+.3f}" for k in range(14, 21)))
    lines.append(f"scratch at 2^20: ed25519_VerifyBatch_indexed_scratch_bytes(2^20, 256) = {lib.ed25519_VerifyBatch_indexed_scratch_bytes(1 << 20, 256)}, "
                 f"(2^20, 2^20) = {lib.ed25519_VerifyBatch_indexed_scratch_bytes(1 << 20, 1 << 20)}, "
                 f"ed25519_VerifyBatch_scratch_bytes(2^20) = {lib.ed25519_VerifyBatch_scratch_bytes(1 << 20)}")
    if a.parent_lib:
        runs = {}
        for _ in range(2):
            for who, path in (("this build", None), ("parent", a.parent_lib)):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)] + (["--lib", path] if path else [])
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, check=True).stdout
                for name, v in json.loads(out.strip().splitlines()[-1]).items():
                    runs.setdefault(name, {}).setdefault(who, []).extend(v)
        lines.append("")
        lines.append("the existing calls at 2^20, default tunables, fresh processes, this build and the parent commit's alternating (2 x "
                     f"{a.reps} rounds each, each the median of {a.reps} calls):")
        for name, by in runs.items():
            for who, v in by.items():
                lines.append(f"  ed25519_{name:<27} {who:>10}: median {np.median(v):7.3f} ms  [{min(v):7.3f} .. {max(v):7.3f}]  spread {max(v) - min(v):.3f} ms")
            d = float(np.median(by["this build"]) - np.median(by["parent"]))
            margin = max(max(v) - min(v) for v in by.values())
            lines.append(f"  this build - parent: {d:+.3f} ms; margin (the call's own round-to-round spread): {margin:.3f} ms -> "
                         + ("did not move" if d <= margin else "SLOWER THAN THE PARENT"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

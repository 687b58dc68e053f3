"""The instruction counts of the secret-bearing kernels do not depend on the secret.  tests/test_secret_taint.py
sees the device SOURCE; a branch the gfx950 compiler puts around a secret-dependent select shows only in the code that runs, as
counts that move with the secret.  So one child process (tests/secret_counts_child.py) runs under `rocprofv3 --pmc`, a counter run
of its own with no tracing, and issues every secret-bearing *_dev call once per secret class with identical public inputs; the
tests read the per-dispatch counters and hold, per call kind and size, that the kernel names and every compared counter are equal,
dispatch for dispatch, in all six classes.

With random per-lane secrets a divergent branch runs both sides in every wave and the counts stay put, so four of the classes are
uniform across the call (all 0x00, all 0xff, two random values repeated in every row): a secret-dependent branch is then
wave-uniform and skips instructions.  The fifth has independent random rows, the sixth repeats the third: the control.

Counters compared: SQ_WAVES, SQ_INSTS_VALU, SQ_INSTS_SALU, SQ_INSTS_SMEM, SQ_INSTS_LDS, SQ_INSTS_VMEM.

tests/ct_probe.hip proves that the method sees a leak: a kernel that multiplies under `if (secret & 1)` must differ in
SQ_INSTS_VALU between all-zero and all-ones input, one that selects by mask must not."""
import collections
import json
import os
import sqlite3
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import secret_counts_child as child  # noqa: E402

COUNTERS = ("SQ_WAVES", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_SMEM", "SQ_INSTS_LDS", "SQ_INSTS_VMEM")
COMPARED = COUNTERS                      # (a counter that classes uniform_a and uniform_a_again disagree in would leave this list)
MARKER = "k_ct_marker"
NOT_OURS = ("void at::", "__amd")        # torch's fills and the runtime's copy kernels
LIMIT = 300                              # seconds for the profiled child, start-up of the profiler included

Dispatch = collections.namedtuple("Dispatch", "kernel counters")


@pytest.fixture(scope="module")
def segments(tmp_path_factory):
    """{(kind, n, class): [Dispatch, ...]} of one profiled run of the child"""
    out = tmp_path_factory.mktemp("secret_counts")
    cmd = ["timeout", "-k", "10", str(LIMIT), "rocprofv3", "--pmc", *COUNTERS, "-d", str(out), "-o", "counts", "--",
           sys.executable, os.path.join(HERE, "secret_counts_child.py"), str(out)]
    t0 = time.time()
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=os.path.dirname(HERE))
    print(f"rocprofv3 + child: {time.time() - t0:.1f} s")
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout.decode(errors='replace')[-3000:]}"
    with open(out / "manifest.json") as f:
        manifest = json.load(f)
    dbs = [os.path.join(d, f) for d, _, files in os.walk(out) for f in files if f.endswith(".db")]
    assert len(dbs) == 1, f"expected one rocpd database, found {dbs}\n{p.stdout.decode(errors='replace')[-2000:]}"
    db = sqlite3.connect(dbs[0])
    per_dispatch = collections.OrderedDict()
    for dispatch_id, name, counter, value in db.execute(
            "select dispatch_id, kernel_name, counter_name, value from counters_collection order by dispatch_id"):
        d = per_dispatch.setdefault(dispatch_id, Dispatch(name, {}))
        d.counters[counter] = d.counters.get(counter, 0) + value
    parts, cur = [], None
    for d in per_dispatch.values():
        if d.kernel.startswith(MARKER):
            cur = []
            parts.append(cur)
        elif cur is not None and not d.kernel.startswith(NOT_OURS):
            cur.append(d)
    assert len(parts) == len(manifest), (len(parts), len(manifest))
    got = collections.OrderedDict()
    for what, dispatches in zip(manifest, parts):
        key = (what["kind"], what["n"], what["cls"])
        assert key not in got
        for d in dispatches:
            assert set(d.counters) >= set(COUNTERS), (key, d.kernel, sorted(d.counters))
        got[key] = dispatches
    return got


def describe(d):
    return f"{d.kernel.split('(')[0]} " + " ".join(f"{c[3:]}={int(d.counters[c])}" for c in COUNTERS)


def test_probe_kernels_show_that_a_leak_is_seen(segments):
    def valu(kind, cls):
        (d,) = segments[(kind, child.PROBE_N, cls)]
        print(kind, cls, describe(d))
        return d.counters["SQ_INSTS_VALU"]
    assert valu("probe_branch", "zeros") != valu("probe_branch", "ones"), "a branch on the secret did not move SQ_INSTS_VALU"
    assert valu("probe_select", "zeros") == valu("probe_select", "ones"), "a select by mask moved SQ_INSTS_VALU"


CALLS = [(kind, n) for kind, sizes in child.SIZES.items() for n in sizes]


@pytest.mark.parametrize("kind,n", CALLS, ids=[f"{k}-{n}" for k, n in CALLS])
def test_control_reproduces(segments, kind, n):
    """the same secrets twice: every compared counter must reproduce, or it says nothing about the other classes"""
    a, b = segments[(kind, n, "uniform_a")], segments[(kind, n, "uniform_a_again")]
    assert a, "the call dispatched no kernel"
    assert [d.kernel for d in a] == [d.kernel for d in b]
    for x, y in zip(a, b):
        for c in COMPARED:
            assert x.counters[c] == y.counters[c], f"{c} does not reproduce: {describe(x)} | {describe(y)}"


@pytest.mark.parametrize("kind,n", CALLS, ids=[f"{k}-{n}" for k, n in CALLS])
def test_counts_do_not_move_with_the_secret(segments, kind, n):
    ref = segments[(kind, n, child.CLASSES[0])]
    assert ref, "the call dispatched no kernel"
    for d in ref:
        print(child.CLASSES[0], describe(d))
    for cls in child.CLASSES[1:]:
        got = segments[(kind, n, cls)]
        assert [d.kernel for d in got] == [d.kernel for d in ref], f"class {cls} dispatched other kernels"
        for x, y in zip(ref, got):
            for c in COMPARED:
                assert x.counters[c] == y.counters[c], f"{c} moves with the secret ({child.CLASSES[0]} | {cls}): {describe(x)} | {describe(y)}"

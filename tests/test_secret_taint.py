"""No secret reaches a branch, and only the documented row fetches take an address from one, checked on the
device source compiled for the CPU: tests/host_emul/taint_*.cpp are stand-alone programs over the emulation units, built with
MemorySanitizer (tests/host_emul/build.py: build_taint).  A case marks the secret inputs of one operation uninitialised and calls
the unit's entry point; MemorySanitizer reports every branch condition and every load or store address that derives from them.
Each report is mapped to (kind, innermost function outside the C model) and held against tests/ct_allowed.py.

Every unit is built twice: the second build checks branch conditions only, so a report it gives is a `branch`; one that only the
full build gives, at a line where the second is silent, is an `address`.  A CPU test: the programs run as subprocesses, nothing is
loaded into python, and it stays off machines with a GPU."""
import collections
import concurrent.futures
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "host_emul"))
import build as emul_build  # noqa: E402
import ct_allowed  # noqa: E402
import dispatch_cases  # noqa: E402
import invert_cases  # noqa: E402

MODEL_FILES = ("valu_model.h", "coop_wave.h")            # the C model of the instructions: a report is charged to its caller
# 0, and one length on each side of a SHA-512 block edge of both hashes: H(enc(R) || pk || m) turns at 47 | 48, H(prefix || m) at 79 | 80
MSG_LENGTHS = (0,) + tuple(n for n in dispatch_cases.MSG_LENGTHS if n in (47, 48, 79, 80))
INVERT_K = 4                                             # one group size of the shared inversion: seven lanes, the last slot ragged
INVERT_N = invert_cases.ragged_n(7, INVERT_K, 2)
JOBS = min(16, os.cpu_count() or 1)                      # programs running side by side
SELFCHECK_UNIT = "key_convert"                           # the smallest program; the self-check is the same code in all of them

FRAME = re.compile(r"^\s+#(\d+) 0x[0-9a-f]+\s+\((.+)\+0x([0-9a-f]+)\)")
Report = collections.namedtuple("Report", "kind function where")


def _skip_reason():
    if os.path.exists("/dev/kfd"):
        return "a GPU machine: sanitizer runs stay off it"
    cxx, why = emul_build.taint_toolchain()
    return None if cxx else why


pytestmark = pytest.mark.skipif(_skip_reason() is not None, reason=_skip_reason() or "")


def run_program(prog, *args):
    """stderr of one run: {case: [pc of the innermost frame of each report, ...]} in order, and the text after @@END"""
    env = dict(os.environ, MSAN_OPTIONS="halt_on_error=0:symbolize=0:exitcode=0:fast_unwind_on_fatal=1")
    p = subprocess.run([prog, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    text = p.stderr.decode(errors="replace")
    assert p.returncode == 0, f"{prog} {args}: exit {p.returncode}\n{text[-2000:]}"
    cases, case, end = collections.OrderedDict(), None, None
    for line in text.splitlines():
        if line.startswith("@@CASE "):
            case = line[7:]
            assert case not in cases, f"case named twice: {case}"
            cases[case] = []
        elif line.startswith("@@END"):
            end = line[5:].strip()
        else:
            m = FRAME.match(line)
            if m and m.group(1) == "0":
                assert case is not None, f"a report in front of the first case:\n{text[:2000]}"
                assert os.path.basename(m.group(2)) == os.path.basename(prog), f"a report outside the program: {line}"
                cases[case].append(int(m.group(3), 16))
    assert end is not None, f"{prog} did not finish:\n{text[-2000:]}"
    return cases, end


def symbolise(prog, pcs):
    """{pc: (function, 'file:line') of the innermost frame, inlined ones included, outside the model's files}"""
    _, symbolizer = emul_build.taint_toolchain()
    pcs = sorted(set(pcs))
    if not pcs:
        return {}
    # frame 0 holds the address behind the call that reports: one byte back lies inside the reporting instruction's line
    query = "".join(f"{hex(pc - 1)}\n" for pc in pcs)
    out = subprocess.run([symbolizer, "--obj=" + prog, "--inlines", "--functions=short", "--demangle", "--output-style=LLVM"],
                         input=query.encode(), stdout=subprocess.PIPE, check=True).stdout.decode()
    blocks = [b for b in out.split("\n\n") if b.strip()]
    assert len(blocks) == len(pcs), (len(blocks), len(pcs))
    found = {}
    for pc, block in zip(pcs, blocks):
        lines = block.strip().splitlines()
        frames = [(lines[i], lines[i + 1]) for i in range(0, len(lines) - 1, 2)]
        for function, where in frames:
            path, line = where.rsplit(":", 2)[:2]
            if os.path.basename(path) not in MODEL_FILES:
                found[pc] = (function.split("<")[0], f"{os.path.basename(path)}:{line}")       # (an instance of a template: its name)
                break
        else:
            found[pc] = (frames[0][0], frames[0][1]) if frames else ("?", "?")
    return found


def unit_reports(unit, *runs):
    """({case: set of Report}, [text after @@END]) of one unit: each of `runs` is the arguments of one run, a share of the unit's
    cases; every run goes through both builds, all of them side by side"""
    progs = emul_build.build_taint((unit,))
    jobs = [(progs[(unit, kind)], *args) for args in runs for kind in ("full", "branch")]
    with concurrent.futures.ThreadPoolExecutor(min(JOBS, len(jobs))) as pool:
        done = list(pool.map(lambda job: run_program(*job), jobs))
    full, branch, end_full = collections.OrderedDict(), collections.OrderedDict(), []
    for i in range(0, len(done), 2):
        assert not set(full) & set(done[i][0]), "two runs ran the same case"
        full.update(done[i][0])
        branch.update(done[i + 1][0])
        end_full.append(done[i][1])
    assert list(full) == list(branch), "the two builds ran different cases"
    sym_full = symbolise(progs[(unit, "full")], [pc for v in full.values() for pc in v])
    sym_branch = symbolise(progs[(unit, "branch")], [pc for v in branch.values() for pc in v])
    out = collections.OrderedDict()
    for case in full:
        branches = {sym_branch[pc] for pc in branch[case]}
        reports = {Report("branch", f, w) for f, w in branches}
        reports |= {Report("address", *sym_full[pc]) for pc in full[case] if sym_full[pc] not in branches}
        out[case] = reports
    return out, end_full


@pytest.fixture(scope="module")
def programs():
    return emul_build.build_taint()


@pytest.fixture(scope="module")
def invert_files(tmp_path_factory):
    """limbs for the shared inversion, with zero slots on its slot map and without (tests/invert_cases.py)"""
    d = tmp_path_factory.mktemp("taint_invert")
    slots = invert_cases.batch_slots(INVERT_N, INVERT_K)
    zeros = invert_cases.all_zeros(invert_cases.zero_patterns(slots, seed=1))
    assert zeros
    paths = []
    for name, z in (("zero", zeros), ("plain", set())):
        limbs, _ = invert_cases.make_inputs(INVERT_N, z, seed=len(z) + 1)
        paths.append(str(d / f"{name}.bin"))
        np.ascontiguousarray(limbs, np.uint32).tofile(paths[-1])
    return paths


@pytest.fixture(scope="module")
def all_reports(programs, invert_files):
    """{unit: {case: set of Report}}, every case run once; the units with signing cases in one run per message length"""
    def one(unit):
        runs = [["cases", "base"] + ([*invert_files, str(INVERT_N), str(INVERT_K)] if unit == "emul" else [])]
        if unit in ("emul", "sign_ctx"):
            runs += [["cases", str(n)] for n in MSG_LENGTHS]
        reports, ends = unit_reports(unit, *runs)
        assert ends == ["overflows=0"] * len(runs), f"{unit}: {emul_build.MAD_OVERFLOW} ({ends})"
        return reports

    with concurrent.futures.ThreadPoolExecutor(2) as pool:            # (the two large units overlap; each runs JOBS programs at a time)
        return dict(zip(emul_build.TAINT_UNITS, pool.map(one, emul_build.TAINT_UNITS)))


def test_selfcheck_of_the_method(programs):
    """the four lane functions of taint_harness.h come out as written there -- else no silence of the other tests means anything"""
    got, _ = unit_reports(SELFCHECK_UNIT, ["selfcheck"])
    kinds = {case: sorted((r.kind, r.function) for r in reports) for case, reports in got.items()}
    assert kinds["selfcheck_branch"] == [("branch", "selfcheck_branch")]
    assert kinds["selfcheck_index"] == [("address", "selfcheck_index")]
    assert not ct_allowed.allows("address", "selfcheck_index")
    assert ("branch", "selfcheck_row_branch") in kinds["selfcheck_row_branch"], "taint did not survive the row fetch"
    assert kinds["selfcheck_select"] == []


def test_selfcheck_needs_the_poisoned_table(programs):
    """... and the third one is silent on a clean table: the row's taint is the table's, which is why the cases poison theirs"""
    got, _ = unit_reports(SELFCHECK_UNIT, ["selfcheck", "clean-table"])
    assert {(r.kind, r.function) for r in got["selfcheck_row_branch"]} == {("address", "selfcheck_row_branch")}


def test_cases_cover_every_operation(all_reports):
    cases = [c for unit in all_reports.values() for c in unit]
    for prefix in ("x25519/", "x25519_public_ladder/", "x25519_public/", "one_peer/comb", "one_peer/ladder", "peer_indexed/", "keypair/",
                   "sign/", "blinding_init/", "sign_ctx_init/", "sign_indexed/", "private_to_x25519/", "invert/zero_slot", "invert/no_zero"):
        assert any(c.startswith(prefix) for c in cases), prefix
    for n in MSG_LENGTHS:
        for op in ("sign/", "sign_indexed/"):
            forms = {c.split("/")[1] for c in cases if c.startswith(op) and c.endswith(f"/len{n}")}
            assert forms == {"lane", "quad", "wave"}, (op, n, forms)


def test_no_secret_branch_and_only_listed_addresses(all_reports):
    bad = collections.OrderedDict()
    for unit, cases in all_reports.items():
        for case, reports in cases.items():
            for r in sorted(reports):
                if not ct_allowed.allows(r.kind, r.function):
                    bad.setdefault((r.kind, r.function, r.where), []).append(f"{unit}:{case}")
    lines = [f"{kind} in {function} ({where}): {len(cs)} cases, first {cs[0]}" for (kind, function, where), cs in bad.items()]
    assert not bad, "secret-dependent:\n" + "\n".join(lines)


def test_every_allowed_entry_is_hit(all_reports):
    hit = {(r.kind, r.function) for cases in all_reports.values() for reports in cases.values() for r in reports}
    stale = [e for e in ct_allowed.ALLOWED if (e.kind, e.function) not in hit]
    assert not stale, f"entries of tests/ct_allowed.py that no case reaches: {stale}"
    with open(os.path.join(os.path.dirname(HERE), "DESIGN.md")) as f:
        design = " ".join(f.read().split())
    for e in ct_allowed.ALLOWED:
        assert e.kind in ("address", "branch") and e.reason.strip(), e
        assert " ".join(e.licence.split()) in design, f"{e.function}: DESIGN.md has no such sentence: {e.licence}"

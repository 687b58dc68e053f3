"""The scalar calls under the secret-taint check of tests/test_secret_taint.py (its run, symbolise and skip helpers, by import): with
every scalar input byte marked uninitialised, ed25519_ScalarInvert at every group size (n = 1 and n = K + 1: a whole group and a
ragged one), ed25519_ScalarMul, _ScalarMulAdd, _ScalarAdd, _ScalarSub, _ScalarNegate, _ScalarComplement and _ScalarReduce give NO
report at all: the reductions, the zero test of the inversion, its swap and its forced-zero output are masks, and the only decisions
are on the element index.  The program (tests/host_emul/taint_scalar.cpp) is stand-alone and runs as a subprocess; nothing is loaded
into python, and like the test it borrows from it stays off machines with a GPU."""
import pytest

import test_secret_taint as base
from scalar_model import KS

pytestmark = pytest.mark.skipif(base._skip_reason() is not None, reason=base._skip_reason() or "")

CALLS = ("mul", "muladd", "add", "sub", "negate", "complement", "reduce")


@pytest.fixture(scope="module")
def reports():
    got, ends = base.unit_reports("scalar", ["cases", "base"])
    assert ends == ["overflows=0"], f"{base.emul_build.MAD_OVERFLOW} ({ends})"
    return got


def test_cases_cover_every_call(reports):
    want = {f"invert/k{k}/n{n}" for k in KS for n in (1, k + 1)}
    want |= {f"{call}/n{n}" for call in CALLS for n in (1, 6)}
    assert set(reports) == want


def test_invert_has_no_report_at_all(reports):
    bad = {case: sorted(r) for case, r in reports.items() if case.startswith("invert/") and r}
    assert not bad, bad


def test_elementwise_calls_have_no_report_at_all(reports):
    bad = {case: sorted(r) for case, r in reports.items() if not case.startswith("invert/") and r}
    assert not bad, bad

"""The constant-time multiscalar calls under the secret-taint check of tests/test_secret_taint.py (its run, symbolise and skip helpers,
by import): with every scalar of ed25519_MultiScalarMult and ristretto255_MultiScalarMult marked uninitialised, at m = 1 and 6 terms in
1 and 3 groups, the lane code of all three stages (tests/host_emul/taint_msm.cpp over msm.cpp: rows, the chunked sum, the finish)
gives NO report of either kind -- no branch condition and no load or store address derives from a scalar, not even a row fetch: the
walk selects its rows by masks, which rows a summing lane reads is a function of m alone, and the verdict comes from the points.  The
allow-list is empty: tests/ct_allowed.py is not consulted.  The _vartime calls are for public inputs and are not tainted.  The program
is stand-alone and runs as a subprocess; nothing is loaded into python, and like the test it borrows from it stays off machines with
a GPU."""
import pytest

import test_secret_taint as base

pytestmark = pytest.mark.skipif(base._skip_reason() is not None, reason=base._skip_reason() or "")


@pytest.fixture(scope="module")
def reports():
    got, ends = base.unit_reports("msm", ["cases", "base"])
    assert ends == ["overflows=0"], f"{base.emul_build.MAD_OVERFLOW} ({ends})"
    return got


def test_cases_cover_both_groups_and_every_shape(reports):
    assert set(reports) == {f"msm/{group}/m{m}/g{g}" for group in ("ed25519", "ristretto255") for m in (1, 6) for g in (1, 3)}


def test_no_report_of_either_kind(reports):
    bad = {case: sorted(rs) for case, rs in reports.items() if rs}
    assert not bad, bad

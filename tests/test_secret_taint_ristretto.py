"""The ristretto255 calls under the secret-taint check of tests/test_secret_taint.py (its run, symbolise and skip helpers, by import):
with the 32 scalar bytes marked uninitialised, ristretto255_ScalarMult at every window width -- decode, walk and encode -- gives NO
report; with the 64 hash bytes marked, ristretto255_FromHash gives none either (the square-root step's comparisons, the map's
selections and the encoding's rotation and negations are masks); ristretto255_ScalarMultBase gives only what tests/ct_allowed.py
lists, the wide comb's row fetch.  The program (tests/host_emul/taint_ristretto.cpp) is stand-alone and runs
as a subprocess; nothing is loaded into python, and like the test it borrows from it stays off machines with a GPU."""
import pytest

import ct_allowed
import test_secret_taint as base

pytestmark = pytest.mark.skipif(base._skip_reason() is not None, reason=base._skip_reason() or "")

WINDOWS = (2, 3, 4)


@pytest.fixture(scope="module")
def reports():
    got, ends = base.unit_reports("ristretto", ["cases", "base"])
    assert ends == ["overflows=0"], f"{base.emul_build.MAD_OVERFLOW} ({ends})"
    return got


def test_cases_cover_every_call(reports):
    want = {f"scalarmult/w{w}/n{n}" for w in WINDOWS for n in (1, 6)}
    want |= {f"{call}/n{n}" for call in ("from_hash", "scalarmult_base") for n in (1, 6)}
    assert set(reports) == want


def test_scalarmult_has_no_report_at_all(reports):
    bad = {case: sorted(r) for case, r in reports.items() if case.startswith("scalarmult/") and r}
    assert not bad, bad


def test_from_hash_has_no_report_at_all(reports):
    bad = {case: sorted(r) for case, r in reports.items() if case.startswith("from_hash/") and r}
    assert not bad, bad


def test_scalarmult_base_fetches_rows_and_nothing_else(reports):
    for case, found in reports.items():
        if not case.startswith("scalarmult_base/"):
            continue
        assert found, f"{case}: the wide comb's row fetch was not seen -- is the scalar still marked?"
        bad = [r for r in sorted(found) if not ct_allowed.allows(r.kind, r.function)]
        assert not bad, (case, bad)
        assert {(r.kind, r.function) for r in found} == {("address", "wb_load_pa_signed")}, (case, sorted(found))

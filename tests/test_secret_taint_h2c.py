"""The hashing calls under the secret-taint check of tests/test_secret_taint.py (its run, symbolise and skip helpers, by import): with
the message bytes marked uninitialised, ed25519_HashToCurve, ed25519_EncodeToCurve, ristretto255_HashToGroup, ed25519_HashToScalar and
c25519_ExpandMessageXmd give NO report -- the block loops run on the lengths, the tail words come from the call's arguments, the
map's selections, its sign fix-up and its exceptional case are masks -- at a message length whose last word straddles message and
tail and at a word-aligned one, with one element and with six; with the 32 bytes of u marked, ed25519_MapToCurve gives none either
(u = 0, the exceptional input, among them).  The program (tests/host_emul/taint_h2c.cpp) is stand-alone and runs as a subprocess;
nothing is loaded into python, nothing is listed in tests/ct_allowed.py, and like the test it borrows from it stays off machines with
a GPU."""
import pytest

import test_secret_taint as base

pytestmark = pytest.mark.skipif(base._skip_reason() is not None, reason=base._skip_reason() or "")

STRADDLING, ALIGNED = 37, 64                  # 37 % 8 = 5: the tail starts inside the message's last word; 64: on a word
CALLS = ("hash_to_curve", "encode_to_curve", "hash_to_group", "hash_to_scalar")


@pytest.fixture(scope="module")
def reports():
    got, ends = base.unit_reports("h2c", ["cases", f"base,{STRADDLING}"], ["cases", f"{ALIGNED}"])
    assert ends == ["overflows=0"] * 2, f"{base.emul_build.MAD_OVERFLOW} ({ends})"
    return got


def test_cases_cover_every_call(reports):
    want = {f"{call}/len{n_bytes}/n{n}" for call in CALLS + ("expand",) for n_bytes in (STRADDLING, ALIGNED) for n in (1, 6)}
    want |= {f"map/n{n}" for n in (1, 6)}
    assert set(reports) == want


@pytest.mark.parametrize("call", CALLS + ("expand", "map"))
def test_call_has_no_report_at_all(reports, call):
    bad = {case: sorted(r) for case, r in reports.items() if case.startswith(call + "/") and r}
    assert not bad, bad

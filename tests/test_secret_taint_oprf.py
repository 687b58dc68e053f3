"""The OPRF / VOPRF calls under the secret-taint check of tests/test_secret_taint.py (its run, symbolise and skip helpers, by import):
with the named inputs marked uninitialised -- Blind: input and blind; Finalize: input and blind; OPRF_BlindEvaluate: skS;
VOPRF_BlindEvaluate: skS and proof_rand -- the lane code gives NO branch report anywhere, and the only address reports are the base
comb's row fetch (wb_load_pa_signed, which tests/ct_allowed.py lists for signing), and only in the VOPRF server, for [skS]B and
[r]B: the variable-base walks select their rows by masks, the hashes run on lengths, the inversion mod L is division steps on masks,
and the verdicts that depend on a secret being zero are formed and applied as masks.  At an input length whose bytes straddle a word
behind Finalize's two length bytes and at one that ends on a word, with one row and with six; the server with one request and with
three.  The program (tests/host_emul/taint_oprf.cpp) is stand-alone and runs as a subprocess; nothing is loaded into python,
tests/ct_allowed.py is not edited, and like the test it borrows from it stays off machines with a GPU."""
import pytest

import ct_allowed
import test_secret_taint as base

pytestmark = pytest.mark.skipif(base._skip_reason() is not None, reason=base._skip_reason() or "")

STRADDLING, ALIGNED = 5, 30                      # 2 + 5 ends inside a word, 2 + 30 on one


@pytest.fixture(scope="module")
def reports():
    got, ends = base.unit_reports("oprf", ["cases", f"base,{STRADDLING}"], ["cases", f"{ALIGNED}"])
    assert ends == ["overflows=0"] * 2, f"{base.emul_build.MAD_OVERFLOW} ({ends})"
    return got


def test_cases_cover_every_call_and_size(reports):
    want = {f"{call}/len{n_bytes}/n{n}" for call in ("blind", "finalize") for n_bytes in (STRADDLING, ALIGNED) for n in (1, 6)}
    want |= {f"{call}/n{n}" for call in ("evaluate", "voprf") for n in (1, 6)}
    assert set(reports) == want


def test_no_secret_branch(reports):
    bad = {case: sorted(r for r in rs if r.kind == "branch") for case, rs in reports.items()}
    assert not any(bad.values()), bad


def test_only_the_servers_comb_row_fetch_takes_a_secret_address(reports):
    for case, rs in reports.items():
        bad = sorted(r for r in rs if r.kind == "address" and not ct_allowed.allows("address", r.function))
        assert not bad, (case, bad)
        if case.startswith("voprf/"):
            assert {r.function for r in rs} == {"wb_load_pa_signed"}, (case, sorted(rs))
        else:
            assert not rs, (case, sorted(rs))

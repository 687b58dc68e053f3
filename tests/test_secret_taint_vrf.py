"""ed25519_VRF_Prove under the secret-taint check of tests/test_secret_taint.py (its run, symbolise and skip helpers, by import): with
the 32 seed bytes of every private key marked uninitialised -- and so SHA-512(seed), x, k and what s is computed from -- the lane code
gives NO branch report, and the only address reports are the base comb's row fetch for [k]B (wb_load_pa_signed, which
tests/ct_allowed.py lists for signing): the variable-base walks [x]H and [k]H select their rows by masks, the hashes run on lengths,
the inversions and encodings see public points only.  At an alpha length that straddles a word behind the 32 key bytes and at a
word-aligned one, with one element and with six.  The program (tests/host_emul/taint_vrf.cpp) is stand-alone and runs as a
subprocess; nothing is loaded into python, tests/ct_allowed.py is not edited, and like the test it borrows from it stays off machines
with a GPU."""
import pytest

import ct_allowed
import test_secret_taint as base

pytestmark = pytest.mark.skipif(base._skip_reason() is not None, reason=base._skip_reason() or "")

STRADDLING, ALIGNED = 5, 32


@pytest.fixture(scope="module")
def reports():
    got, ends = base.unit_reports("vrf", ["cases", f"{STRADDLING}"], ["cases", f"{ALIGNED}"])
    assert ends == ["overflows=0"] * 2, f"{base.emul_build.MAD_OVERFLOW} ({ends})"
    return got


def test_cases_cover_both_lengths_and_sizes(reports):
    assert set(reports) == {f"prove/len{n_bytes}/n{n}" for n_bytes in (STRADDLING, ALIGNED) for n in (1, 6)}


def test_no_secret_branch(reports):
    bad = {case: sorted(r for r in rs if r.kind == "branch") for case, rs in reports.items()}
    assert not any(bad.values()), bad


def test_only_the_comb_row_fetch_takes_a_secret_address(reports):
    for case, rs in reports.items():
        bad = sorted(r for r in rs if r.kind == "address" and not ct_allowed.allows("address", r.function))
        assert not bad, (case, bad)
        assert {r.function for r in rs} == {"wb_load_pa_signed"}, (case, sorted(rs))

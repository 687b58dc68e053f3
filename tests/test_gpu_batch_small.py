"""GPU suite (MI355X): the host-pointer (*_batch) calls of tests/piece_cases.py at the sizes the piece suite does not reach, the
only ones where the pointers a wrapper receives are the pinned staging itself (csrc/host_pipeline.hpp run_batch): 1 row, the
one-element call that returns on the completion word; 3 and 64 rows, zero-copy calls (64 is ZERO_COPY_MAX_ROWS); 65 rows, the first
staged call.  Every row must be the models' (a call whose arrays together pass ZERO_COPY_MAX_BYTES is staged at any of these sizes,
with the same expectation), the guard row must survive and the inputs stay as they were.  Byte-exact: no tolerance is involved."""
import pytest

import piece_cases as pc
from curve25519_amd import _lib

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 64, 65)


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    return _lib.load()


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_small_calls(lib, family):
    arrays = pc.family_rows(family)
    for n in SIZES:
        results = pc.run_family(lib, family, arrays, n)
        assert len(results) == len(pc.CALLS[family]) + len(pc.in_place_variants(family))
        assert all(r["n"] == n and r["chunk"] == n for r in results)
        assert not pc.failures(results), (n, pc.failures(results)[:3])

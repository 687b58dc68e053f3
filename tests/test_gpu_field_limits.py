"""GPU suite: the raw-limb self-test hooks on the MI355X (include/curve25519_amd.h: c25519_amd_*_limb_selftest) with the edge inputs
of tests/limb_vectors.py -- the field code at the limits of its limb bound contract on one lane, a quad and a wave, through the real
v_mad_u64_u32 chains, DPP moves and permlane swaps.  Values are checked against Python big integers as on the model
(tests/test_field_limits.py), and the device's output limbs must be bit-identical to the model's: the same algorithm gives the same
limbs, so this is what shows the asm matches the C model at the limits."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import limb_vectors as lv  # noqa: E402
import test_field_limits as tfl  # noqa: E402

pytestmark = pytest.mark.gpu

ENTRY = {"lane": "c25519_amd_fe_limb_selftest", "quad": "c25519_amd_quad_limb_selftest", "wave": "c25519_amd_wave_limb_selftest"}


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "the GPU suite needs an MI355X"
    from curve25519_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def model():
    return tfl.load_model()


def run_device(_lib, shape, op, recs):
    recs = np.ascontiguousarray(recs, np.uint32)
    out = np.zeros((recs.shape[0], lv.OUT_WORDS), np.uint32)
    _lib.check(getattr(_lib.load(), ENTRY[shape])(out.ctypes.data, recs.ctypes.data, recs.shape[0], op), ENTRY[shape])
    return out


@pytest.mark.parametrize("shape,op", tfl.CASES, ids=[f"{s}-{tfl.SHAPES[s][1][o]}" for s, o in tfl.CASES])
def test_device_at_the_contract_limits(dev, model, shape, op):
    recs = tfl.SHAPES[shape][2](op)
    got = run_device(dev, shape, op, recs)
    red, small = tfl.bounds_for(shape, op)
    bad = lv.check(shape, op, recs, got, red, small)
    assert not bad, "\n".join(bad)
    exp = tfl.run_model(model, shape, op, recs)
    diff = np.nonzero((got != exp).any(axis=1))[0]
    assert diff.size == 0, f"{diff.size} records differ from the model's limbs, first {diff[:8].tolist()}"


def test_device_rejects_an_unknown_op(dev):
    recs = lv.lane_cases(0)[:1]
    out = np.zeros((1, lv.OUT_WORDS), np.uint32)
    assert dev.load().c25519_amd_wave_limb_selftest(out.ctypes.data, recs.ctypes.data, 1, 7) != 0

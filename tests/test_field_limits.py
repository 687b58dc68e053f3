"""CPU suite: the field arithmetic at the limits of its limb bound contract (curve25519_amd/csrc/fe25519.cuh), on the one-lane,
quad and wave code paths.  The raw-limb hooks take limb vectors directly -- no conversion from bytes, so operands can sit where
the kernels' worst cases put them (tests/limb_vectors.py builds them from tools/fe_bounds.py's own classes) -- and every output
is compared with Python big integers mod p.  Runs the device source compiled for the host against the C model of the gfx950
primitives (tests/host_emul/); tests/test_gpu_field_limits.py runs the same records on the device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import limb_vectors as lv  # noqa: E402
from host_emul.build import assert_no_mad_overflow, open_lib  # noqa: E402

SHAPES = {"lane": ("emul_fe_limb_op", lv.LANE_OPS, lv.lane_cases), "quad": ("emul_quad_limb_op", lv.QUAD_OPS, lv.quad_cases),
          "wave": ("emul_wave_limb_op", lv.WAVE_OPS, lv.wave_cases)}


def load_model():
    return open_lib({name: ([C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], None) for name, _, _ in SHAPES.values()})


@pytest.fixture(scope="module")
def model():
    lib = load_model()
    assert lib.emul_mad_overflow_count() == 0
    yield lib
    assert_no_mad_overflow(lib)


def run_model(lib, shape, op, recs):
    recs = np.ascontiguousarray(recs, np.uint32)
    out = np.zeros((recs.shape[0], lv.OUT_WORDS), np.uint32)
    getattr(lib, SHAPES[shape][0])(out.ctypes.data, recs.ctypes.data, recs.shape[0], op)
    return out


def bounds_for(shape, op):
    """(reduced bound, carry_small bound) the outputs of an op must meet."""
    if shape == "lane":
        return (lv.R if op in lv.LANE_REDUCED else None), None
    if shape == "wave" and op == 1:
        return None, lv.wave_small_bound()
    return lv.R, None


CASES = [(shape, op) for shape, (_, ops, _) in SHAPES.items() for op in ops]


@pytest.mark.parametrize("shape,op", CASES, ids=[f"{s}-{SHAPES[s][1][o]}" for s, o in CASES])
def test_outputs_at_the_contract_limits(model, shape, op):
    """Every output value is right mod p, its canonical words too, and every output the contract calls reduced stays within
    reduced_fixpoint() (carry_small's within its own named bound)."""
    before = model.emul_mad_overflow_count()
    recs = SHAPES[shape][2](op)
    out = run_model(model, shape, op, recs)
    red, small = bounds_for(shape, op)
    bad = lv.check(shape, op, recs, out, red, small)
    assert not bad, "\n".join(bad)
    assert model.emul_mad_overflow_count() == before


def test_carry_small_class_is_what_the_checker_names():
    """The wave's carry_small outputs form a limb class of their own (limb 0 up to ~1.10 x 2^26, above the reduced bound), which
    fe_bounds.py names and checks at every consumer; its general bound covers that class."""
    import fe_bounds as fb
    fb.coop_section(fb.reduced_fixpoint())
    small = fb.coop_small_class()
    assert small[0] > lv.R[0], "the class is above the reduced bound in limb 0"
    assert 1.09 < fb.beta(small) < 1.11
    assert all(s <= g for s, g in zip(small, lv.wave_small_bound()))


def test_ladder_steps_agree_across_shapes(model):
    """One lane, a quad and a wave run the ladder step on the same raw state: the same values (their limbs differ: different carry
    chains and signs), both bit choices, both forms of the base point."""
    for base9 in (False, True):
        recs = lv.quad_cases(1 if base9 else 0)
        lane = run_model(model, "lane", 15 if base9 else 14, recs)
        quad = run_model(model, "quad", 1 if base9 else 0, recs)
        wave = run_model(model, "wave", 3 if base9 else 2, recs[:48])
        assert np.array_equal(lane[:, 40:], quad[:, 40:])
        assert np.array_equal(lane[:48, 40:], wave[:, 40:])


def test_point_ops_agree_across_shapes(model):
    """ge_double on one lane, on a quad (lanes X, Y, T, Z) and on a wave (rows X, Y, Z, T): the same three coordinates X, Y, Z."""
    recs = lv.lane_cases(16)[:64]
    lane = run_model(model, "lane", 16, recs)
    quad_in = recs.copy()
    quad_in[:, 20:30], quad_in[:, 30:40] = recs[:, 30:40], recs[:, 20:30]
    quad = run_model(model, "quad", 3, quad_in)
    wave = run_model(model, "wave", 5, recs)
    for k_lane, k_quad in ((0, 0), (1, 1), (2, 3), (3, 2)):
        assert np.array_equal(lane[:, 40 + 8 * k_lane: 48 + 8 * k_lane], quad[:, 40 + 8 * k_quad: 48 + 8 * k_quad])
    assert np.array_equal(lane[:, 40:], wave[:, 40:])


BITE = r"""
import sys
sys.path[:0] = [{tests!r}]
import limb_vectors as lv, test_field_limits as t
lib = t.load_model()
recs = lv.lane_cases(0, scale=1.05)
out = t.run_model(lib, "lane", 0, recs)
print(len(lv.check("lane", 0, recs, out)), lib.emul_mad_overflow_count())
"""


def test_the_inputs_sit_at_the_edge():
    """Bite test: the same generator at 1.05 x the contract's maxima (fe_mul's b at beta 3.47, so 19 b wraps 32 bits) must produce
    wrong values on the model -- the cases above really are at the limit.  In a process of its own: the overflow it provokes must
    not count against the other tests."""
    code = BITE.format(tests=os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    wrong, _ = map(int, p.stdout.split())
    assert wrong > 0, "inputs at 1.05 x the contract's maxima all came out right: the edge cases are not at the edge"

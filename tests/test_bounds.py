"""CPU suite, part 5: worst-case limb bounds of the device field arithmetic.  tools/fe_bounds.py replays every
formula of the kernels on per-limb upper bounds and asserts that no 32-bit operand, 64-bit column or biased
subtraction can overflow for ANY input -- the random parity tests cannot show that."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fe_bound_contract_holds():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fe_bounds.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all bounds hold" in out.stdout


def test_checker_detects_a_violation():
    """The checker must actually bite: a multiplication whose operands are two subtractions deep overflows."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fe_bounds as fb
    R = fb.reduced_fixpoint()
    deep = fb.add(fb.sub(R, R), fb.sub(R, R))          # beta 6 on both sides
    try:
        fb.mul(deep, deep, "too deep")
    except fb.Bad:
        return
    raise AssertionError("bound checker accepted an overflowing multiplication")


def test_every_section_reports():
    """A section of the checker cannot quietly vanish: each prints its own line."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fe_bounds.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in ("x25519 ladder, inversion, encoding: ok", "edwards double / add / decompress / table build / encodings: ok",
                 "lattice verification walk, signed comb and blinded base walk: ok",
                 "quad25519 ladder step, addition, doubling, batch-inversion exchange: ok",
                 "coop25519 products, carries, ladder, two-wave ladder, mont_double, edwards add / double: ok",
                 "coop25519 carry_small output class: beta <= 1.1"):
        assert line in out.stdout, line


def _fb():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fe_bounds as fb
    return fb


def test_quad_section_detects_a_violation():
    """The quad ladder's level 2 multiplies two beta-3 operands against the 3.3 limit: one q_sub deeper must not pass."""
    fb = _fb()
    R = fb.reduced_fixpoint()
    fb.quad_ladder_step(R, fb.FROM_WORDS, False)
    try:
        fb.quad_ladder_step(R, fb.FROM_WORDS, False, deeper=1)
    except fb.Bad:
        return
    raise AssertionError("bound checker accepted a quad level-2 product one subtraction deeper")


def test_coop_section_detects_a_violation():
    """The wave's product pre-scales the multiplier by 38 in 32 bits: a multiplier at 1.05 x the contract's beta must not pass,
    nor may carry_small take a sum of 2^46."""
    fb = _fb()
    R = fb.reduced_fixpoint()
    fb.mul_level(fb.at_beta(fb.CONTRACT["mul_a"]), fb.at_beta(fb.CONTRACT["mul_b"]), "at the limit")
    for bad in (lambda: fb.mul_level(fb.at_beta(fb.CONTRACT["mul_a"]), fb.at_beta(1.05 * fb.CONTRACT["mul_b"]), "beyond"),
                lambda: fb.carry_small([fb.CARRY_SMALL_IN] + R[1:], "beyond")):
        try:
            bad()
        except fb.Bad:
            continue
        raise AssertionError("bound checker accepted a wave product or carry beyond its contract")

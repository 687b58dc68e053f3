"""The library is linked from build.ENGINE_UNITS; the resource tests and the ISA tools look at csrc/engine.hip, which includes the
units as one.  Both must name every csrc/engine_*.hip and nothing else, or the shipped kernels and the inspected ones come apart."""
import os
import re

from curve25519_amd import build


def test_every_engine_unit_is_built_and_included():
    on_disk = sorted(f[:-4] for f in os.listdir(build.CSRC) if re.fullmatch(r"engine_\w+\.hip", f))
    with open(os.path.join(build.CSRC, "engine.hip")) as f:
        included = re.findall(r'^#include "(\w+)\.hip"', f.read(), re.M)
    assert on_disk and sorted(build.ENGINE_UNITS) == on_disk
    assert sorted(included) == on_disk
    assert len(set(build.ENGINE_UNITS)) == len(build.ENGINE_UNITS) and len(set(included)) == len(included)

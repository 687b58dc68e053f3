"""The `usage` fixture of the tests/test_resources*.py modules: {demangled kernel name: record} from the compiler's own remarks
(tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage on engine.hip, cross-compiled for gfx950 -- no GPU
needed).  Each module imports the fixture from here; pytest sets it up once per importing module, and kernel_usage() is memoised, so
the engine is compiled once per process however many of the modules run."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import resource_usage  # noqa: E402
from resource_usage import regs, spill_free  # noqa: E402,F401


@pytest.fixture(scope="session")
def usage():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    return resource_usage.kernel_usage()

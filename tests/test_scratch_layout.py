"""The three public *_scratch_bytes functions against the formulas include/curve25519_amd.h prints for them, and the carver the
engine sizes and cuts every call's device scratch with (csrc/scratch_carve.hpp) on its own under the host sanitizers.  No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = (1, 3, 4, 5, 255, 256, 257, 65535, 65536, 65537, 1 << 20, 1 << 26)
WINDOWS = (None, 7, 8, 10, 13)


def r4(x):
    return (x + 3) // 4 * 4


def shape(n, window):
    """c, wa, wz, K of the header: the built-in width is 10 below 2^16 and 13 from there"""
    c = window if window is not None else (10 if n < 1 << 16 else 13)
    wa, wz = -(-255 // c), -(-130 // c)
    return wa, wz, (wa + 1) * 2 ** (c - 1)


# the formulas as the header prints them (whitespace aside): the functions below are these lines in Python
HEADER_FORMULAS = (
    "4 * (n * 640 + 4 * r4(10 n) + r4(14 n) + 2 * r4(5 n) + 5 * r4(n) + 4)",
    "4 * (2n * 40 + (K + wa + 1) * 40 + n * (wa + wz) + 16 * ceil(n / 256) + r4(n) + 2 K + 4)",
    "4 * (N * 40 + (K + wa + 1) * 40 + n * wz + n_key * wa + 16 * ceil(n / 256) + 16 * n_key + r4(N) + 2 K + 4)",
)


def verify_bytes(n):
    return 4 * (n * 640 + 4 * r4(10 * n) + r4(14 * n) + 2 * r4(5 * n) + 5 * r4(n) + 4)


def batch_bytes(n, window):
    wa, wz, K = shape(n, window)
    return 4 * (2 * n * 40 + (K + wa + 1) * 40 + n * (wa + wz) + 16 * -(-n // 256) + r4(n) + 2 * K + 4)


def indexed_bytes(n, n_key, window):
    wa, wz, K = shape(n, window)
    N = n_key + n
    return 4 * (N * 40 + (K + wa + 1) * 40 + n * wz + n_key * wa + 16 * -(-n // 256) + 16 * n_key + r4(N) + 2 * K + 4)


def test_the_header_prints_the_formulas_this_file_checks():
    text = " ".join(re.sub(r"^\s*\*", " ", open(os.path.join(ROOT, "include", "curve25519_amd.h")).read(), flags=re.M).split())
    for formula in HEADER_FORMULAS:
        assert formula in text, formula


@pytest.mark.parametrize("window", WINDOWS)
def test_public_scratch_sizes_equal_the_header_formulas(window):
    from curve25519_amd import _lib
    lib = _lib.load()
    with _lib.tunable("BATCH_EQ_WINDOW", -1 if window is None else window):
        for n in SIZES:
            assert lib.ed25519_VerifySignature_scratch_bytes(n) == verify_bytes(n), n
            assert lib.ed25519_VerifyBatch_scratch_bytes(n) == batch_bytes(n, window), (n, window)
            for n_key in (1, 7, 256, n):
                assert lib.ed25519_VerifyBatch_indexed_scratch_bytes(n, n_key) == indexed_bytes(n, n_key, window), (n, n_key, window)


def test_carver_sizing_and_carving_agree_under_the_host_sanitizers(tmp_path):
    """tests/c/scratch_carve_test.cpp: the sizing pass and the carving pass of one sequence of take / align / proj calls end at the
    same offset, the parts are disjoint and aligned as asked, and the sizing pass forms no pointer (address and undefined-behaviour
    sanitizers on a stand-alone host program: nothing is loaded into python)"""
    exe = str(tmp_path / "scratch_carve_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "curve25519_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "scratch_carve_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "scratch_carve_test ok" in out.stdout

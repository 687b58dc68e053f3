"""CPU suite, part 2: the drop-in boundary.  The C-ABI library must load without a GPU, export every
symbol the headers in include/ declare, fail loudly (error code + message, never a CPU result) when
asked to compute without a device, and the product package must not touch the oracle."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


HEADERS = ("curve25519_dh.h", "ed25519_signature.h", "curve25519_amd.h")
PREFIXES = ("curve25519_", "ed25519_", "c25519_", "ristretto255_")


def declared_functions():
    names = set()
    for h in HEADERS:
        text = open(os.path.join(ROOT, "include", h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        for m in re.finditer(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", text):
            name = m.group(1)
            if name.startswith(PREFIXES):
                names.add(name)
    return sorted(names)


def declared_prototypes():
    """{name: [parameter text, ...]} of every function the three headers declare (`(void)` is no parameter)"""
    protos = {}
    for h in HEADERS:
        text = open(os.path.join(ROOT, "include", h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*|^\s*#[^\n]*", "", text, flags=re.M)
        for m in re.finditer(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(([^()]*)\)\s*;", text):
            name, params = m.group(1), " ".join(m.group(2).split())
            if name.startswith(PREFIXES):
                assert name not in protos, f"{name} is declared twice"
                protos[name] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return protos


def test_headers_declare_the_reference_api():
    names = declared_functions()
    for must in ("curve25519_dh_CalculatePublicKey", "curve25519_dh_CalculatePublicKey_fast",
                 "curve25519_dh_CreateSharedKey", "ed25519_CreateKeyPair", "ed25519_SignMessage",
                 "ed25519_Blinding_Init", "ed25519_Blinding_Finish", "ed25519_VerifySignature",
                 "ed25519_Verify_Init", "ed25519_Verify_Check", "ed25519_Verify_Finish"):
        assert must in names
    text = open(os.path.join(ROOT, "include", "ed25519_signature.h")).read()
    for macro, val in (("ed25519_public_key_size", 32), ("ed25519_secret_key_size", 32),
                       ("ed25519_private_key_size", 64), ("ed25519_signature_size", 64)):
        assert re.search(rf"#define\s+{macro}\s+{val}\b", text)


def test_library_exports_every_declared_symbol():
    from curve25519_amd import _lib
    lib = _lib.load()
    for name in declared_functions():
        assert hasattr(lib, name), f"{name} declared in include/ but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature in curve25519_amd/_lib.py"
    assert b"gfx950" in lib.c25519_amd_version()
    # per element: the larger of the two per-lane table formats (two 9-row window tables of the fast path in packed
    # 128-byte rows, 576 words; the reference-order kernels' 16-row 4-fold table of 40-limb rows is 640), the (X, Y, Z, prefix) projective scratch (the fast path's decoded points), and the
    # fast path's scalars (sigma as 14 words of comb columns, rho, tau), flags, slow list, the walk's element order, the quad path's two point flags and the counters
    r4 = lambda x: (x + 3) // 4 * 4  # noqa: E731
    for n in (64, 65, 1 << 20):
        words = n * 640 + 4 * r4(10 * n) + r4(14 * n) + 2 * r4(5 * n) + 5 * r4(n) + 4
        assert lib.ed25519_VerifySignature_scratch_bytes(n) == 4 * words


def test_ctypes_signatures_match_the_prototypes():
    """every declared function: as many argtypes as the prototype has parameters, and a pointer type exactly where the parameter
    has a `*` -- a missing size_t in the table is a wrong call, not an error"""
    from curve25519_amd import _lib
    protos = declared_prototypes()
    assert sorted(protos) == declared_functions() and len(protos) >= 180
    for name, params in protos.items():
        argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(params), (name, params, argtypes)
        for i, (p, t) in enumerate(zip(params, argtypes)):
            assert (t in (C.c_void_p, C.c_char_p)) == ("*" in p), (name, i, p, t)


def test_headers_compile_as_c_and_cxx(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "curve25519_dh.h"\n#include "ed25519_signature.h"\n#include "curve25519_amd.h"\n'
                   "int main(void){unsigned char b[ed25519_signature_size]; return sizeof b == 64 ? 0 : 1;}\n")
    for cc, flags in (("gcc", ["-std=c99", "-pedantic", "-Werror"]), ("g++", ["-x", "c++", "-Werror"])):
        subprocess.check_call([cc, *flags, "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                               str(tmp_path / "t.o")])


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from curve25519_amd import _lib, api
    lib = _lib.load()
    assert lib.c25519_amd_device_count() == 0
    sk = np.zeros((2, 32), np.uint8)
    with pytest.raises(_lib.EngineError):
        api.curve25519_dh_CreateSharedKey(sk, sk)
    with pytest.raises(_lib.EngineError):
        api.ed25519_CreateKeyPair(sk)
    assert lib.c25519_amd_last_error() != b""
    # n == 0 is a no-op everywhere, even without a device
    assert lib.curve25519_dh_CreateSharedKey_batch(sk.ctypes.data, sk.ctypes.data, sk.ctypes.data, 0) == 0


def test_product_does_not_use_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline may touch oracle/."""
    pkg = os.path.join(ROOT, "curve25519_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cuh", ".hpp", ".h", ".c", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                code = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith(("#", "//", "*", '"""')))
                assert "oracle_lib" not in code and "liborc25519" not in code and "orc25519.h" not in code, f
    for h in os.listdir(os.path.join(ROOT, "include")):
        assert "orc_" not in open(os.path.join(ROOT, "include", h)).read()
    out = subprocess.check_output(["ldd", os.path.join(pkg, "libcurve25519_amd.so")], text=True)
    assert "liborc" not in out and "curve25519_ref" not in out


def test_bench_self_launch_fails_only_for_lack_of_devices():
    """`python bench.py --gpus 2` (no torchrun, the driver's invocation) must get past the launcher logic: on this
    GPU-less box the only acceptable failure is the device count."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, env=env)
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        assert p.returncode == 0
    else:
        assert p.returncode != 0
        assert "GPU(s)" in p.stderr and "launch with torch.distributed.run" not in p.stderr


def test_roofline_denominator_is_the_half_rate_mad_peak():
    """bench.py prices the kernels against the accumulating v_mad_u64_u32 rate of tools/ubench/mad_peak (whole-asm loop,
    128 per trip) as committed under profiles/: plain half rate, 35-40 T lane-MAC/s on MI355X -- not the 28-32 T of a
    16-per-trip loop that earlier rounds divided by.  Guards the denominator and its source."""
    sys.path.insert(0, ROOT)
    import bench
    peak, src = bench.measured_mad_peak()
    assert src and src.endswith("_mad_peak.json"), src
    assert 35e12 < peak < 40e12, peak
    rates = json.load(open(os.path.join(ROOT, "profiles", src)))["rates"]
    assert rates["mad_acc_16_aligned"] < 0.85 * peak, "the short-loop artefact is part of the record"
    assert abs(rates["v_mul_lo_u32"] / peak - 1) < 0.06, "MAD and the other half-rate instructions issue at the same rate"

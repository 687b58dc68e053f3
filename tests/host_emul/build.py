"""Builds the host-emulation libraries of tests/host_emul: device headers of curve25519_amd/csrc compiled by g++ against the C model
of the gfx950 primitives (valu_model.h).  build() gives libc25519_emul.so (emul.cpp), build_lib() any of them; open_lib() loads one
for a test.  A library is rebuilt when a file the compiler read for it (its -MMD list, kept next to it as <lib>.d) has changed.
build_taint() gives the secret-taint programs (taint_<unit>.cpp over taint_harness.h): stand-alone MemorySanitizer builds by the ROCm
clang, run as subprocesses by tests/test_secret_taint.py and never loaded into python.
TEST INFRASTRUCTURE -- see valu_model.h."""
import concurrent.futures
import ctypes
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "curve25519_amd", "csrc")
LIB = os.path.join(HERE, "libc25519_emul.so")
# run in HERE with relative paths, so that the dependency file names relative paths and holds wherever the tree is copied
CXX = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
       "-include", "valu_model.h", "-I", "../../curve25519_amd/csrc", "-I", "."]
MAD_OVERFLOW = "a v_mad_u64_u32 column wrapped 2^64: the bound contract is broken"


def stale(lib: str) -> bool:
    """the library or its dependency file is missing, or a file named there (the source and valu_model.h among them) is missing or
    newer than the library"""
    if not (os.path.exists(lib) and os.path.exists(lib + ".d")):
        return True
    with open(lib + ".d") as f:
        deps = f.read().replace("\\\n", " ").partition(":")[2].split()
    built = os.path.getmtime(lib)
    deps = [os.path.join(HERE, d) for d in deps]
    return not deps or any(not os.path.exists(d) or os.path.getmtime(d) > built for d in deps)


def build_lib(source: str, lib_name: str, extra_include_dirs=(), force: bool = False) -> str:
    """tests/host_emul/<source> -> tests/host_emul/<lib_name>, if it is stale or force is set; returns the library's path"""
    lib = os.path.join(HERE, lib_name)
    if not force and not stale(lib):
        return lib
    tmp, dep = f"{lib_name}.tmp.{os.getpid()}", f"{lib_name}.d.tmp.{os.getpid()}"
    includes = [a for d in extra_include_dirs for a in ("-I", os.path.relpath(d, HERE))]
    subprocess.check_call([*CXX, *includes, "-MMD", "-MF", dep, source, "-o", tmp, "-lpthread"], cwd=HERE)
    os.replace(os.path.join(HERE, dep), lib + ".d")
    os.replace(os.path.join(HERE, tmp), lib)
    return lib


# ---- the secret-taint programs ----------------------------------------------------------------------------------------------
TAINT_UNITS = ("emul", "sign_ctx", "peer_ctx", "one_peer", "key_convert")
TAINT_DIR = os.path.join(HERE, "taint_bin")
# -O1: at -O0 every ?: is a branch; MemorySanitizer instruments AFTER the IR optimisations, so a source branch the optimiser turns
# into a select is not reported (the GPU compiler does the same with it).  Without -fno-sanitize-memory-param-retval a secret passed
# by value is itself a report.
TAINT_FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=memory", "-fsanitize-recover=memory", "-fno-sanitize-memory-param-retval",
               "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
               "-include", "valu_model.h", "-I", "../../curve25519_amd/csrc", "-I", "."]
# a second build of every unit that checks branch conditions only: a report it gives is a BRANCH, one only the full build gives is an
# ADDRESS (MemorySanitizer's message is the same for both)
TAINT_BRANCH_ONLY = ["-mllvm", "-msan-check-access-address=0"]
TAINT_JOBS = 16


def taint_toolchain():
    """(clang++, llvm-symbolizer) of the ROCm LLVM with a MemorySanitizer runtime, or (None, reason)"""
    roots = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm")]
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm"))
    for root in roots:
        cxx, sym = os.path.join(root, "bin", "clang++"), os.path.join(root, "bin", "llvm-symbolizer")
        if not (os.path.exists(cxx) and os.path.exists(sym)):
            continue
        for d, _, files in os.walk(os.path.join(root, "lib", "clang")):
            if any(f.startswith("libclang_rt.msan") and f.endswith(".a") for f in files):
                return cxx, sym
        return None, f"{root} has no libclang_rt.msan"
    return None, "no ROCm clang++ with llvm-symbolizer"


def build_taint(units=TAINT_UNITS, force: bool = False) -> dict:
    """{(unit, kind): program} for kind in ("full", "branch"), built where stale, at most TAINT_JOBS compilers at a time"""
    cxx, _ = taint_toolchain()
    if cxx is None:
        raise RuntimeError("no MemorySanitizer toolchain")
    os.makedirs(TAINT_DIR, exist_ok=True)
    out, jobs = {}, []
    for unit in units:
        for kind, extra in (("full", []), ("branch", TAINT_BRANCH_ONLY)):
            prog = os.path.join(TAINT_DIR, f"taint_{unit}_{kind}")
            out[(unit, kind)] = prog
            if force or stale(prog):
                jobs.append((unit, prog, extra))

    def compile_one(job):
        unit, prog, extra = job
        rel = os.path.relpath(prog, HERE)
        tmp, dep = f"{rel}.tmp.{os.getpid()}", f"{rel}.d.tmp.{os.getpid()}"
        subprocess.check_call([cxx, *TAINT_FLAGS, *extra, "-MMD", "-MF", dep, f"taint_{unit}.cpp", "-o", tmp, "-lpthread"], cwd=HERE)
        os.replace(os.path.join(HERE, dep), prog + ".d")
        os.replace(os.path.join(HERE, tmp), prog)

    if jobs:
        with concurrent.futures.ThreadPoolExecutor(min(TAINT_JOBS, os.cpu_count() or 1, len(jobs))) as pool:
            list(pool.map(compile_one, jobs))
    return out


def build(force: bool = False) -> str:
    return build_lib("emul.cpp", os.path.basename(LIB), force=force)


def open_lib(functions=None, source: str = "emul.cpp", lib_name: str = os.path.basename(LIB), extra_include_dirs=(), mad_counter: bool = True):
    """Builds the library if needed and opens it.  functions: {name: argtypes} or {name: (argtypes, restype)}; a name given without
    a restype keeps ctypes' int.  mad_counter: the library has valu_model.h's overflow counter (every one that multiplies does)."""
    lib = ctypes.CDLL(build_lib(source, lib_name, extra_include_dirs))
    if mad_counter:
        lib.emul_mad_overflow_count.restype = ctypes.c_ulonglong
    for name, sig in (functions or {}).items():
        fn = getattr(lib, name)
        if isinstance(sig, tuple):
            fn.argtypes, fn.restype = sig
        else:
            fn.argtypes = sig
    return lib


def assert_no_mad_overflow(lib):
    assert lib.emul_mad_overflow_count() == 0, MAD_OVERFLOW


if __name__ == "__main__":
    print(build(force=True))

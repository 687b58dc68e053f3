"""The compile-time names the device sources test (#if / #ifdef / #ifndef / #elif on C25519_*) are the build's shape
parameters and hooks, nothing else.  A decided A/B experiment keeps its record under profiles/ and leaves no switch behind in
the headers every kernel change is read against; a new name needs a line here with its reason."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "curve25519_amd", "csrc")

ALLOWED = {
    # shape parameters
    "C25519_ED_BLOCK": "lanes per workgroup of the Ed25519 batch kernels",
    "C25519_VI_WAVES": "waves per SIMD the register allocator aims at: Verify_Init",
    "C25519_VC_WAVES": "waves per SIMD: Verify_Check",
    "C25519_VW_WAVES": "waves per SIMD: the verification walk",
    "C25519_VD_WAVES": "waves per SIMD: the point decoding and window-table kernel",
    "C25519_XF_WAVES": "waves per SIMD: the fused X25519 kernel",
    "C25519_XF_BLOCK": "lanes per workgroup of the fused X25519 kernel",
    "C25519_WALK_BLOCK": "lanes per verification-walk workgroup (they share one staged comb table)",
    "C25519_WALK_COMB_TEETH": "teeth of the walk's signed comb for sigma * B",
    # build hooks
    "C25519_VALU_PRIMITIVES": "the host emulator's C model of valu_gfx950.cuh (tests/host_emul)",
    "C25519_LAT_COUNT": "the host emulator's loop-trip counters of the lattice reduction",
    "C25519_CYCLE_PROBE": "the in-kernel cycle probe of the measurement library bench.py loads",
    # a size-dependent trade-off: both sides live, the host emulator runs both
    "C25519_INDEXED_REPACK": "aligned copy of the indexed Verify_Check rows (profiles/indexed_check_ab.txt)",
}

DIRECTIVE = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$")


def directive_names():
    names = {}
    for f in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, f)
        if not os.path.isfile(path):
            continue
        with open(path, encoding="utf-8") as fh:
            for ln, line in enumerate(fh, 1):
                m = DIRECTIVE.match(line)
                if m:
                    for name in re.findall(r"\bC25519_\w+", m.group(1).split("//")[0]):
                        names.setdefault(name, f"{f}:{ln}")
    return names


def test_compile_time_names_are_the_allowed_ones():
    names = directive_names()
    extra = {n: names[n] for n in sorted(set(names) - set(ALLOWED))}
    missing = sorted(set(ALLOWED) - set(names))
    assert not extra, f"compile-time switches outside the allow-list (first use): {extra}"
    assert not missing, f"allow-listed names no longer tested by any directive: {missing}"

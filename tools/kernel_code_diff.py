#!/usr/bin/env python3
"""tools/kernel_code_diff.py -- did a source change leave the kernels' gfx950 code alone?

    python tools/kernel_code_diff.py --old A.s [A2.s ...] --new B.s [B2.s ...] [--allow NAME ...]

The inputs are `hipcc <build.FLAGS> --cuda-device-only -S` outputs of the translation units before and after the change.  Per kernel
symbol (a function with an .amdhsa_kernel record) the instruction lines and local labels are kept, comments and directives dropped,
and the two numbers that depend on where in its file a function stands are renumbered: the function index in .LBB<f>_<n> and the
counter in .Lpost_getpc<n>.  Nothing else is normalised: a register, an operand, an instruction moved by one place is a difference.
One line per kernel: same / differs / only-old / only-new, with the instruction counts of both sides.  A symbol that several files
of a side emit (the k_batch_invert instantiations) is compared copy by copy: `same` means that every copy of either side has an
identical copy on the other.  Exit status 1 if any kernel differs or is missing on a side, unless --allow names it (the whole
symbol, or the function's plain name: k_ed25519_verify_check_coop).  The text is compared as text: no disassembly, no look at what an
instruction does.
"""
import argparse
import re
import sys


def plain_name(sym):
    """_Z26k_ed25519_verify_init_coopPKvm... -> k_ed25519_verify_init_coop; a symbol that is not mangled this way stays"""
    m = re.match(r"_Z(\d+)", sym)
    return sym[m.end():m.end() + int(m.group(1))] if m else sym


def kernels(text):
    """{symbol: (tuple of normalised lines, instruction count)} of one assembly file"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, sym = {}, None
    for l in text.split("\n"):
        l = l.split(";")[0].rstrip()
        if sym is None:                                                    # between functions: wait for a kernel's own label
            if l.endswith(":") and l[:-1] in names:
                sym, lines, getpc = l[:-1], [], {}
            continue
        if l.startswith(".Lfunc_end"):
            out[sym] = (tuple(lines), sum(not x.endswith(":") for x in lines))
            sym = None
            continue
        l = l.strip()
        if not l or (l.startswith(".") and not l.endswith(":")):           # blank, comment or directive
            continue
        l = re.sub(r"\.LBB\d+_", ".LBB_", l)
        l = re.sub(r"\.Lpost_getpc(\d+)", lambda g: ".Lpost_getpc#%d" % getpc.setdefault(g.group(1), len(getpc)), l)
        lines.append(re.sub(r"\s+", " ", l))
    return out


def side(paths):
    """{symbol: [copy, ...]} over the files of one side"""
    out = {}
    for p in paths:
        with open(p) as f:
            for sym, k in kernels(f.read()).items():
                out.setdefault(sym, []).append(k)
    return out


def counts(copies):
    return "/".join(str(n) for _, n in copies) if copies else "-"


def compare(old, new):
    """[(status, symbol, old counts, new counts)], sorted by symbol"""
    rows = []
    for sym in sorted(set(old) | set(new)):
        o, n = old.get(sym, []), new.get(sym, [])
        status = "only-old" if not n else "only-new" if not o else "same" if {c for c, _ in o} == {c for c, _ in n} else "differs"
        rows.append((status, sym, counts(o), counts(n)))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True, metavar="FILE.s")
    ap.add_argument("--new", nargs="+", required=True, metavar="FILE.s")
    ap.add_argument("--allow", nargs="*", default=[], metavar="NAME", help="kernels that may differ or be missing")
    a = ap.parse_args(argv)
    rows = compare(side(a.old), side(a.new))
    bad = 0
    for status, sym, o, n in rows:
        allowed = status != "same" and (sym in a.allow or plain_name(sym) in a.allow)
        bad += status != "same" and not allowed
        print(f"{status:9s}{' (allowed)' if allowed else ''} {o:>11s} -> {n:<11s} {plain_name(sym)}  {sym}")
    tally = {s: sum(r[0] == s for r in rows) for s in ("same", "differs", "only-old", "only-new")}
    print(f"# {len(rows)} kernels: " + ", ".join(f"{v} {k}" for k, v in tally.items()) + f"; {bad} not allowed")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the device assembly of two source trees: what a refactor that claims "every kernel
disassembles identically to the parent's" has to show.

Every .hip of both directories is compiled to gfx950 assembly (tools/lint_vmcnt.py's compile_to_asm, i.e. the
library's optimisation level) and split into kernels (its parse_kernels).  Basic-block labels are renumbered per
kernel in order of appearance, so that a kernel that merely moved inside its file still compares equal.  Per file:
kernels on one side only, the count of identical kernels, and for each differing kernel its instruction count and
register / scratch / LDS / occupancy figures on both sides.

usage: isa_diff.py OLD_CSRC NEW_CSRC      (exit code 1 when the kernel name sets differ)
       e.g.  git worktree add DIR HEAD~1 && tools/isa_diff.py DIR/cbinfer_amd/csrc cbinfer_amd/csrc"""
import glob
import os
import re
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lint_vmcnt import compile_to_asm, parse_kernels  # noqa: E402

FIGURES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def normalised(body):
    """The instruction texts of one kernel with its local labels renumbered in order of appearance."""
    names = {}
    return [LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), ins) for _, ins, _ in body]


def figures(asm, kernels):
    """{kernel: {figure: value}} from the '; NumVgprs: 128' comment lines the compiler leaves behind each kernel."""
    out, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", line)
        if m and m.group(1) in kernels:
            name = m.group(1)
            out[name] = {}
        m = re.match(r"^;\s*(\w+):\s*(\d+)", line)
        if m and name and m.group(1) in FIGURES:
            out[name].setdefault(m.group(1), int(m.group(2)))
    return out


def disassemble(src, tmp, tag):
    out = os.path.join(tmp, tag + "_" + os.path.basename(src) + ".s")
    compile_to_asm(src, out)
    asm = open(out).read()
    kernels = parse_kernels(asm)
    return {k: normalised(b) for k, b in kernels.items()}, figures(asm, kernels)


def demangled(names):
    import subprocess
    try:
        txt = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, txt.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old_dir, new_dir = sys.argv[1:]
    files = sorted({os.path.basename(f) for d in (old_dir, new_dir) for f in glob.glob(os.path.join(d, "*.hip"))})
    status = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(int(os.environ.get("ISA_DIFF_JOBS", "8"))) as pool:
        jobs = {(f, tag): pool.submit(disassemble, os.path.join(d, f), tmp, tag)
                for f in files for tag, d in (("old", old_dir), ("new", new_dir)) if os.path.exists(os.path.join(d, f))}
        for f in files:
            if (f, "old") not in jobs or (f, "new") not in jobs:
                print("%-18s only in %s" % (f, old_dir if (f, "old") in jobs else new_dir))
                status = 1
                continue
            (old, oldfig), (new, newfig) = jobs[f, "old"].result(), jobs[f, "new"].result()
            differ = [k for k in old if k in new and old[k] != new[k]]
            print("%-18s %3d kernel(s): %d identical, %d differ" % (f, len(old), len(set(old) & set(new)) - len(differ),
                                                                    len(differ)))
            for side, only in (("old", set(old) - set(new)), ("new", set(new) - set(old))):
                for k, name in sorted(demangled(sorted(only)).items()):
                    print("    only in %s: %s" % (side, name))
                    status = 1
            for k, name in demangled(differ).items():
                print("    differs: %s" % name)
                for side, body, fig in (("old", old[k], oldfig[k]), ("new", new[k], newfig[k])):
                    print("        %s %6d instructions  " % (side, sum(not i.endswith(":") for i in body)) +
                          "  ".join("%s %d" % (n, fig.get(n, -1)) for n in FIGURES))
    return status


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Is the device code of two builds of the library the same?  tools/compare_device_code.py <lib A> <lib B> [--show N]

For every kernel of the gfx950 code object of both libraries (__graft_entry__.kernel_resources / kernel_isa):
  * the same set of kernel names;
  * the same vgpr_count, sgpr_count, spill counts, private_segment_fixed_size and group_segment_fixed_size;
  * the same instruction stream (disassembly, addresses and encodings stripped) after ONE normalisation: the 32-bit literal of the
    s_add_u32 that directly follows an s_getpc_b64 is a pc-relative address of something outside the kernel -- it moves whenever an
    earlier kernel of the code object changes its size or its place, so it is masked.
Prints the number of kernels, the differing ones with their instruction and register counts (and the first --show differing lines), and
exits with status 1 on any difference. The check a refactor of the host side, a move of source text or a retired switch
(tools/strip_switches.py) has to pass: no GPU needed, build both libraries and compare.
"""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
PC_LITERAL = re.compile(r"^(s_add_u32\s+\S+\s+\S+\s+)\S+$")


def instructions(lines):
    """the instruction texts of one kernel's disassembly, pc-relative literals masked"""
    out = []
    for line in lines:
        ins = " ".join(line.split("//")[0].split())
        if not ins or ins.endswith(":") or ins.startswith("Disassembly") or "file format" in ins:
            continue
        if out and out[-1].startswith("s_getpc_b64"):
            ins = PC_LITERAL.sub(r"\1<pc-relative>", ins)
        out.append(ins)
    return out


def describe(lib):
    res = ge.kernel_resources(lib)
    isa = ge.kernel_isa(lib, sorted(res))
    return {k: ({f: res[k].get(f) for f in FIELDS}, instructions(isa[k])) for k in res}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    ap.add_argument("--show", type=int, default=3, help="differing instruction lines printed per kernel")
    a = ap.parse_args()
    A, B = describe(a.lib_a), describe(a.lib_b)
    only_a, only_b = sorted(set(A) - set(B)), sorted(set(B) - set(A))
    differing = 0
    for k in sorted(set(A) & set(B)):
        (ra, ia), (rb, ib) = A[k], B[k]
        if ra == rb and ia == ib:
            continue
        differing += 1
        print("DIFFERS %s\n    A: %d instructions %s\n    B: %d instructions %s" % (k, len(ia), ra, len(ib), rb))
        shown = 0
        for i, (x, y) in enumerate(zip(ia, ib)):
            if x != y and shown < a.show:
                print("    [%d] %s   |   %s" % (i, x, y))
                shown += 1
    for k in only_a:
        print("ONLY IN A %s" % k)
    for k in only_b:
        print("ONLY IN B %s" % k)
    print("%d kernels in A, %d in B; only in A: %d, only in B: %d; differing: %d" % (len(A), len(B), len(only_a), len(only_b), differing))
    return 1 if (only_a or only_b or differing) else 0


if __name__ == "__main__":
    sys.exit(main())

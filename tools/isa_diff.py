#!/usr/bin/env python3
"""Compare the kernels of two `hipcc -S` outputs of one translation unit, opcode by opcode:

    python tools/isa_diff.py before.s after.s

One row per kernel: instruction count, VGPRs, SGPRs, scratch, LDS and code bytes of AFTER (`old>new` where BEFORE differs) and a verdict —
`identical` (the same instruction lines once branch labels are renumbered), `same opcode histogram`, or the opcodes whose counts differ."""
import collections
import re
import sys

META = (("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
        ("lds", r"; LDSByteSize: (\d+)"), ("code", r"; codeLenInByte = (\d+)"))


def kernels(path):
    """{name: (instruction lines, {resource: value})} for every function of the file."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:\n(.*?)^; Occupancy", text, re.S | re.M):
        lines = [ln.split(";")[0].strip() for ln in m.group(2).split("\n")]
        ins = [re.sub(r"\.LBB\d+_\d+", "L", ln) for ln in lines if ln and not ln.startswith(".") and not ln.endswith(":")]
        out[m.group(1)] = (ins, {k: int(re.search(rx, m.group(3)).group(1)) for k, rx in META})
    return out


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    print("| kernel | instr | vgpr | sgpr | scratch | lds | code | verdict |\n|---|---|---|---|---|---|---|---|")
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("| %s | only in %s |" % (name, sys.argv[1] if name in a else sys.argv[2]))
            continue
        (ia, ma), (ib, mb) = a[name], b[name]
        ha, hb = (collections.Counter(ln.split()[0] for ln in i) for i in (ia, ib))
        if ia == ib:
            verdict = "identical"
        elif ha == hb:
            verdict = "same opcode histogram"
        else:
            verdict = " ".join("%s%+d" % (op, hb[op] - ha[op]) for op in sorted(set(ha) | set(hb)) if ha[op] != hb[op])
        cols = [len(ib) if len(ia) == len(ib) else "%d>%d" % (len(ia), len(ib))] + [mb[k] if ma[k] == mb[k] else "%d>%d" % (ma[k], mb[k]) for k, _ in META]
        print("| %s | %s | %s |" % (name, " | ".join(str(c) for c in cols), verdict))

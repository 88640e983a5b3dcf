#!/usr/bin/env python3
"""Compare the kernels of two `hipcc -S` outputs of one translation unit, opcode by opcode:

    python tools/isa_diff.py [--arith] before.s after.s

One row per kernel: instruction count, VGPRs, SGPRs, scratch, LDS and code bytes of AFTER (`old>new` where BEFORE differs) and a verdict —
`identical` (the same instruction lines once branch labels are renumbered), `same opcode histogram`, or the opcodes whose counts differ.
--arith adds a line per kernel for refactors that may move address code only: whether the counts of every matrix, LDS, memory, barrier,
conversion and floating-point opcode (ARITH) equal BEFORE's, scratch is not above BEFORE's, LDS is equal and AFTER has at most 256 VGPRs; exit 1 if not."""
import collections
import re
import sys

META = (("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
        ("lds", r"; LDSByteSize: (\d+)"), ("code", r"; codeLenInByte = (\d+)"))
# what a refactor of a kernel's structure must leave alone (integer, address, compare / select, move, scalar, s_nop and s_waitcnt may differ)
ARITH = re.compile(r"^(v_mfma|ds_|global_|buffer_|flat_|scratch_|s_barrier|v_exp_|v_cvt)|^v_.*_(f16|f32|f64|bf16)")


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
    arith = "--arith" in sys.argv
    files = [x for x in sys.argv[1:] if x != "--arith"]
    a, b = kernels(files[0]), kernels(files[1])
    broken = []
    print("| kernel | instr | vgpr | sgpr | scratch | lds | code | verdict |\n|---|---|---|---|---|---|---|---|")
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("| %s | only in %s |" % (name, files[0] if name in a else files[1]))
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
        if arith:
            moved = [op for op in sorted(set(ha) | set(hb)) if ha[op] != hb[op] and ARITH.search(op)]
            ok = not moved and mb["scratch"] <= ma["scratch"] and ma["lds"] == mb["lds"] and mb["vgpr"] <= 256
            broken += [] if ok else [name]
            print("|  | arith: %d of %d instructions, counts %s; scratch %d -> %d; lds %d = %d; vgpr %d -> %d: %s |" % (
                sum(n for op, n in hb.items() if ARITH.search(op)), len(ib), "differ in " + " ".join(moved) if moved else "equal",
                ma["scratch"], mb["scratch"], ma["lds"], mb["lds"], ma["vgpr"], mb["vgpr"], "ok" if ok else "BROKEN"))
    if arith:
        print("kernels that break a condition: %d %s" % (len(broken), " ".join(broken)))
        sys.exit(1 if broken else 0)

"""Static instruction classes per LOOP of one kernel in a saved .s file (hipcc -save-temps): what a ray pays besides its arithmetic.
    python tools/asm_loop_stats.py <file.s> <kernel name substring> [min instructions per loop = 400]
A loop is the span from a label to the last backward branch that targets it; nested spans are listed innermost first, and an outer
span's counts include its inner loops'.  Per loop: instructions, basic blocks (labels + 1) and the largest one, scalar loads (s_load*),
conditional branches, v_readlane / v_writelane (SGPR spill traffic and lane moves), s_waitcnt, flat against global stores and loads,
LDS-DMA loads (global_load_lds*), 64-bit VALU address adds (v_lshl_add_u64), MFMAs."""
import re
import sys


def main():
    s = open(sys.argv[1]).read()
    m = re.search(r"^(\S*" + re.escape(sys.argv[2]) + r"\S*):", s, re.M)
    if not m:
        sys.exit(f"no kernel matching {sys.argv[2]}")
    body = s[m.start():s.index(".end_amdhsa_kernel", m.start())].split("\n")
    mn = int(sys.argv[3]) if len(sys.argv) > 3 else 400
    ins, labels = [], {}            # (opcode, operand text) in order; label -> index of its first instruction
    for ln in body:
        mm = re.match(r"^(\.LBB\d+_\d+):", ln)
        if mm:
            labels[mm.group(1)] = len(ins)
            continue
        t = ln.split(";")[0].split()
        if ln.startswith("\t") and t and not t[0].startswith("."):
            ins.append((t[0], " ".join(t[1:])))
    starts = sorted(set(labels.values()))
    loops = {}
    for i, (op, arg) in enumerate(ins):
        if op.startswith(("s_cbranch", "s_branch")) and arg in labels and labels[arg] <= i:
            loops[labels[arg]] = max(loops.get(labels[arg], 0), i)
    print(m.group(1))
    cols = ("insts", "blocks", "maxblk", "s_load", "cbranch", "readlane", "writelane", "waitcnt", "flat_st", "glob_st", "flat_ld", "glob_ld", "lds_dma",
            "add_u64", "mfma")
    print("span              " + " ".join(f"{c:>9s}" for c in cols))
    for a, b in sorted(loops.items(), key=lambda ab: ab[1] - ab[0]):
        if b - a + 1 < mn:
            continue
        ops = [op for op, _ in ins[a:b + 1]]
        cuts = [a] + [x for x in starts if a < x <= b] + [b + 1]
        n = lambda f: sum(1 for op in ops if f(op))
        row = (len(ops), len(cuts) - 1, max(y - x for x, y in zip(cuts, cuts[1:])), n(lambda o: o.startswith("s_load")), n(lambda o: o.startswith("s_cbranch")),
               n(lambda o: o.startswith("v_readlane")), n(lambda o: o.startswith("v_writelane")), n(lambda o: o.startswith("s_waitcnt")),
               n(lambda o: o.startswith("flat_store")), n(lambda o: o.startswith("global_store")), n(lambda o: o.startswith("flat_load")),
               n(lambda o: o.startswith("global_load") and "_lds_" not in o), n(lambda o: o.startswith("global_load_lds")),
               n(lambda o: o.startswith("v_lshl_add_u64")), n(lambda o: o.startswith("v_mfma")))
        print(f"[{a:6d},{b:6d}]   " + " ".join(f"{v:9d}" for v in row))


if __name__ == "__main__":
    main()

"""Static comparison of two builds' device assembly (the *-gfx950.s files hipcc -save-temps leaves in the object directory):
    python tools/asm_compare.py PARENT_DIR CHILD_DIR [--table NAME]
Per translation unit and kernel: is the instruction stream the parent's once comments, label numbers and the compilation unit's id
symbol are taken out?  Kernels on one side only are listed.  A template parameter appended with its default (render_kernel_p's
DYN = false) renames every instantiation: a kernel is matched by its name or by its name without one trailing `Lb0E`.
--table NAME: VGPRs / spilled VGPRs / spilled SGPRs / scratch bytes of every kernel whose demangled name contains NAME, both sides."""
import os
import re
import shutil
import subprocess
import sys


def kernels(path):
    """{mangled name: instruction lines}, {mangled name: metadata record} of one assembly file"""
    code, meta, name, body, rec = {}, {}, None, [], None
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
        elif name is not None:
            if ".end_amdhsa_kernel" in line:
                code[name], name = body, None
            else:
                s = line.split(";")[0].rstrip()
                if s.strip() and not s.lstrip().startswith(".amdhsa_"):
                    body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", s))
        m = re.match(r"^\s+(- )?\.(agpr_count|name|private_segment_fixed_size|sgpr_spill_count|vgpr_count|vgpr_spill_count):\s*(\S+)", line)
        if m:
            if m.group(2) == "agpr_count":
                rec = {}
            elif rec is not None:
                rec[m.group(2)] = m.group(3)
                if m.group(2) == "vgpr_spill_count":
                    meta[rec["name"]] = rec
    return code, meta


def main():
    pa, ch = sys.argv[1], sys.argv[2]
    want = sys.argv[sys.argv.index("--table") + 1] if "--table" in sys.argv else None
    same = diff = new = 0
    for f in sorted(os.listdir(ch)):
        if not f.endswith("gfx950.s") or not os.path.exists(os.path.join(pa, f)):
            continue
        (kp, tp), (kc, tc) = kernels(os.path.join(pa, f)), kernels(os.path.join(ch, f))

        def parent_of(n):
            if n in kp:
                return n
            m = n.replace("Lb0EEEv", "EEv", 1)
            return m if m in kp else None
        names = sorted(set(kp) | set(kc))
        filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
        r = subprocess.run([filt] + names, capture_output=True, text=True) if filt and names else None
        dm = dict(zip(names, r.stdout.splitlines())) if r is not None and r.returncode == 0 else {n: n for n in names}
        rows, matched = [], set()
        for n in sorted(kc):
            p = parent_of(n)
            if p is None:
                new += 1
                rows.append(f"  new       {dm[n]}")
                continue
            matched.add(p)
            a, b = [x.replace(p, "K") for x in kp[p]], [x.replace(n, "K") for x in kc[n]]
            if a == b:
                same += 1
            else:
                diff += 1
                nd = sum(1 for x, y in zip(a, b) if x != y) + abs(len(a) - len(b))
                rows.append(f"  DIFFERENT {dm[n]}  ({len(a)} -> {len(b)} lines, {nd} differ)")
        rows += [f"  gone      {dm[n]}" for n in kp if n not in matched]
        print(f"{f}: {len(kc)} kernels" + ("" if rows else ", every one the parent's instruction stream"))
        if rows:
            print("\n".join(rows))
        if want:
            def fmt(t):
                return "-" if not t else f"{t['vgpr_count']} / {t['vgpr_spill_count']} / {t['sgpr_spill_count']} / {t['private_segment_fixed_size']}"
            for n in sorted(kc):
                if want in dm[n]:
                    short = dm[n].replace("void bts::", "").replace("(bts::FwdParams)", "")
                    print(f"    {short:<72s} parent {fmt(tp.get(parent_of(n) or '')):>22s}   this tree {fmt(tc.get(n)):>22s}")
    print(f"kernels with the parent's instruction stream: {same}; different: {diff}; new: {new}")


if __name__ == "__main__":
    main()

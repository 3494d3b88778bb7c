"""Compare the device code of two builds of one unit, kernel by kernel, instruction by instruction.

    hipcc <HIPFLAGS of the Makefile without -MMD -MP> -DRCG_SYS=Sys3WRobot -DRCG_SYS_VT=kVt3WRobot -DRCG_SYS_PART=4 \
          --cuda-device-only -S rcognita_amd/csrc/rcg_sys_inst.hip -o A.s                      (in each tree)
    python3 tools/compare_disasm.py A.s B.s k_actor_search [--show 12]

For every kernel both files have whose (mangled) name contains the pattern: the instruction counts, the number of lines a
diff of the two instruction streams marks, how many of those are not scalar loads (the kernel-argument loads a moved argument
offset changes), the mnemonics of the marked lines and their multiset difference, and the first `--show` marked lines.  Labels,
directives and comments are left out; register numbers are not normalised, so a renumbering shows as a difference.
Exit status 0 when every compared kernel differs in scalar loads and `s_add_u32` (offset arithmetic) only, 1 otherwise.
"""
import collections
import difflib
import re
import sys

FUNC = re.compile(r"^(_Z\w+):")


def read(path):
    out, cur = {}, None
    with open(path, errors="replace") as f:
        for line in f:
            m = FUNC.match(line)
            if m:
                cur = out.setdefault(m.group(1), [])
                continue
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            s = line.split(";")[0].strip()
            if cur is None or not s or s.startswith(".") or s.endswith(":"):
                continue
            cur.append(re.sub(r"\s+", " ", s))
    return out


def main(argv):
    show = int(argv[argv.index("--show") + 1]) if "--show" in argv else 12
    args = [a for i, a in enumerate(argv[1:], 1) if not a.startswith("--") and argv[i - 1] != "--show"]
    a, b, pat = read(args[0]), read(args[1]), args[2]
    names = sorted(k for k in set(a) & set(b) if pat in k)
    bad = 0
    for k in names:
        x, y = a[k], b[k]
        marked = [l for l in difflib.unified_diff(x, y, lineterm="", n=0) if l[0] in "+-" and not l.startswith(("+++", "---"))]
        mnem = lambda l: l[1:].split(" ")[0]
        other = [l for l in marked if not mnem(l).startswith("s_load_dword")]
        ca, cb = collections.Counter(l.split(" ")[0] for l in x), collections.Counter(l.split(" ")[0] for l in y)
        multiset = {m: cb[m] - ca[m] for m in set(ca) | set(cb) if ca[m] != cb[m]}
        offsets_only = all(mnem(l) == "s_add_u32" for l in other) and not multiset
        bad += not offsets_only
        print(f"{k}\n  instructions {len(x)} / {len(y)}; marked lines {len(marked)}, not scalar loads {len(other)}; mnemonics of the "
              f"marked lines {sorted(set(map(mnem, marked)))}; counts that differ {multiset or 'none'}; "
              f"{'argument offsets only' if offsets_only else 'MORE THAN ARGUMENT OFFSETS'}")
        for l in other[:show]:
            print("     " + l)
    print(f"{len(names)} kernels compared, {bad} differ in more than argument offsets")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

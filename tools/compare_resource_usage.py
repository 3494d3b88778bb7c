"""Compare the kernels of two builds by their resource usage.

    make -O -j8 lib HIPCC="hipcc -Rpass-analysis=kernel-resource-usage" > A.log 2>&1     (in each tree)
    python3 tools/compare_resource_usage.py A.log B.log

Reads the compiler's `kernel-resource-usage` remarks of both logs and reports, per kernel (mangled name), every figure that
differs: SGPRs, VGPRs, AGPRs, spills, scratch, occupancy, LDS.  Kernels that exist in one log only are listed.  `make -O` keeps
the output of one compilation together (without it the remarks of parallel compilations interleave and cannot be attributed);
the compilations of the -DRCG_DEV twin, whose kernels carry the same names, are left out.  Exit status 0 when every kernel
both logs have is unchanged and neither log has a kernel of its own (`--allow-new`: the second log may), 1 otherwise.
"""
import re
import sys

KEY = re.compile(r"remark:\s+(?:Function Name: (\S+)|([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)) \[-Rpass-analysis")


def read(path):
    out, cur, skip = {}, None, False
    with open(path, errors="replace") as f:
        for line in f:
            if "remark:" not in line and " -c " in line and "--offload-arch" in line:  # the echo of a compile command
                skip, cur = "-DRCG_DEV" in line, None
            m = None if skip else KEY.search(line)
            if not m:
                continue
            if m.group(1):
                cur = out.setdefault(m.group(1), {})
            elif cur is not None:
                cur[m.group(2).strip()] = m.group(3)
    return out


def main(argv):
    allow_new = "--allow-new" in argv
    paths = [a for a in argv[1:] if not a.startswith("--")]
    a, b = read(paths[0]), read(paths[1])
    common = sorted(set(a) & set(b))
    differ = [(k, {f: (a[k].get(f), b[k].get(f)) for f in set(a[k]) | set(b[k]) if a[k].get(f) != b[k].get(f)}) for k in common]
    differ = [(k, d) for k, d in differ if d]
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    print(f"{len(a)} kernels in {paths[0]}, {len(b)} in {paths[1]}, {len(common)} in both; {len(differ)} differ, "
          f"{len(only_a)} only in the first, {len(only_b)} only in the second")
    for k, d in differ:
        print("DIFFERS", k, d)
    for k in only_a:
        print("ONLY-FIRST", k)
    for k in only_b:
        print("ONLY-SECOND", k)
    bad = bool(differ or only_a or (only_b and not allow_new))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

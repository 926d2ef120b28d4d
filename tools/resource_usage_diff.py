#!/usr/bin/env python3
"""Compare the compiler's kernel resource usage of two builds of the kernel files.

Compile each file once per tree with the flags of nanort_amd/csrc/Makefile plus `-Rpass-analysis=kernel-resource-usage`
(add `-DNRT_PROF=1 -DNRT_ROCTX=1` for the profiling instantiations), one compile per log so that the remarks of two
compilers do not interleave; with `-S --cuda-device-only` the assembly gives the code length as well:

    hipcc $HIPFLAGS -Rpass-analysis=kernel-resource-usage -S --cuda-device-only traverse.hip -o traverse.s 2> traverse.log

    tools/resource_usage_diff.py parent/traverse.log,parent/traverse.s branch/traverse.log,branch/traverse.s

Each side is a comma-separated list of remark logs and assembly files (any number of source files: a kernel that moved from one
file to another is found by its mangled name).  `--kernels REGEX` picks the kernels by their demangled names (default
`k_traverse`).  Prints one markdown row per kernel: VGPRs, SGPRs, scratch bytes per lane, waves per SIMD, LDS bytes per block
and code bytes (`-` without assembly) of both builds, and whether they are the same.  A kernel whose mangled name exists on
one side only is paired with one of the same demangled name without its parameter list, and the row says that the name differs.
A kernel that gained template parameters, all `false` in the instantiation at hand (`k<16, true>` -> `k<16, true, false>`, `k` ->
`k<false>`: a feature switch added at its off position), is paired the same way.  A kernel that exists in the second build only
is printed with its figures; `--allow-new` lets such kernels pass.

Exit status 1 when a PLAIN instantiation of k_traverse_wide differs in any figure, or any other kernel changed its waves per SIMD
or gained scratch, or a kernel has no partner (`--allow-new`: has none in the second build); with `--strict`, when anything differs
at all.
"""
import argparse
import re
import subprocess
import sys

FIELDS = (("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "waves"),
          ("LDS Size [bytes/block]", "lds"))
KEYS = [k for _, k in FIELDS] + ["code"]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def parse(paths):
    kernels = {}
    for path in paths.split(","):
        cur = asm = None
        for line in open(path, errors="replace"):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = kernels.setdefault(m.group(1), {})
                continue
            m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
            if m:
                asm = kernels.setdefault(m.group(1), {})
                continue
            m = re.match(r"; codeLenInByte = (\d+)", line)
            if m and asm is not None:
                asm["code"] = int(m.group(1))
                asm = None
                continue
            if cur is None:
                continue
            for label, key in FIELDS:
                m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
                if m:
                    cur[key] = int(m.group(1))
    return kernels


def is_plain(name):
    # k_traverse_wide<T, STACK, STATS, KIND, PLAIN, CLOCK, WIDTH, ORDER>: the fifth template argument
    m = re.search(r"k_traverse_wide<([^>]*)>", name)
    if not m:
        return None
    args = [a.strip() for a in m.group(1).split(",")]
    return len(args) > 4 and args[4] == "true"


def short_name(name):
    return re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "")).replace("void ", "").replace("nrt::", "")


def without_trailing_false(short):
    """`k<16, false, false>` -> [`k<16, false>`, `k<16>`], `k<false>` -> [`k`]: the names it may have had before template
    parameters were added at `false`, the longest first."""
    m = re.match(r"(.*?)<(.*)>$", short)
    if not m:
        return []
    args = [a.strip() for a in m.group(2).split(",")]
    out = []
    while args and args[-1] == "false":
        args.pop()
        out.append(m.group(1) + ("<" + ", ".join(args) + ">" if args else ""))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("first")
    ap.add_argument("second")
    ap.add_argument("--kernels", default="k_traverse", help="regular expression over the demangled kernel names")
    ap.add_argument("--strict", action="store_true", help="any difference fails")
    ap.add_argument("--allow-new", action="store_true", help="a kernel of the second build without a partner in the first does not fail")
    o = ap.parse_args()
    a, b = parse(o.first), parse(o.second)
    names = demangle(sorted(set(a) | set(b)))
    rows = []  # (short name, plain, first figures, second figures, same mangled name)
    alone = {}
    for mangled, name in names.items():
        if not re.search(o.kernels, name):
            continue
        if mangled in a and mangled in b:
            rows.append((short_name(name), is_plain(name), a[mangled], b[mangled], True))
        else:
            alone.setdefault(short_name(name), {})["a" if mangled in a else "b"] = (a.get(mangled) or b.get(mangled))
    # a kernel of the first build whose partner gained template parameters at `false`: one row under the new name
    for short in sorted((k for k, v in alone.items() if "a" not in v), key=len):
        for old in without_trailing_false(short):
            if old in alone and "b" not in alone[old]:
                alone[short]["a"] = alone.pop(old)["a"]
                break
    for short, sides in alone.items():
        rows.append((short, None, sides.get("a"), sides.get("b"), False))
    bad = 0
    print("| kernel | PLAIN | VGPRs | SGPRs | scratch | waves/SIMD | LDS | code bytes | same |")
    print("|---|---|---|---|---|---|---|---|---|")
    for short, plain, x, y, same_name in sorted(rows, key=lambda r: r[0]):
        if x is None or y is None:
            z = x or y
            cells = ["%d" % z[k] if z.get(k) is not None else "-" for k in KEYS]
            print("| `%s` | - | %s | only in %s |" % (short, " | ".join(cells), "the second" if x is None else "the first"))
            if y is None or not o.allow_new:
                bad = 1
            continue
        same = all(x.get(k) == y.get(k) for k in KEYS)
        cells = []
        for k in KEYS:
            if x.get(k) is None and y.get(k) is None:
                cells.append("-")
            elif x.get(k) == y.get(k):
                cells.append("%d" % x[k])
            else:
                cells.append("%s -> %s" % (x.get(k, "-"), y.get(k, "-")))
        verdict = ("yes" if same else "no") + ("" if same_name else " (mangled name differs)")
        print("| `%s` | %s | %s | %s |" % (short, {None: "-", True: "yes", False: "no"}[plain], " | ".join(cells), verdict))
        if (plain or o.strict) and not same:
            bad = 1
        if not plain and (x["waves"] != y["waves"] or y["scratch"] > x["scratch"]):
            bad = 1
    return bad


if __name__ == "__main__":
    sys.exit(main())

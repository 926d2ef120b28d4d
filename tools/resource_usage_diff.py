#!/usr/bin/env python3
"""Compare the compiler's kernel resource-usage remarks of two builds of traverse.hip.

Compile the file once per tree with the flags of nanort_amd/csrc/Makefile plus
`-Rpass-analysis=kernel-resource-usage` (add `-DNRT_PROF=1 -DNRT_ROCTX=1` for the profiling instantiations), one
compile per log so that the remarks of two compilers do not interleave:

    hipcc $HIPFLAGS -Rpass-analysis=kernel-resource-usage -c traverse.hip -o /dev/null 2> log

    tools/resource_usage_diff.py parent.log branch.log

prints one markdown row per k_traverse* kernel: VGPRs, SGPRs, scratch bytes per lane, waves per SIMD and LDS bytes per
block of both builds, and whether they are the same.  Exit status 1 when a PLAIN instantiation differs in any figure or a
non-PLAIN one changed its waves per SIMD or gained scratch.
"""
import re
import subprocess
import sys

FIELDS = (("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "waves"),
          ("LDS Size [bytes/block]", "lds"))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def parse(path):
    kernels, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
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


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    names = demangle(sorted(set(a) | set(b)))
    bad = 0
    print("| kernel | PLAIN | VGPRs | SGPRs | scratch | waves/SIMD | LDS | same |")
    print("|---|---|---|---|---|---|---|---|")
    for mangled, name in sorted(names.items(), key=lambda kv: kv[1]):
        if "k_traverse" not in name:
            continue
        short = re.sub(r"\(.*$", "", name).replace("void nrt::", "").replace("(nrt::TraverseArgs", "")
        x, y = a.get(mangled), b.get(mangled)
        if x is None or y is None:
            print("| `%s` | | only in %s | | | | | no |" % (short, "the second" if x is None else "the first"))
            bad = 1
            continue
        plain = is_plain(name)
        same = x == y
        cells = ["%d" % x[k] if x[k] == y[k] else "%d -> %d" % (x[k], y[k]) for _, k in FIELDS]
        print("| `%s` | %s | %s | %s |" % (short, {None: "-", True: "yes", False: "no"}[plain], " | ".join(cells), "yes" if same else "no"))
        if plain and not same:
            bad = 1
        if not plain and (x["waves"] != y["waves"] or y["scratch"] > x["scratch"]):
            bad = 1
    return bad


if __name__ == "__main__":
    sys.exit(main())

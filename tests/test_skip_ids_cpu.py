"""Per-ray skip ids (include/nanort_hip.h, "per-ray skip ids"), the parts that need no GPU: the library exports the new entry
points and the header declares exactly them; include/nanort.h compiles with the new trailing arguments with and without
NANORT_USE_HIP_BACKEND; and the header's host TraverseBatch(rays, n, intersector, ..., skip_prim_ids) equals per-ray Traverse()
with per-ray options (tests/cpp/skip_ids_check.cc: 576 triangles in two sheets, 1500 rays, sentinel / out-of-range / foreign ids mixed in)."""
import os
import re
import subprocess

from nanort_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "tests", "cpp", "skip_ids_check.cc")

SKIP_SYMBOLS = sorted(
    "%s_%s" % (name, sfx)
    for name in ("nrtTraverseBatchSkip", "nrtTraverseBatchSkipDevice", "nrtOccludedBatchSkip", "nrtOccludedBatchSkipDevice",
                 "nrtTraverseBatchesSkipDevice", "nrtTraverseBatchesSkip")
    for sfx in ("f32", "f64"))


def cxx(args):
    r = subprocess.run(["g++"] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "g++ %s failed:\n%s" % (" ".join(args), r.stdout[-3000:])


def test_library_exports_and_header_declares_exactly_the_skip_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    exported = sorted(s for s in re.findall(r" T (nrt\w+)", out) if "Skip" in s)
    assert exported == SKIP_SYMBOLS
    header = open(os.path.join(INC, "nanort_hip.h")).read()
    declared = sorted(s for s in set(re.findall(r"NRT_API\s+[\w\s\*]+?\b(nrt\w+)\s*\(", header)) if "Skip" in s)
    assert declared == SKIP_SYMBOLS
    assert all(s in capi.SYMBOLS for s in SKIP_SYMBOLS)
    L = capi.lib()  # (the ctypes rows: one more pointer than the call without ids)
    for sfx in ("f32", "f64"):
        for name, base in (("nrtTraverseBatchSkip_", "nrtTraverseBatch_"), ("nrtTraverseBatchSkipDevice_", "nrtTraverseBatchDevice_"),
                           ("nrtOccludedBatchSkip_", "nrtOccludedBatch_"), ("nrtOccludedBatchSkipDevice_", "nrtOccludedBatchDevice_"),
                           ("nrtTraverseBatchesSkipDevice_", "nrtTraverseBatchesDevice_"), ("nrtTraverseBatchesSkip_", "nrtTraverseBatches_")):
            assert len(getattr(L, name + sfx).argtypes) == len(getattr(L, base + sfx).argtypes) + 1


def test_header_compiles_with_the_backend(tmp_path):
    cxx(["-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-DNANORT_USE_HIP_BACKEND", "-D__HIP_PLATFORM_AMD__", "-I", INC, "-c", SRC, "-o",
         str(tmp_path / "skip_ids_check_hip.o")])


def test_host_fallback_equals_per_ray_traverse_with_per_ray_options(tmp_path):
    exe = tmp_path / "skip_ids_check"
    cxx(["-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "batch_vs_per_ray_mismatches 0" in r.stdout and "skipped_triangle_reported 0" in r.stdout, r.stdout
    m = re.search(r"rays (\d+) faces (\d+) wave1_hits (\d+) wave2_hits (\d+)", r.stdout)
    rays, faces, hit1, hit2 = (int(x) for x in m.groups())
    assert faces >= 300 and hit1 * 10 >= rays * 8 and hit2 * 10 >= rays * 8, r.stdout  # (not vacuous: most rays hit in both waves)

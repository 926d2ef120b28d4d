"""The combined ray query without a GPU (include/nanort_hip.h, "one descriptor for every triangle ray query"): the
four entry points and the descriptor in the library, the header and the binding table; include/nanort.h's QueryTriangleIntersector,
BatchQuery and host TraverseBatchQuery (tests/cpp/query_check.cc) with and without the backend; the conditions the GPU tests'
fixtures rest on (tests/query_fixture.py); the fixture's expectation against the three existing ones where only one feature is on;
and the scratch of the new kernel instantiations against k_traverse_motion's, from the compiler's resource remarks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import masks_fixture as kf
import motion_fixture as mf
import own_walks_fixture as ow
import query_fixture as qf
from helpers import assert_hits_identical, trace_options
from nanort_amd import capi
from nanort_amd.wire import hit_dtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "tests", "cpp", "query_check.cc")
CSRC = os.path.join(ROOT, "nanort_amd", "csrc")
REALS = [np.float32, np.float64]
IDS = ["f32", "f64"]
NAMES = tuple(base + sfx for base in ("nrtQueryBatch_", "nrtQueryBatchDevice_") for sfx in ("f32", "f64"))
FIELDS = ("struct_size", "flags", "rays", "num_rays", "options", "skip_prim_ids", "times", "ray_masks", "hits_out", "mask_out")


def cxx(args):
    r = subprocess.run(["g++"] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "g++ %s failed:\n%s" % (" ".join(args), r.stdout[-3000:])


@pytest.fixture(scope="module")
def worlds(oracle):
    """The two worlds per precision with their figures, computed once for the file."""
    out = {}
    for real in REALS:
        for name, make in (("shells", qf.shells), ("pile", qf.pile)):
            w = make(oracle, real)
            out[(name, np.dtype(real).name)] = (w, w.figures(oracle))
    return out


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_library_header_and_binding_table_carry_the_four_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r" T (nrt\w+)", out))
    header = open(os.path.join(INC, "nanort_hip.h")).read()
    L = capi.lib()
    for name in NAMES:
        assert name in exported and name in capi.SYMBOLS and ("NRT_API nrt_status %s(" % name) in header, name
        assert not any(word in name for word in ("Skip", "Masked", "Motion")), name  # (the older ABI tests filter the exports on these)
        assert len(getattr(L, name).argtypes) == (3 if "Device" in name else 2), name
    assert sorted(exported) == sorted(capi.SYMBOLS)


def test_descriptor_layout_agrees_between_ctypes_and_the_header(tmp_path):
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nanort_hip.h"', "int main(void) {"]
    for s in ("f32", "f64"):
        lines.append('  printf("%s %%zu", sizeof(nrt_ray_query_%s));' % (s, s))
        lines += ['  printf(" %%zu", offsetof(nrt_ray_query_%s, %s));' % (s, k) for k in FIELDS]
        lines.append('  printf("\\n");')
    lines.append('  printf("flags %u %u %u\\n", NRT_QUERY_OCCLUSION, NRT_QUERY_MOTION, NRT_QUERY_MASKED);')
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src), "-o", str(exe)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    want = [ctypes.sizeof(capi.RayQuery)] + [getattr(capi.RayQuery, k).offset for k in FIELDS]
    assert [k for k, _ in capi.RayQuery._fields_] == list(FIELDS)
    for line, s in zip(out, ("f32", "f64")):
        words = line.split()
        assert words[0] == s and [int(x) for x in words[1:]] == want, (line, want)
    assert want[0] == 72
    assert out[2].split() == ["flags", str(capi.NRT_QUERY_OCCLUSION), str(capi.NRT_QUERY_MOTION), str(capi.NRT_QUERY_MASKED)]
    header = open(os.path.join(INC, "nanort_hip.h")).read()
    assert "static_assert(sizeof(nrt_ray_query_f32) == 72 && sizeof(nrt_ray_query_f64) == 72" in header


def test_null_context_and_descriptor_are_refused_without_a_device():
    L = capi.lib()
    q = capi.RayQuery(ctypes.sizeof(capi.RayQuery), 0, 16, 1, None, None, None, None, 16, None)
    for s in ("f32", "f64"):
        assert getattr(L, "nrtQueryBatch_" + s)(None, ctypes.addressof(q)) == capi.NRT_ERR_INVALID
        assert getattr(L, "nrtQueryBatchDevice_" + s)(None, ctypes.addressof(q), None) == capi.NRT_ERR_INVALID
        assert getattr(L, "nrtQueryBatch_" + s)(None, None) == capi.NRT_ERR_INVALID


# ---- 2. include/nanort.h --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", [[], ["-DNANORT_USE_HIP_BACKEND", "-D__HIP_PLATFORM_AMD__"]], ids=["host", "backend"])
def test_header_compiles_with_and_without_the_backend(tmp_path, backend):
    cxx(["-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror"] + backend + ["-I", INC, "-c", SRC, "-o", str(tmp_path / "query_check.o")])
    if backend:  # ... and the program tests/test_gpu_query.py runs against the GPU
        cxx(["-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror"] + backend + ["-I", INC, "-c", os.path.join(ROOT, "tests", "cpp", "query_backend_check.cc"),
             "-o", str(tmp_path / "query_backend_check.o")])


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("query_check") / "query_check")
    cxx(["-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", exe])
    return exe


FEATURES = {"motion": 2, "masked": 4, "ids": 8, "motion+ids": 10, "masked+ids": 12, "motion+masked": 6, "all": 14, "all, culled": 14}


@pytest.mark.parametrize("features", sorted(FEATURES))
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_host_batch_query_equals_per_ray_traverse_the_old_intersectors_and_the_expectation(oracle, worlds, host_check, tmp_path, real, features):
    """tests/cpp/query_check.cc on the shells: the host TraverseBatchQuery equals per-ray Traverse() with a QueryTriangleIntersector,
    and with one feature alone the Motion / Masked intersectors (the program's exit status); its records equal the fixture's
    expectation over the same tree (here).  The 'all' arm runs with an id range that takes a band out of the outer shell, the
    'all, culled' arm with the GPU test's options: a range inside the innermost shell and back-face culling, which from a point
    between the shells leave next to nothing (measured: one hit)."""
    w, _ = worlds[("shells", np.dtype(real).name)]
    bits = FEATURES[features]
    motion, masked, ids = bool(bits & 2), bool(bits & 4), bool(bits & 8)
    o = qf.shell_options() if features == "all, culled" else trace_options(range_=(50, 3900), skip=412) if features == "all" else trace_options(skip=412)
    mesh, tree, rp, out = (os.path.join(str(tmp_path), x) for x in ("mesh.bin", "tree.bin", "rays.bin", "out.bin"))
    with open(mesh, "wb") as fp:
        fp.write(np.array([w.v.shape[0], w.f.shape[0]], dtype=np.uint32).tobytes() + w.v.tobytes() + w.v1.tobytes() + w.f.tobytes() + w.pm.tobytes())
    with open(tree, "wb") as fp:  # BVHAccel::Load's format
        fp.write(np.array([w.nodes.shape[0]], dtype=np.uint64).tobytes() + np.ascontiguousarray(w.nodes).tobytes()
                 + np.array([w.idx.shape[0]], dtype=np.uint64).tobytes() + np.ascontiguousarray(w.idx, dtype=np.uint32).tobytes())
    with open(rp, "wb") as fp:
        fp.write(np.array([w.rays.shape[0]], dtype=np.uint64).tobytes() + w.rays.tobytes() + w.times.tobytes() + w.words.tobytes() + w.ids.tobytes())
    oo = o[()] if o.shape == () else o[0]
    r = subprocess.run([host_check, "f32" if real == np.float32 else "f64", mesh, tree, rp, out, str(int(oo["prim_ids_range"][0])),
                        str(int(oo["prim_ids_range"][1])), str(int(oo["skip_prim_id"])), str(int(oo["cull_back_face"])), str(bits)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:])
    raw = open(out, "rb").read()
    H = hit_dtype(real)
    n = w.rays.shape[0]
    h = np.frombuffer(raw, H, n, 0)
    m = np.frombuffer(raw, np.uint8, n, n * H.itemsize)
    eh, em = w.expected(oracle, motion=motion, masked=masked, ids=ids, opts=o)
    assert em.sum() > (0 if features == "all, culled" else 100)
    assert_hits_identical(eh, em, h, m)


# ---- 3. the fixture conditions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_fixture_condition_shells_every_feature_matters(worlds, real):
    """Measured with the oracle, f32 and f64 alike: 4096 faces, the reference's tree 21 deep, 3153 groups; the all-three query hits on
    70.2 % of the rays and never names the skipped primitive; it differs from the query without ids on 83.5 %, without masks on
    55.8 %, at time 0 on 43.6 %, from all three at once on 17.3 % (16.0 % as hits).  A tenth is asked for: a kernel that dropped any
    one of the three would be seen."""
    w, (h, m, _, all_three) = worlds[("shells", np.dtype(real).name)]
    assert w.f.shape[0] == 4096 and w.rays.shape[0] == qf.SHELL_RAYS
    assert qf.num_groups(real, w.times, w.words, w.ids) > 1000
    assert float(all_three.mean()) >= qf.SHELL_MIN_ALL_THREE, float(all_three.mean())
    assert float((all_three & (m != 0)).mean()) >= qf.SHELL_MIN_ALL_THREE
    assert not ((m != 0) & (h["prim_id"] == w.ids)).any()
    assert (w.ids != qf.NO_ID).mean() > 0.5 and (w.ids == qf.NO_ID).any()


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_fixture_condition_pile_every_feature_matters_past_the_lds_stack(worlds, real):
    """Measured: 156 groups, 1318 of the 1500 rays hit, on 322 all three features matter (150 asked for); the oracle's max-stack
    counter over the whole query is 137 — past the walk's 32 LDS entries, in the slot's spill array."""
    w, (h, m, depth, all_three) = worlds[("pile", np.dtype(real).name)]
    assert w.stats["max_tree_depth"] > ow.PILE_MIN_STACK
    assert int(all_three.sum()) >= qf.PILE_MIN_ALL_THREE, int(all_three.sum())
    assert depth > ow.PILE_MIN_STACK, depth
    assert m.sum() > 0 and not ((m != 0) & (h["prim_id"] == w.ids)).any()


# ---- 4. one feature on: the existing expectations -------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_expectation_with_one_feature_is_the_existing_expectation(oracle, worlds, real):
    w, _ = worlds[("shells", np.dtype(real).name)]
    o = trace_options(range_=(50, 3900), skip=412, cull=False)
    # MOTION alone
    assert_hits_identical(*mf.expected(oracle, w.nodes, w.idx, w.v, w.v1, w.f, w.rays, w.times, o), *w.expected(oracle, masked=False, ids=False, opts=o))
    # MASKED alone (keyframe 0)
    assert_hits_identical(*kf.expected(oracle, w.nodes, w.idx, w.v, w.f, w.pm, w.rays, w.words, o), *w.expected(oracle, motion=False, ids=False, opts=o))
    # ids alone: per ray, the options with that ray's id (the per-ray skip id contract)
    eh, em = w.expected(oracle, motion=False, masked=False, opts=o)
    sel = np.arange(0, w.rays.shape[0], 41)
    for i in sel:
        oi = o.copy()
        oi["skip_prim_id"] = w.ids[i]
        h1, m1 = oracle.traverse(w.nodes, w.idx, w.v, w.f, w.rays[i:i + 1], oi)
        assert_hits_identical(h1, m1, eh[i:i + 1], em[i:i + 1])
    # nothing on: the plain query
    assert_hits_identical(*oracle.traverse(w.nodes, w.idx, w.v, w.f, w.rays, o), *w.expected(oracle, motion=False, masked=False, ids=False, opts=o))
    # the flags decide, not the arrays: MOTION off ignores the times, MASKED off the words
    assert_hits_identical(*w.expected(oracle, motion=False, masked=False, ids=False), *oracle.traverse(w.nodes, w.idx, w.v, w.f, w.rays))


# ---- 5. the kernels' scratch ----------------------------------------------------------------------------------------------------------
def _scratch(path):
    """{demangled-enough kernel name: scratch bytes per lane} from hipcc's kernel-resource-usage remarks for one file."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")  # the product flags, as the Makefile states them
    args = re.search(r"^HIPFLAGS := (.*)$", text, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    assert "-ffp-contract=off" in args and "-O3" in args, args
    r = subprocess.run([hipcc] + args + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", path, "-o", os.devnull],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stdout[-3000:]
    out, name = {}, None
    for line in r.stdout.splitlines():
        f = re.search(r"Function Name: (\S+)", line)
        if f:
            name = f.group(1)
        s = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if s and name:
            out[name] = int(s.group(1))
    return out


def test_no_new_instantiation_uses_more_scratch_than_the_motion_walk():
    query = motion = _scratch("own_walks.hip")  # (every own walk is an instantiation of that one file)
    for t in ("f", "d"):  # the mangled template argument of the precision: If / Id
        base = [v for k, v in motion.items() if "k_traverse_motionI" + t in k]
        new = {k: v for k, v in query.items() if "k_traverse_queryI" + t in k}
        assert len(base) == 1 and len(new) == 3, (motion, query)
        assert all(v <= base[0] for v in new.values()), (new, base)

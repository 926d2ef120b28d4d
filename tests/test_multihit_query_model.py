"""Multi-hit with per-ray skip ids, visibility words and motion times without a GPU (include/nanort_hip.h, nrtMultiHitQueryBatch*;
DESIGN.md 3.16): the expectation of tests/multihit_query_fixture.py against the two it composes (multihit_fixture.model with
nothing on, query_fixture.expected at K = 1); include/nanort.h's MultiHitBatchQuery and host MultiHitTraverseBatchQuery
(tests/cpp/multihit_query_check.cc); the four entry points and the descriptor in the library, the header and the binding table; and
the conditions the GPU tests' fixtures rest on."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import multihit_fixture as mhf
import multihit_query_fixture as mq
import own_walks_fixture as ow
import query_fixture as qf
from nanort_amd import capi
from nanort_amd.wire import hit_dtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "tests", "cpp", "multihit_query_check.cc")
REALS = [np.float32, np.float64]
IDS = ["f32", "f64"]
NAMES = tuple(base + sfx for base in ("nrtMultiHitQueryBatch_", "nrtMultiHitQueryBatchDevice_") for sfx in ("f32", "f64"))
FIELDS = ("struct_size", "flags", "rays", "num_rays", "options", "skip_prim_ids", "times", "ray_masks", "hits_out", "counts_out", "max_hits", "reserved")


# ---- 1. the expectation against the two it composes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_expectation_with_nothing_on_is_the_multihit_model(oracle, real):
    w = mq.world(oracle, "shells", real)
    for K in (2, 4):
        eh, ec = mq.expect(oracle, "shells", real, K, motion=False, masked=False, ids=False)
        mh, mc = mhf.model(w.nodes, w.idx, w.v, w.f, w.rays, K)
        assert mhf.hits_bytes(eh) == mhf.hits_bytes(mh) and np.array_equal(ec, mc)
        assert mc.sum() > 1000


@pytest.mark.parametrize("name", ["shells", "pile"])
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_k1_equals_the_combined_query_but_for_ties(oracle, real, name):
    """count and t equal query_fixture.expected's flag and t on every ray; where prim_id differs, the K = 64 row of that ray holds both
    primitives at exactly that t and multi-hit names the smaller."""
    w = mq.world(oracle, name, real)
    h1, c1 = mq.expect(oracle, name, real, 1)
    ch, cm = w.expected(oracle)
    h64, c64 = mq.expect(oracle, name, real, 64)

    def ties_ok(idx, mh, closest):
        for j, i in enumerate(idx):
            row = h64[i, :c64[i]]
            at_t = row["prim_id"][row["t"] == mh["t"][j]]
            assert mh["prim_id"][j] in at_t and closest["prim_id"][j] in at_t, (i, mh[j], closest[j])
            assert mh["prim_id"][j] < closest["prim_id"][j] and mh["prim_id"][j] == at_t.min()

    mhf.check_k1_against_closest(h1, c1, ch, cm, ties_ok)
    assert cm.sum() > 100


# ---- 2. include/nanort.h --------------------------------------------------------------------------------------------------------------
def cxx(args):
    r = subprocess.run(["g++"] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "g++ %s failed:\n%s" % (" ".join(args), r.stdout[-3000:])


def test_check_program_compiles_with_the_backend(tmp_path):
    """... the program tests/test_gpu_multihit_query.py runs against the GPU."""
    cxx(["-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-DNANORT_USE_HIP_BACKEND", "-D__HIP_PLATFORM_AMD__", "-I", INC, "-c", SRC, "-o",
         str(tmp_path / "multihit_query_check.o")])


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("multihit_query_check") / "multihit_query_check")
    cxx(["-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", exe])
    return exe


def write_world(w, directory):
    mesh, tree, rp = (os.path.join(directory, x) for x in ("mesh.bin", "tree.bin", "rays.bin"))
    with open(mesh, "wb") as fp:
        fp.write(np.array([w.v.shape[0], w.f.shape[0]], dtype=np.uint32).tobytes() + w.v.tobytes() + w.v1.tobytes() + w.f.tobytes() + w.pm.tobytes())
    with open(tree, "wb") as fp:  # BVHAccel::Load's format
        fp.write(np.array([w.nodes.shape[0]], dtype=np.uint64).tobytes() + np.ascontiguousarray(w.nodes).tobytes()
                 + np.array([w.idx.shape[0]], dtype=np.uint64).tobytes() + np.ascontiguousarray(w.idx, dtype=np.uint32).tobytes())
    with open(rp, "wb") as fp:
        fp.write(np.array([w.rays.shape[0]], dtype=np.uint64).tobytes() + w.rays.tobytes() + w.times.tobytes() + w.words.tobytes() + w.ids.tobytes())
    return mesh, tree, rp


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_header_host_form_returns_the_expectation(oracle, host_check, tmp_path, real, K):
    w = mq.world(oracle, "shells", real)
    mesh, tree, rp = write_world(w, str(tmp_path))
    out = os.path.join(str(tmp_path), "out.bin")
    r = subprocess.run([host_check, "f32" if real == np.float32 else "f64", mesh, tree, rp, out, str(K), "14"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:])
    raw = open(out, "rb").read()
    n, H = w.rays.shape[0], hit_dtype(real)
    counts = np.frombuffer(raw, np.uint32, n, 0)
    rows = np.frombuffer(raw, H, n * K, 4 * n).reshape(n, K)
    mq.assert_rows_identical(*mq.expect(oracle, "shells", real, K), rows, counts)


# ---- 3. the ABI -----------------------------------------------------------------------------------------------------------------------
def test_library_header_and_binding_table_carry_the_four_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r" T (nrt\w+)", out))
    header = open(os.path.join(INC, "nanort_hip.h")).read()
    L = capi.lib()
    for name in NAMES:
        assert name in exported and name in capi.SYMBOLS and ("NRT_API nrt_status %s(" % name) in header, name
        assert len(getattr(L, name).argtypes) == (3 if "Device" in name else 2), name
    assert sorted(exported) == sorted(capi.SYMBOLS)


def test_descriptor_layout_agrees_between_ctypes_and_the_header(tmp_path):
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nanort_hip.h"', "int main(void) {"]
    for s in ("f32", "f64"):
        lines.append('  printf("%s %%zu", sizeof(nrt_multihit_query_%s));' % (s, s))
        lines += ['  printf(" %%zu", offsetof(nrt_multihit_query_%s, %s));' % (s, k) for k in FIELDS]
        lines.append('  printf("\\n");')
    lines.append('  printf("first %zu %zu\\n", offsetof(nrt_ray_query_f32, hits_out), offsetof(nrt_ray_query_f64, hits_out));')
    lines.append('  printf("max %u\\n", NRT_MAX_MULTIHIT);')
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src), "-o", str(exe)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    want = [ctypes.sizeof(capi.MultiHitQuery)] + [getattr(capi.MultiHitQuery, k).offset for k in FIELDS]
    assert [k for k, _ in capi.MultiHitQuery._fields_] == list(FIELDS)
    for line, s in zip(out, ("f32", "f64")):
        words = line.split()
        assert words[0] == s and [int(x) for x in words[1:]] == want, (line, want)
    assert want[0] == 80
    # the first 56 bytes lie as in nrt_ray_query_*
    assert out[2].split() == ["first", "56", "56"] and capi.MultiHitQuery.hits_out.offset == 56
    for k in FIELDS[:8]:
        assert getattr(capi.MultiHitQuery, k).offset == getattr(capi.RayQuery, k).offset, k
    # the K-buffer's bound
    assert out[3].split() == ["max", str(capi.NRT_MAX_MULTIHIT)] and capi.NRT_MAX_MULTIHIT == 64
    header = open(os.path.join(INC, "nanort_hip.h")).read()
    assert "static_assert(sizeof(nrt_multihit_query_f32) == 80 && sizeof(nrt_multihit_query_f64) == 80" in header


def test_null_context_and_descriptor_are_refused_without_a_device():
    L = capi.lib()
    q = capi.MultiHitQuery(ctypes.sizeof(capi.MultiHitQuery), 0, 16, 1, None, None, None, None, 16, None, 4, 0)
    for s in ("f32", "f64"):
        assert getattr(L, "nrtMultiHitQueryBatch_" + s)(None, ctypes.addressof(q)) == capi.NRT_ERR_INVALID
        assert getattr(L, "nrtMultiHitQueryBatchDevice_" + s)(None, ctypes.addressof(q), None) == capi.NRT_ERR_INVALID
        assert getattr(L, "nrtMultiHitQueryBatch_" + s)(None, None) == capi.NRT_ERR_INVALID


def test_the_staged_rows_cap_is_named_in_the_source():
    assert mq.staged_rows_cap() == 256 << 20


# ---- 4. the fixture conditions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_fixture_condition_shells(oracle, real):
    """Evaluated on the model, f32 and f64 alike.  Rows that differ from the row without ids, without masks and at time 0 all at once:
    17.3 % at K = 1, 22.4 % at K = 2, 25.0 % at K = 4 (a tenth is asked for).  At K = 2: 1223 empty, 835 partly filled and 2041 full
    rows (500 each asked for), and 1288 rays with more than 2 candidates, whose rows evict (1000 asked for).  At K = 4 only one row
    fills: that arm covers the miss fill, not the bound."""
    w = mq.world(oracle, "shells", real)
    n = w.rays.shape[0]
    assert w.f.shape[0] == 4096 and n == qf.SHELL_RAYS
    for K in (1, 2, 4):
        share = float(mq.all_three(oracle, "shells", real, K).mean())
        assert share >= qf.SHELL_MIN_ALL_THREE, (K, share)
    _, c2 = mq.expect(oracle, "shells", real, 2)
    empty, partly, full = int((c2 == 0).sum()), int(((c2 > 0) & (c2 < 2)).sum()), int((c2 == 2).sum())
    assert min(empty, partly, full) >= 500, (empty, partly, full)
    _, c4 = mq.expect(oracle, "shells", real, 4)
    assert int((c4 > 2).sum()) >= 1000, int((c4 > 2).sum())
    assert (c4 < 4).sum() > 1000  # the miss fill
    h, c = mq.expect(oracle, "shells", real, 4)
    held = np.arange(4)[None, :] < c[:, None]
    assert not (held & (h["prim_id"] == w.ids[:, None])).any()  # no row names the skipped primitive


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_fixture_condition_pile(oracle, real):
    """Evaluated on the model, f32 and f64 alike: all three matter on 322 (K = 1), 387 (K = 2), 463 (K = 4) and 581 (K = 64) rays (150
    asked for); 1318 rows are full at K = 4 and at K = 64 (1000 asked for); the tree is deeper than the walk's 32 LDS entries."""
    w = mq.world(oracle, "pile", real)
    assert w.stats["max_tree_depth"] > ow.PILE_MIN_STACK
    for K in (1, 2, 4, 64):
        rays = int(mq.all_three(oracle, "pile", real, K).sum())
        assert rays >= qf.PILE_MIN_ALL_THREE, (K, rays)
    for K in (4, 64):
        _, c = mq.expect(oracle, "pile", real, K)
        assert int((c == K).sum()) >= 1000, (K, int((c == K).sum()))

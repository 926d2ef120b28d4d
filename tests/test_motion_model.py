"""Motion blur without a GPU (include/nanort_hip.h, "motion blur"): the numpy restatement of the vertex rule
(tests/motion_fixture.py), the fixture condition that makes the GPU tests able to see a wrong time, the twelve new symbols and their
refusals that never reach HIP, and include/nanort.h's host classes — Build() over MotionTriangleMesh and the per-ray Traverse()
with SetTime() — against the oracle on the header's own tree with numpy-interpolated vertices."""
import os
import subprocess

import numpy as np
import pytest

import motion_fixture as mf
import refit_model
from helpers import assert_hits_identical, trace_options
from nanort_amd import capi, scenes
from nanort_amd.wire import hit_dtype, node_dtype, ray_dtype, widen_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REALS = [np.float32, np.float64]
NAMES = tuple(base + sfx for base in ("nrtSetMeshMotion_", "nrtSetMeshMotionDevice_", "nrtTraverseBatchMotion_", "nrtTraverseBatchMotionDevice_",
                                      "nrtOccludedBatchMotion_", "nrtOccludedBatchMotionDevice_") for sfx in ("f32", "f64"))


@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_lerp_reaches_the_keyframes_and_stays_between_them(c1_mesh, real):
    v0 = np.ascontiguousarray(c1_mesh[0].astype(real))
    bits = np.uint32 if real == np.float32 else np.uint64
    for name, v1 in mf.deformations(v0).items():
        assert np.array_equal(mf.lerp(v0, v1, 0.0).view(bits), v0.view(bits)), name
        assert np.array_equal(mf.lerp(v0, v1, 1.0).view(bits), v1.view(bits)), name
        lo, hi = np.minimum(v0, v1), np.maximum(v0, v1)
        for s in mf.clamp_times(mf.TIME_VALUES, real):
            x = mf.lerp(v0, v1, s)
            assert ((x >= lo) & (x <= hi)).all(), (name, s)
    # the clamp of the time: NaN, negatives and -0.0 to 0, above 1 to 1, everything else itself
    s = mf.clamp_times(mf.TIME_VALUES, real)
    want = np.array([0, 1, 0.5, 0.25, real(1.0 / 3.0), np.nextafter(np.float32(1), np.float32(0)), 0, 0, 1, 0], dtype=real)
    assert np.array_equal(s.view(bits), want.view(bits))


def test_assigned_times_differ_between_neighbours():
    t = mf.assign_times(4099, np.float32)
    b = t.view(np.uint32)
    assert (b[1:] != b[:-1]).all()
    assert len(np.unique(b)) == len(mf.TIME_VALUES)


@pytest.mark.parametrize("name", ["wave", "translate"])
def test_fixture_condition_the_time_matters(oracle, c1_mesh, name):
    """At time 0.5 at least a tenth of the camera rays see a record that is neither keyframe 0's nor keyframe 1's: a walk that
    ignored the time, or took a neighbour's, fails the GPU tests."""
    v0, f = c1_mesh
    v1 = mf.deformations(v0)[name]
    nodes, idx, _ = oracle.build(v0, f)
    nodes = mf.motion_boxes(refit_model.refit, nodes, idx, v0, v1, f)
    share = mf.time_matters_share(oracle, nodes, idx, v0, v1, f, scenes.camera_rays(96, 64))
    assert share >= 0.10, share


@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_fixture_conditions_of_the_own_walk_tests(oracle, real):
    """What tests/test_gpu_own_walks.py rests on, from the reference alone (measured, f32 and f64 alike): over the soup with its
    jittered keyframe 1125 of the 6000 hostile rays hit at their times (100 asked for) and 681 records differ from the keyframe-0
    record (50 asked for); the pile's tree with union boxes is still deeper than the motion walk's 32 LDS entries (max stack 137)."""
    import own_walks_fixture as ow

    v0, v1, f, rays, times = ow.soup_motion(real)
    nodes, idx, _ = ow.motion_tree(oracle, v0, v1, f)
    _, _, hits, differ = ow.motion_figures(oracle, nodes, idx, v0, v1, f, rays, times)
    assert hits >= ow.SOUP_MOTION_MIN_HITS and differ >= ow.SOUP_MOTION_MIN_DIFFER, (hits, differ)
    v, f, rays, _ = ow.pile(real)
    nodes, idx, st = ow.motion_tree(oracle, v, ow.pile_keyframe1(v), f)
    _, _, cnt = oracle.traverse(nodes, idx, v, f, rays, count=True)
    assert st["max_tree_depth"] > ow.PILE_MIN_STACK and cnt[3] > ow.PILE_MIN_STACK


def test_binding_table_header_and_library_carry_the_twelve_symbols():
    header = open(os.path.join(ROOT, "include", "nanort_hip.h")).read()
    assert len(NAMES) == 12
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name) and ("NRT_API nrt_status %s(" % name) in header, name


def test_null_context_is_refused_without_a_device():
    L = capi.lib()
    for s in ("f32", "f64"):
        assert getattr(L, "nrtSetMeshMotion_" + s)(None, 16, 12) == capi.NRT_ERR_INVALID
        assert getattr(L, "nrtSetMeshMotion_" + s)(None, None, 0) == capi.NRT_ERR_INVALID
        assert getattr(L, "nrtSetMeshMotionDevice_" + s)(None, 16, 1, 12, None) == capi.NRT_ERR_INVALID
        assert getattr(L, "nrtTraverseBatchMotion_" + s)(None, 16, 16, 1, None, 16, None) == capi.NRT_ERR_INVALID
        assert getattr(L, "nrtTraverseBatchMotionDevice_" + s)(None, 16, 16, 1, None, 16, None, None) == capi.NRT_ERR_INVALID
        assert getattr(L, "nrtOccludedBatchMotion_" + s)(None, 16, 16, 1, None, 16) == capi.NRT_ERR_INVALID
        assert getattr(L, "nrtOccludedBatchMotionDevice_" + s)(None, 16, 16, 1, None, 16, None) == capi.NRT_ERR_INVALID


# ---- include/nanort.h, host classes ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("motion_host_check") / "motion_host_check")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "motion_host_check.cc"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


def run_host_check(exe, tmp, real, v0, v1, f, rays, times, opts):
    sfx = "f32" if real == np.float32 else "f64"
    mesh, rp, out = (os.path.join(str(tmp), x) for x in ("mesh.bin", "rays.bin", "out.bin"))
    with open(mesh, "wb") as fp:
        fp.write(np.array([v0.shape[0], f.shape[0]], dtype=np.uint32).tobytes() + np.ascontiguousarray(v0, real).tobytes()
                 + np.ascontiguousarray(v1, real).tobytes() + np.ascontiguousarray(f, np.uint32).tobytes())
    with open(rp, "wb") as fp:
        fp.write(np.array([rays.shape[0]], dtype=np.uint64).tobytes() + np.ascontiguousarray(rays, ray_dtype(real)).tobytes()
                 + np.ascontiguousarray(times, real).tobytes())
    o = opts[()] if opts.shape == () else opts[0]
    r = subprocess.run([exe, sfx, mesh, rp, out, str(int(o["prim_ids_range"][0])), str(int(o["prim_ids_range"][1])), str(int(o["skip_prim_id"])),
                        str(int(o["cull_back_face"]))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    raw = open(out, "rb").read()
    nn, ni = (int(x) for x in np.frombuffer(raw, np.uint64, 2))
    N, H = node_dtype(real), hit_dtype(real)
    off = 16
    nodes = np.frombuffer(raw, N, nn, off)
    off += nn * N.itemsize
    idx = np.frombuffer(raw, np.uint32, ni, off)
    off += ni * 4
    hits = np.frombuffer(raw, H, rays.shape[0], off)
    off += rays.shape[0] * H.itemsize
    return nodes, idx, hits, np.frombuffer(raw, np.uint8, rays.shape[0], off)


@pytest.fixture(scope="module")
def world(c1_mesh):
    v, f = c1_mesh
    cam = scenes.camera_rays(48, 32)
    return v, f, cam


OPTIONS = {
    "default": dict(),
    "range": dict(range_=(100, 700)),
    "skip": dict(skip=412),
    "cull": dict(cull=True),
    "all": dict(range_=(50, 900), skip=412, cull=True),
}


@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_header_host_classes_equal_the_oracle_on_the_headers_tree(oracle, host_check, tmp_path, world, real, opt):
    v, f, cam = world
    v0 = np.ascontiguousarray(v.astype(real))
    v1 = mf.deformations(v0)["wave"]
    rays = widen_rays(cam) if real == np.float64 else cam
    times = mf.assign_times(rays.shape[0], real)
    assert len(np.unique(mf.clamp_times(times, real))) >= 6  # (the ten times fold to seven shutter times)
    o = trace_options(**OPTIONS[opt])
    nodes, idx, h, m = run_host_check(host_check, tmp_path, real, v0, v1, f, rays, times, o)
    # the header's boxes hold both keyframes: the union of the per-keyframe boxes of the numpy refit model
    refit_model.assert_boxes_equal(nodes, mf.motion_boxes(refit_model.refit, nodes, idx, v0, v1, f))
    eh, em = mf.expected(oracle, nodes, idx, v0, v1, f, rays, times, o)
    assert em.sum() > (100 if opt in ("default", "skip") else 0)  # (culling leaves little of a box seen from inside)
    assert_hits_identical(eh, em, h, m)

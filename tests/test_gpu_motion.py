"""Motion blur on the GPU (nanort_amd/csrc/own_walks.hip; include/nanort_hip.h, "motion blur"): a second vertex
keyframe per triangle context and one time per ray.

Parity is exact.  For the rays that share one clamped time s the expected records are oracle.traverse — the project's pinned
restatement of the reference — over the CONTEXT'S OWN node array and the vertices interpolated to s in numpy by the rule of
include/nanort_motion.h (tests/motion_fixture.py: numpy rounds every operation on its own, as the device does); the motion walk is
the literal binary loop, so every byte of every record and mask must match (assert_hits_identical, no tolerance).  Neighbouring
rays carry different times (motion_fixture.assign_times) and tests/test_motion_model.py asserts that the time changes the records of
the wave and translate deformations: a walk that dropped, truncated or mis-indexed the time fails here."""
import os
import subprocess

import numpy as np
import pytest

import motion_fixture as mf
import refit_model
import size_thresholds as sz
from bvh_check import validate_bvh
from helpers import assert_hits_identical, trace_options
from multihit_fixture import hits_bytes, model as multihit_model
from nanort_amd import BVHAccel, CurveGeometry, CylinderGeometry, MotionTriangleMesh, SphereGeometry, TriangleMesh, scenes
from nanort_amd.capi import NRT_ERR_INVALID, NRT_ERR_PRECISION, NrtError
from nanort_amd.wire import default_build_options, hit_dtype, ray_dtype, widen_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REALS = [np.float32, np.float64]
DEFORMATIONS = ["jitter", "translate", "wave", "collapse", "same"]


def _sfx(real):
    return "f32" if np.dtype(real) == np.float32 else "f64"


def odd_count(rays):
    """The same rays, trimmed so that their count is no multiple of 64 (the last wave of the launch is a partial one)."""
    n = rays.shape[0]
    n -= 37 if n % 64 == 0 else 0
    assert n % 64 != 0 and n > 128  # (above one claim chunk: lanes are refilled)
    return np.ascontiguousarray(rays[:n])


def window_rays(rays, seed):
    """The same rays with random [min_t, max_t] windows around the mesh (the camera is 15 to 25 away from it): some windows end
    in front of the hit, some begin behind it, some hold it."""
    rng = np.random.default_rng(seed)
    r = rays.copy()
    a = rng.uniform(0, 22, size=r.shape[0])
    r["min_t"], r["max_t"] = a, a + rng.uniform(0, 12, size=r.shape[0])
    return r


class World:
    """One precision: C1's mesh, its keyframe-1 deformations, and three ray sets with their per-ray times (computed once)."""

    def __init__(self, real, c1_mesh):
        self.real = real
        v, f = c1_mesh
        self.v0 = np.ascontiguousarray(v.astype(real))
        self.f = f
        self.v1 = mf.deformations(self.v0)
        cam = scenes.camera_rays(96, 64)
        a32 = BVHAccel(np.float32)
        a32.Build(f.shape[0], TriangleMesh(v.astype(np.float32), f))
        h32, m32 = a32.TraverseBatch(cam)
        bounce = scenes.secondary_rays("bounce", v.astype(np.float32), f, cam, h32, m32)
        a32.close()
        if real == np.float64:
            cam, bounce = widen_rays(cam), widen_rays(bounce)
        self.sets = [odd_count(cam), odd_count(bounce), odd_count(window_rays(cam, 3))]
        self.times = [mf.assign_times(r.shape[0], real, seed=3 + k) for k, r in enumerate(self.sets)]

    def built(self, name, bo=None, n_faces=None):
        f = self.f if n_faces is None else self.f[:n_faces]
        a = BVHAccel(self.real)
        assert a.Build(f.shape[0], MotionTriangleMesh(self.v0, self.v1[name], f), bo)
        return a, f


@pytest.fixture(scope="module", params=REALS, ids=["f32", "f64"])
def w(request, c1_mesh):
    return World(request.param, c1_mesh)


@pytest.fixture(scope="module")
def w32(c1_mesh):
    return World(np.float32, c1_mesh)


def check_queries(oracle, a, w, v1, f, opts=None, sets=None, occlusion=True):
    nodes, idx = a.GetTree()
    for k in (range(len(w.sets)) if sets is None else sets):
        rays, times = w.sets[k], w.times[k]
        eh, em = mf.expected(oracle, nodes, idx, w.v0, v1, f, rays, times, opts)
        assert opts is not None or em.sum() > 100  # (not vacuous)
        h, m = a.TraverseBatchMotion(rays, times, opts)
        assert a.LastKernelName() == "nrt::k_traverse_motion<%s>" % ("float" if w.real == np.float32 else "double")
        assert_hits_identical(eh, em, h, m)
        if occlusion:
            assert np.array_equal(a.OccludedBatchMotion(rays, times, opts), em)
    return nodes, idx


# ---- 1. trees ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_faces", [None, 1, 2, 5, 513])
def test_trees_hold_both_keyframes_and_are_deterministic(w, n_faces):
    a, f = w.built("wave", n_faces=n_faces)
    nodes, idx = a.GetTree()
    v1 = w.v1["wave"]
    for v in (w.v0, v1):  # a valid tree whose boxes contain each keyframe
        validate_bvh(nodes, idx, v, f, exact_bounds=False)
    refit_model.assert_boxes_equal(nodes, mf.motion_boxes(refit_model.refit, nodes, idx, w.v0, v1, f))
    b, _ = w.built("wave", n_faces=n_faces)
    n2, i2 = b.GetTree()
    assert n2.tobytes() == nodes.tobytes() and i2.tobytes() == idx.tobytes(), "two motion builds differ"
    b.close()
    # keyframe 1 == keyframe 0: the bytes of a plain build
    p = BVHAccel(w.real)
    assert p.Build(f.shape[0], TriangleMesh(w.v0, f))
    pn, pi = p.GetTree()
    s, _ = w.built("same", n_faces=n_faces)
    sn, si = s.GetTree()
    assert sn.tobytes() == pn.tobytes() and si.tobytes() == pi.tobytes(), "keyframe 1 == keyframe 0 does not build the plain tree"
    s.close()
    p.close()
    # ... and a plain build after the keyframe was removed gives the plain bytes again
    a.SetMeshMotion(None)
    assert not a.IsValid(), "nrtSetMeshMotion(NULL) keeps the tree"
    assert a.BuildCurrent()
    rn, ri = a.GetTree()
    assert rn.tobytes() == pn.tobytes() and ri.tobytes() == pi.tobytes(), "a build after nrtSetMeshMotion(NULL) is not the plain build"
    a.close()


# ---- 2 + 3. records and occlusion flags ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DEFORMATIONS)
def test_records_and_flags_for_every_deformation(oracle, w, name):
    a, f = w.built(name)
    check_queries(oracle, a, w, w.v1[name], f)
    a.close()


@pytest.mark.parametrize("min_leaf", [1, 16])
def test_records_for_leaf_sizes(oracle, w, min_leaf):
    bo = default_build_options(w.real)
    bo["min_leaf_primitives"] = min_leaf
    a, f = w.built("wave", bo)
    nodes, _ = check_queries(oracle, a, w, w.v1["wave"], f, sets=(0, 2))
    assert nodes["data"][nodes["flag"] == 1, 0].max() <= min_leaf
    a.close()


OPTIONS = {
    "range": dict(range_=(100, 700)),
    "skip": dict(skip=412),
    "cull": dict(cull=True),
    "all": dict(range_=(50, 900), skip=412, cull=True),
}


@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_records_and_flags_under_trace_options(oracle, w, opt):
    a, f = w.built("wave")
    check_queries(oracle, a, w, w.v1["wave"], f, opts=trace_options(**OPTIONS[opt]), sets=(0, 1))
    a.close()


@pytest.mark.parametrize("n_faces", [1, 2, 5])
def test_records_where_the_root_is_a_leaf(oracle, w, n_faces):
    bo = default_build_options(w.real)
    bo["min_leaf_primitives"] = 16  # (five triangles in one leaf too)
    a, f = w.built("translate", bo, n_faces=n_faces)
    nodes, _ = a.GetTree()
    assert nodes.shape[0] == 1 and nodes["flag"][0] == 1
    # rays aimed at the moving triangles: from the camera towards points of both keyframes
    rng = np.random.default_rng(5)
    n = 333
    tri = w.v0[f[rng.integers(0, f.shape[0], size=n)]].mean(axis=1) + rng.uniform(0, 11, size=(n, 1)) * np.array([0, 0, 1.0])
    rays = np.zeros(n, dtype=ray_dtype(w.real))
    rays["org"] = (0.0, 5.0, 20.0)
    d = tri - np.array([0.0, 5.0, 20.0])
    rays["dir"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays["max_t"] = 1e30
    times = mf.assign_times(n, w.real, seed=9)
    eh, em = mf.expected(oracle, *a.GetTree(), w.v0, w.v1["translate"], f, rays, times)
    h, m = a.TraverseBatchMotion(rays, times)
    assert_hits_identical(eh, em, h, m)
    assert np.array_equal(a.OccludedBatchMotion(rays, times), em)
    assert 0 < em.sum()
    a.close()


def test_null_times_is_time_zero(oracle, w):
    a, f = w.built("wave")
    nodes, idx = a.GetTree()
    rays = w.sets[0]
    oh, om = oracle.traverse(nodes, idx, w.v0, f, rays)
    h, m = a.TraverseBatchMotion(rays, None)
    assert_hits_identical(oh, om, h, m)
    assert np.array_equal(a.OccludedBatchMotion(rays, None), om)
    a.close()


# ---- 4. spill path ---------------------------------------------------------------------------------------------------------------
def test_deep_adopted_tree_takes_the_overflow_stack(oracle):
    v0, f = scenes.plane(300, 150)
    v1 = v0.astype(np.float64).copy()
    v1[:, 1] += 0.3 * np.sin(3.0 * v1[:, 0]) * np.cos(2.0 * v1[:, 2])
    v1 = np.ascontiguousarray(v1.astype(np.float32))
    nodes, idx, st = oracle.build(v0, f)
    assert st["max_tree_depth"] > 40
    nodes = mf.motion_boxes(refit_model.refit, nodes, idx, v0, v1, f)
    a = BVHAccel(np.float32)
    a.SetMesh(MotionTriangleMesh(v0, v1, f))
    a.SetTree(nodes, idx)
    rays = scenes.camera_rays(320, 180)
    _, _, cnt = oracle.traverse(nodes, idx, v0, f, rays, count=True)
    assert cnt[3] > 33, "fixture no longer exercises the spill path"
    times = mf.assign_times(rays.shape[0], np.float32)
    eh, em = mf.expected(oracle, nodes, idx, v0, v1, f, rays, times)
    h, m = a.TraverseBatchMotion(rays, times)
    assert_hits_identical(eh, em, h, m)
    assert np.array_equal(a.OccludedBatchMotion(rays, times), em)
    a.close()


# ---- 5. device forms -------------------------------------------------------------------------------------------------------------
def test_device_forms_on_a_side_stream(oracle, w):
    import torch

    real, f = w.real, w.f
    tdt = torch.float32 if real == np.float32 else torch.float64
    v1 = w.v1["wave"]
    side = torch.cuda.Stream()
    a = BVHAccel(real)
    a.SetMesh(TriangleMesh(w.v0, f))
    # strided rows: keyframe 1 in the first three of five columns
    wide = np.full((v1.shape[0] + 7, 5), 1e9, dtype=real)
    wide[: v1.shape[0], :3] = v1
    d_wide = torch.from_numpy(wide).cuda()
    torch.cuda.synchronize()
    # a block with too few rows is refused before anything is enqueued, and the context still answers as before
    assert a.BuildCurrent()
    nodes0, idx0 = a.GetTree()
    nv = int(f.max()) + 1
    with pytest.raises(NrtError) as e:
        a.SetMeshMotionDevice(d_wide[: nv - 1], stream=side)
    assert e.value.status == NRT_ERR_INVALID and str(e.value)
    n1, i1 = a.GetTree()
    assert n1.tobytes() == nodes0.tobytes() and i1.tobytes() == idx0.tobytes()
    oh, om = oracle.traverse(nodes0, idx0, w.v0, f, w.sets[0])
    assert_hits_identical(oh, om, *a.TraverseBatch(w.sets[0]))
    a.SetMeshMotionDevice(d_wide, stream=side)
    assert not a.IsValid()
    assert a.BuildCurrent()
    nodes, idx = a.GetTree()
    ref, _ = w.built("wave")
    rn, ri = ref.GetTree()
    assert nodes.tobytes() == rn.tobytes() and idx.tobytes() == ri.tobytes(), "Device keyframe builds another tree than the host keyframe"
    ref.close()
    rays, times = w.sets[1], w.times[1]
    n = rays.shape[0]
    eh, em = mf.expected(oracle, nodes, idx, w.v0, v1, f, rays, times)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    # the times: a view one element into a larger tensor (fp32: an odd 4-byte offset)
    big = torch.full((n + 5,), 0.75, dtype=tdt, device="cuda")
    big[1:1 + n] = torch.from_numpy(times).cuda()
    d_times = big[1:1 + n]
    assert d_times.data_ptr() == big.data_ptr() + times.itemsize
    d_hits = torch.zeros((n * eh.dtype.itemsize,), dtype=torch.uint8, device="cuda")
    d_mask = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    d_occ = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a.TraverseBatchMotionDevice(d_rays, d_times, d_hits, d_mask, stream=side)
    a.OccludedBatchMotionDevice(d_rays, d_times, d_occ, stream=side)
    # nrtBuild right behind the Device launches waits for them (it rewrites the arrays they read)
    assert a.BuildCurrent()
    side.synchronize()
    h = np.frombuffer(d_hits.cpu().numpy().tobytes(), dtype=eh.dtype)
    assert_hits_identical(eh, em, h, d_mask.cpu().numpy())
    assert np.array_equal(d_occ.cpu().numpy(), em)
    n2, i2 = a.GetTree()
    assert n2.tobytes() == nodes.tobytes() and i2.tobytes() == idx.tobytes()
    a.close()


# ---- 6. pieced host loop ---------------------------------------------------------------------------------------------------------
def test_host_call_in_pieces_advances_the_times(oracle, w32):
    w = w32
    assert sz.source_cap("kPiece") == sz.PIECE
    a, f = w.built("wave")
    nodes, idx = a.GetTree()
    base = sz.cut(np.concatenate([w.sets[0], w.sets[1]]))
    bt = mf.assign_times(sz.B, np.float32, seed=21)
    eh, em = mf.expected(oracle, nodes, idx, w.v0, w.v1["wave"], f, base, bt)
    n = sz.PIECE + sz.B
    assert sz.crossing_trips(n, sz.PIECE) == 2 and sz.PIECE % sz.B != 0  # (the second piece starts at another base ray and time)
    rays, times = sz.tiled(base, n), sz.tiled(bt, n)
    h, m = a.TraverseBatchMotion(rays, times)
    assert_hits_identical(sz.tiled(eh, n), sz.tiled(em, n), h, m)
    assert np.array_equal(a.OccludedBatchMotion(rays, times), sz.tiled(em, n))
    a.close()


# ---- 7. existing entry points on a motion context ---------------------------------------------------------------------------------
def test_existing_entry_points_answer_for_keyframe_0(oracle, w):
    a, f = w.built("wave")
    nodes, idx = a.GetTree()
    cam, bounce = w.sets[0], w.sets[1]
    ch, cm = oracle.traverse(nodes, idx, w.v0, f, cam)
    bh, bm = oracle.traverse(nodes, idx, w.v0, f, bounce)
    assert_hits_identical(ch, cm, *a.TraverseBatch(cam))
    assert np.array_equal(a.OccludedBatch(bounce), bm)
    (h0, m0), (_, m1) = a.TraverseBatches([cam, (bounce, "occlusion")])
    assert_hits_identical(ch, cm, h0, m0)
    assert np.array_equal(m1, bm)
    h, c = a.MultiHitTraverseBatch(cam, 4)
    mh, mc = multihit_model(nodes, idx, w.v0, f, cam, 4)
    assert np.array_equal(c, mc) and hits_bytes(h) == hits_bytes(mh)
    a.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def refused(call, status):
    with pytest.raises(NrtError) as e:
        call()
    assert e.value.status == status, e.value
    assert str(e.value).split(": ", 1)[1].strip(), "empty nrtLastError"


def test_refusals_leave_the_context_as_it_was(oracle, w):
    real, f = w.real, w.f
    other = np.float64 if real == np.float32 else np.float32
    rays, times = w.sets[0][:777], w.times[0][:777]
    # no keyframe: motion queries are refused, the plain queries still answer
    a = BVHAccel(real)
    assert a.Build(f.shape[0], TriangleMesh(w.v0, f))
    nodes, idx = a.GetTree()
    oh, om = oracle.traverse(nodes, idx, w.v0, f, rays)
    refused(lambda: a.TraverseBatchMotion(rays, times), NRT_ERR_INVALID)
    refused(lambda: a.OccludedBatchMotion(rays, times), NRT_ERR_INVALID)
    assert_hits_identical(oh, om, *a.TraverseBatch(rays))
    # a keyframe of the other precision
    L = a._L
    v1o = np.ascontiguousarray(w.v1["wave"].astype(other))
    st = getattr(L, "nrtSetMeshMotion_" + _sfx(other))(a._h, v1o.ctypes.data, 3 * v1o.itemsize)
    assert st == NRT_ERR_PRECISION and L.nrtLastError(a._h)
    assert a.IsValid()
    a.close()
    # with a keyframe: refits are refused, queries of the other precision too; the motion query answers as before
    a, _ = w.built("wave")
    nodes, idx = a.GetTree()
    eh, em = mf.expected(oracle, nodes, idx, w.v0, w.v1["wave"], f, rays, times)
    refused(lambda: a.Refit(w.v1["jitter"]), NRT_ERR_INVALID)
    import torch

    d_v = torch.from_numpy(w.v1["jitter"]).cuda()
    refused(lambda: a.RefitDevice(d_v), NRT_ERR_INVALID)
    ro = np.zeros(4, dtype=ray_dtype(other))
    ho = np.zeros(4, dtype=hit_dtype(other))
    to = np.zeros(4, dtype=other)
    st = getattr(L, "nrtTraverseBatchMotion_" + _sfx(other))(a._h, ro.ctypes.data, to.ctypes.data, 4, None, ho.ctypes.data, None)
    assert st == NRT_ERR_PRECISION and L.nrtLastError(a._h)
    n2, i2 = a.GetTree()
    assert n2.tobytes() == nodes.tobytes() and i2.tobytes() == idx.tobytes()
    assert_hits_identical(eh, em, *a.TraverseBatchMotion(rays, times))
    # any nrtSetMesh* removes the keyframe
    a.SetMesh(TriangleMesh(w.v0, f))
    assert a.BuildCurrent()
    refused(lambda: a.TraverseBatchMotion(rays, times), NRT_ERR_INVALID)
    a.close()


# ---- 9. include/nanort.h with the backend ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header_check(tmp_path_factory):
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "nanort_amd", "lib")
    exe = str(tmp_path_factory.mktemp("motion_check") / "motion_check")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", inc, os.path.join(ROOT, "tests", "cpp", "motion_check.cc"),
                        "-o", exe, "-DNANORT_USE_HIP_BACKEND", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include", "-L", libdir, "-lnanort_hip",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


@pytest.mark.parametrize("opt", ["default", "all"])
def test_header_backend_equals_its_own_host_walk(header_check, tmp_path, w, opt):
    """GPU Build() over MotionTriangleMesh; TraverseBatchMotion / OccludedBatchMotion against the header's per-ray Traverse() with
    SetTime() over the read-back tree, byte for byte, inside tests/cpp/motion_check.cc; Refit() refuses."""
    real = w.real
    rays, times = w.sets[0], w.times[0]
    mesh, rp = (os.path.join(str(tmp_path), x) for x in ("mesh.bin", "rays.bin"))
    with open(mesh, "wb") as fp:
        fp.write(np.array([w.v0.shape[0], w.f.shape[0]], dtype=np.uint32).tobytes() + w.v0.tobytes() + w.v1["wave"].tobytes()
                 + np.ascontiguousarray(w.f, np.uint32).tobytes())
    with open(rp, "wb") as fp:
        fp.write(np.array([rays.shape[0]], dtype=np.uint64).tobytes() + rays.tobytes() + times.tobytes())
    o = trace_options(**(OPTIONS["all"] if opt == "all" else {}))
    r = subprocess.run([header_check, _sfx(real), mesh, rp, str(int(o["prim_ids_range"][0])), str(int(o["prim_ids_range"][1])),
                        str(int(o["skip_prim_id"])), str(int(o["cull_back_face"]))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    word, hits, n = r.stdout.split()[-3:]
    assert word == "ok" and int(n) == rays.shape[0] and int(hits) > (500 if opt == "default" else 0)


def test_other_primitive_kinds_are_refused():
    rays = scenes.camera_rays(8, 8)
    times = np.zeros(rays.shape[0], dtype=np.float32)
    c, r = scenes.random_spheres(64)
    e, er = scenes.random_cylinders(64)
    cps, cr = scenes.synthetic_hair(64)
    for geom in (SphereGeometry(c, r), CylinderGeometry(e, er), CurveGeometry(cps, cr)):
        a = BVHAccel(np.float32)
        assert a.Build(geom.num_faces, geom)
        refused(lambda: a.TraverseBatchMotion(rays, times), NRT_ERR_INVALID)
        refused(lambda: a.OccludedBatchMotion(rays, times), NRT_ERR_INVALID)
        refused(lambda: a.SetMeshMotion(np.zeros((64, 3), dtype=np.float32)), NRT_ERR_INVALID)
        assert a.IsValid()
        assert a.OccludedBatch(rays).shape[0] == rays.shape[0]
        a.close()

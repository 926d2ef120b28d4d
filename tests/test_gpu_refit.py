"""BVH refit on the GPU (nanort_amd/csrc/refit.hip, include/nanort_hip.h nrtRefit* / nrtRefitDevice*): the refit tree keeps
every topology byte, its boxes equal the numpy model (tests/refit_model.py) on moved vertices, and every query on it equals
the oracle / the multi-hit model on the refit node array and the new vertices — bit for bit.  Also: refit with unchanged
vertices, a build after a refit, adopted trees, the Device form on side streams, refusals, and scenes over a refit mesh."""
import ctypes

import numpy as np
import pytest

from helpers import assert_hits_identical
from multihit_fixture import hits_bytes, model as multihit_model, random_window_rays
from nanort_amd import BVHAccel, Scene, TriangleMesh, scenes
from nanort_amd.capi import NRT_ERR_INVALID, NRT_ERR_PRECISION, NrtError
from nanort_amd.wire import widen_rays
from refit_model import assert_boxes_equal, refit as model_refit, topology_bytes

pytestmark = pytest.mark.gpu

REALS = [np.float32, np.float64]


def _sfx(real):
    return "f32" if np.dtype(real) == np.float32 else "f64"


def deformations(v):
    """name -> moved vertices: a small jitter, a rigid translation far outside the old bounds, a non-uniform scale, a wave,
    and some triangles collapsed to points."""
    rng = np.random.default_rng(11)
    real = v.dtype
    c = v.mean(axis=0)
    out = {}
    out["jitter"] = (v + rng.normal(scale=1e-3, size=v.shape)).astype(real)
    out["translate"] = (v + np.array([250.0, -130.0, 75.0])).astype(real)
    out["scale"] = ((v - c) * np.array([3.0, 0.25, -1.5]) + c).astype(real)
    w = v.astype(np.float64).copy()
    w[:, 1] += 0.2 * np.sin(3.0 * w[:, 0]) * np.cos(2.0 * w[:, 2])
    out["wave"] = w.astype(real)
    col = v.copy()
    k = rng.choice(v.shape[0], size=max(1, v.shape[0] // 5), replace=False)
    col[k] = c.astype(real)  # every triangle with all three corners in k collapses to a point
    out["collapse"] = col
    return out


@pytest.fixture(scope="module", params=REALS, ids=["f32", "f64"])
def c1(request, c1_mesh):
    real = request.param
    v, f = c1_mesh
    v = np.ascontiguousarray(v.astype(real))
    cam = scenes.camera_rays(96, 64)
    a32 = BVHAccel(np.float32)
    a32.Build(f.shape[0], TriangleMesh(v.astype(np.float32), f))
    h32, m32 = a32.TraverseBatch(cam)
    bounce = scenes.secondary_rays("bounce", v.astype(np.float32), f, cam, h32, m32)
    a32.close()
    if real == np.float64:
        cam, bounce = widen_rays(cam), widen_rays(bounce)
    rnd = random_window_rays(cam, 3)
    return real, v, f, cam, bounce, rnd


def built(real, v, f):
    a = BVHAccel(real)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    return a


def check_traces(oracle, a, nodes, idx, v1, f, rays_list):
    for rays in rays_list:
        oh, om = oracle.traverse(nodes, idx, v1, f, rays)
        h, m = a.TraverseBatch(rays)
        assert_hits_identical(oh, om, h, m)


@pytest.mark.parametrize("name", ["jitter", "translate", "scale", "wave", "collapse"])
def test_refit_boxes_topology_and_traces(oracle, c1, name):
    real, v, f, cam, bounce, rnd = c1
    a = built(real, v, f)
    n0, i0 = a.GetTree()
    v1 = deformations(v)[name]
    a.Refit(v1)
    n1, i1 = a.GetTree()
    assert topology_bytes(n1) == topology_bytes(n0), "refit changed flag / axis / data"
    assert i1.tobytes() == i0.tobytes(), "refit changed the index array"
    assert_boxes_equal(n1, model_refit(n0, i0, v1, f))
    # closest hit, occlusion, and the Batches entry on the refit tree == the oracle on the refit node array and v1
    check_traces(oracle, a, n1, i1, v1, f, (cam, bounce, rnd))
    oh, om = oracle.traverse(n1, i1, v1, f, bounce)
    assert np.array_equal(a.OccludedBatch(bounce), om)
    import torch

    d_rays = torch.from_numpy(cam.view(np.uint8).copy()).cuda()
    d_hits = torch.zeros((cam.shape[0] * oh.dtype.itemsize,), dtype=torch.uint8, device="cuda")
    d_mask = torch.zeros((cam.shape[0],), dtype=torch.uint8, device="cuda")
    a.TraverseBatchesDevice([(d_rays, d_hits, d_mask)])
    torch.cuda.synchronize()
    ch, cm = oracle.traverse(n1, i1, v1, f, cam)
    h = np.frombuffer(d_hits.cpu().numpy().tobytes(), dtype=ch.dtype)
    assert_hits_identical(ch, cm, h, d_mask.cpu().numpy())
    a.close()


@pytest.mark.parametrize("K", [1, 4, 16])
def test_refit_multihit_equals_the_model(c1, K):
    real, v, f, cam, bounce, rnd = c1
    a = built(real, v, f)
    v1 = deformations(v)["wave"]
    a.Refit(v1)
    n1, i1 = a.GetTree()
    for rays in (cam, rnd):
        h, c = a.MultiHitTraverseBatch(rays, K)
        mh, mc = multihit_model(n1, i1, v1, f, rays, K)
        assert np.array_equal(c, mc) and hits_bytes(h) == hits_bytes(mh), "K=%d" % K
    a.close()


def test_refit_with_unchanged_vertices_returns_the_built_tree(c1):
    real, v, f, cam, bounce, rnd = c1
    a = built(real, v, f)
    n0, i0 = a.GetTree()
    for _ in range(2):  # (the second call reuses the plan)
        a.Refit(v)
        n1, i1 = a.GetTree()
        assert topology_bytes(n1) == topology_bytes(n0) and i1.tobytes() == i0.tobytes()
        assert_boxes_equal(n1, n0)
    a.close()


def test_build_after_refit_equals_a_fresh_build(c1):
    """nrtBuild straight after a refit (no nrtSetMesh in between) builds over the refit positions."""
    real, v, f, cam, bounce, rnd = c1
    v1 = deformations(v)["scale"]
    a = built(real, v, f)
    a.Refit(v1)
    nn = ctypes.c_uint64(0)
    a._check(getattr(a._L, "nrtBuild_" + _sfx(real))(a._h, None, None, ctypes.byref(nn)))
    nb, ib = a.GetTree()
    b = built(real, v1, f)
    nf, if_ = b.GetTree()
    assert nb.tobytes() == nf.tobytes() and ib.tobytes() == if_.tobytes()
    a.close()
    b.close()


def test_refit_of_an_adopted_tree(oracle, c1):
    real, v, f, cam, bounce, rnd = c1
    on, oi, _ = oracle.build(v, f)
    a = BVHAccel(real)
    a.SetMesh(TriangleMesh(v, f))
    a.SetTree(on, oi)
    v1 = deformations(v)["translate"]
    a.Refit(v1)
    n1, i1 = a.GetTree()
    assert topology_bytes(n1) == topology_bytes(on) and i1.tobytes() == oi.tobytes()
    assert_boxes_equal(n1, model_refit(on, oi, v1, f))
    check_traces(oracle, a, n1, i1, v1, f, (cam, bounce))
    a.close()


def test_refit_of_an_adopted_tree_with_empty_and_unreachable_records(oracle):
    """Hand-made tree over a soup: an empty leaf, and unreachable records that keep their bytes."""
    from nanort_amd.wire import node_dtype

    real = np.float32
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, size=(60, 3)).astype(real)
    f = rng.integers(0, 60, size=(40, 3), dtype=np.uint32)
    on, oi, _ = oracle.build(v, f, min_leaf=4)
    nd = node_dtype(real)
    extra = np.zeros(3, nd)
    # root' -> (old root, empty leaf); two unreachable records behind them
    root = np.zeros(1, nd)
    nodes = np.concatenate([root, on, extra])
    n = on.shape[0]
    br = nodes["flag"][1:n + 1] == 0
    nodes["data"][1:n + 1][br] += 1  # shift the old tree's child ids by one
    nodes[0]["flag"], nodes[0]["axis"], nodes[0]["data"] = 0, 0, (1, n + 1)
    nodes[0]["bmin"], nodes[0]["bmax"] = on[0]["bmin"], on[0]["bmax"]
    nodes[n + 1]["flag"], nodes[n + 1]["data"] = 1, (0, 0)  # empty leaf
    big = np.finfo(real).max
    nodes[n + 1]["bmin"], nodes[n + 1]["bmax"] = (big,) * 3, (-big,) * 3
    nodes[n + 2]["flag"], nodes[n + 2]["data"] = 1, (3, 0)  # unreachable leaf
    nodes[n + 2]["bmin"], nodes[n + 2]["bmax"] = (9, 9, 9), (10, 10, 10)
    nodes[n + 3]["flag"], nodes[n + 3]["data"] = 0, (1, 2)  # unreachable branch
    nodes[n + 3]["bmin"], nodes[n + 3]["bmax"] = (-7, -7, -7), (7, 7, 7)
    a = BVHAccel(real)
    a.SetMesh(TriangleMesh(v, f))
    a.SetTree(nodes, oi)
    v1 = (v * np.array([2.0, 0.5, 1.0]) + 0.3).astype(real)
    a.Refit(v1)
    n1, i1 = a.GetTree()
    want = model_refit(nodes, oi, v1, f)
    assert topology_bytes(n1) == topology_bytes(nodes)
    assert_boxes_equal(n1, want)
    assert n1[n + 2].tobytes() == nodes[n + 2].tobytes() and n1[n + 3].tobytes() == nodes[n + 3].tobytes()
    rays = random_window_rays(scenes.camera_rays(32, 32), 1)
    rays["org"] = rng.uniform(-3, 3, size=(rays.shape[0], 3))
    check_traces(oracle, a, n1, i1, v1, f, (rays,))
    a.close()


@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_refit_device_on_side_streams_ten_frames(oracle, c1_mesh, real):
    """RefitDevice from a strided [nv, 4] tensor on a side stream, no host sync, then TraverseBatchDevice on a different stream
    and a host TraverseBatch: both see the refit tree, frame after frame."""
    import torch

    v, f = c1_mesh
    v = np.ascontiguousarray(v.astype(real))
    a = built(real, v, f)
    n0, i0 = a.GetTree()
    rays = scenes.camera_rays(64, 48)
    if real == np.float64:
        rays = widen_rays(rays)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    hsz = 16 if real == np.float32 else 32
    s_refit, s_trace = torch.cuda.Stream(), torch.cuda.Stream()
    tdt = torch.float32 if real == np.float32 else torch.float64
    d_v = torch.empty((v.shape[0], 4), dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    for frame in range(10):
        w = v.astype(np.float64).copy()
        w[:, 1] += 0.1 * np.sin(2.0 * w[:, 0] + 0.7 * frame)
        w[:, 0] += 0.05 * frame
        v1 = w.astype(real)
        with torch.cuda.stream(s_refit):
            host4 = np.concatenate([v1, np.full((v.shape[0], 1), -1e30)], axis=1).astype(real)
            d_v.copy_(torch.from_numpy(host4), non_blocking=False)
            a.RefitDevice(d_v, stream=s_refit)
        d_hits = torch.zeros((rays.shape[0] * hsz,), dtype=torch.uint8, device="cuda")
        d_mask = torch.zeros((rays.shape[0],), dtype=torch.uint8, device="cuda")
        a.TraverseBatchDevice(d_rays, d_hits, d_mask, stream=s_trace.cuda_stream)
        hh, hm = a.TraverseBatch(rays)
        s_trace.synchronize()
        want_nodes = model_refit(n0, i0, v1, f)
        n1, i1 = a.GetTree()
        assert_boxes_equal(n1, want_nodes)
        oh, om = oracle.traverse(n1, i1, v1, f, rays)
        assert_hits_identical(oh, om, hh, hm)
        dh = np.frombuffer(d_hits.cpu().numpy().tobytes(), dtype=oh.dtype)
        assert_hits_identical(oh, om, dh, d_mask.cpu().numpy())
        s_refit.synchronize()  # (the next frame rewrites d_v)
    a.close()


def test_refusals_write_nothing(oracle, c1):
    real, v, f, cam, bounce, rnd = c1
    other = np.float64 if real == np.float32 else np.float32
    s = _sfx(real)
    a = BVHAccel(real)
    L = a._L
    a.SetMesh(TriangleMesh(v, f))
    with pytest.raises(NrtError) as e:  # no tree
        a.Refit(v)
    assert e.value.status == NRT_ERR_INVALID and "no tree" in str(e.value)
    a.Build(f.shape[0], TriangleMesh(v, f))
    n0, i0 = a.GetTree()
    h0, m0 = a.TraverseBatch(cam)
    v1 = deformations(v)["scale"]
    assert getattr(L, "nrtRefit_" + s)(None, v1.ctypes.data, 12) == NRT_ERR_INVALID
    assert getattr(L, "nrtRefit_" + s)(a._h, None, v.itemsize * 3) == NRT_ERR_INVALID
    assert getattr(L, "nrtRefit_" + s)(a._h, v1.ctypes.data, v.itemsize * 3 - 1) == NRT_ERR_INVALID
    assert "stride" in L.nrtLastError(a._h).decode()
    o = _sfx(other)
    assert getattr(L, "nrtRefit_" + o)(a._h, v1.astype(other).ctypes.data, np.dtype(other).itemsize * 3) == NRT_ERR_PRECISION
    with pytest.raises(TypeError):
        a.Refit(v1.astype(other))
    import torch

    dv = torch.from_numpy(v1).cuda()
    assert getattr(L, "nrtRefitDevice_" + s)(a._h, dv.data_ptr() + 1, v.itemsize * 3, None) == NRT_ERR_INVALID  # misaligned pointer
    assert getattr(L, "nrtRefitDevice_" + s)(a._h, dv.data_ptr(), v.itemsize * 3 + 1, None) == NRT_ERR_INVALID  # misaligned stride
    assert getattr(L, "nrtRefitDevice_" + s)(a._h, None, v.itemsize * 3, None) == NRT_ERR_INVALID
    n1, i1 = a.GetTree()
    assert n1.tobytes() == n0.tobytes() and i1.tobytes() == i0.tobytes()
    h1, m1 = a.TraverseBatch(cam)
    assert_hits_identical(h0, m0, h1, m1)
    a.close()


def test_refusals_of_sphere_and_cylinder_contexts():
    from nanort_amd import CylinderGeometry, SphereGeometry

    rng = np.random.default_rng(3)
    c = rng.uniform(-1, 1, size=(50, 3)).astype(np.float32)
    r = np.full(50, 0.05, np.float32)
    a = BVHAccel(np.float32)
    assert a.Build(50, SphereGeometry(c, r))
    with pytest.raises(NrtError) as e:
        a.Refit(c)
    assert e.value.status == NRT_ERR_INVALID and "spheres" in str(e.value)
    ends = rng.uniform(-1, 1, size=(50, 2, 3)).astype(np.float32)
    b = BVHAccel(np.float32)
    assert b.Build(50, CylinderGeometry(ends, np.full((50, 2), 0.02, np.float32)))
    with pytest.raises(NrtError) as e:
        b.Refit(ends.reshape(-1, 3))
    assert e.value.status == NRT_ERR_INVALID and "cylinders" in str(e.value)
    a.close()
    b.close()


def test_committed_scene_refuses_after_refit_until_recommitted(c1_mesh):
    v, f = c1_mesh
    v = np.ascontiguousarray(v.astype(np.float32))
    a = built(np.float32, v, f)
    sc = Scene()
    x = np.eye(4, dtype=np.float32)
    x2 = np.eye(4, dtype=np.float32)
    x2[3, :3] = (0.5, 0.0, -0.25)
    sc.AddNode(a, x)
    sc.AddNode(a, x2)
    assert sc.Commit()
    rays = scenes.camera_rays(64, 48)
    v1 = deformations(v)["wave"]
    a.Refit(v1)
    with pytest.raises(NrtError):
        sc.TraverseBatch(rays)
    assert sc.Commit()
    h, m = sc.TraverseBatch(rays)
    n1, i1 = a.GetTree()
    b = BVHAccel(np.float32)
    b.SetMesh(TriangleMesh(v1, f))
    b.SetTree(n1, i1)
    sc2 = Scene()
    sc2.AddNode(b, x)
    sc2.AddNode(b, x2)
    assert sc2.Commit()
    h2, m2 = sc2.TraverseBatch(rays)
    assert np.array_equal(m, m2) and h.tobytes() == h2.tobytes()
    assert m.any()
    sc.close()
    sc2.close()


def test_host_form_through_strides(oracle, c1):
    """nrtRefit from [nv, 4] rows (16 / 32-byte stride) and from rows at an odd byte stride (the byte-load gather)."""
    real, v, f, cam, bounce, rnd = c1
    a = built(real, v, f)
    n0, i0 = a.GetTree()
    it = np.dtype(real).itemsize
    for k, name in enumerate(("wave", "scale", "jitter")):
        v1 = deformations(v)[name]
        want = model_refit(n0, i0, v1, f)
        if k == 0:  # [nv, 4]: the array's own row stride
            a.Refit(np.concatenate([v1, np.full((v1.shape[0], 1), np.nan, real)], axis=1))
        else:  # rows of 3 * itemsize + 1 (k = 1) or + 5 (k = 2) bytes: not a multiple of the element size
            stride = 3 * it + (1 if k == 1 else 5)
            buf = np.full(((v1.shape[0] * stride) // it + 4,), np.nan, real)
            b8 = buf.view(np.uint8)
            for i in range(v1.shape[0]):
                b8[i * stride:i * stride + 3 * it] = np.frombuffer(v1[i].tobytes(), np.uint8)
            a.Refit(buf, vertex_stride_bytes=stride)
        n1, i1 = a.GetTree()
        assert topology_bytes(n1) == topology_bytes(n0)
        assert_boxes_equal(n1, want, "boxes (%s)" % name)
        check_traces(oracle, a, n1, i1, v1, f, (cam,))
    a.close()


@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_fresh_context_refit_is_no_tree(real):
    a = BVHAccel(real)
    s = _sfx(real)
    v = np.zeros((3, 3), real)
    assert getattr(a._L, "nrtRefit_" + s)(a._h, v.ctypes.data, 3 * v.itemsize) == NRT_ERR_INVALID
    assert "no tree" in a._L.nrtLastError(a._h).decode()
    a.close()


def test_short_tensor_refused_before_the_library(c1):
    import torch

    real, v, f, cam, bounce, rnd = c1
    a = built(real, v, f)
    n0, _ = a.GetTree()
    tdt = torch.float32 if real == np.float32 else torch.float64
    with pytest.raises(ValueError):
        a.RefitDevice(torch.from_numpy(v[:-1].copy()).to("cuda", tdt))
    with pytest.raises(ValueError):
        a.Refit(v[:-1])
    n1, _ = a.GetTree()
    assert n1.tobytes() == n0.tobytes()
    a.close()

"""Occlusion queries of sphere, cylinder and curve contexts on the GPU: nrtOccludedBatchPrims_f32 / nrtOccludedBatchPrimsDevice_f32
(include/nanort_hip.h, "occlusion queries for every primitive kind").  Every comparison is byte equality of the mask with
(closest-hit mask != 0) from the same context and with the kind's CPU oracle walking the same node and index arrays; every ray set
has at least a tenth of its rays hitting and a tenth missing (tests/occluded_fixture.py), asserted here again."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

import curves_fixture as cf
import occluded_fixture as of
from helpers import trace_options
from nanort_amd import BVHAccel, CurveGeometry, CylinderGeometry, SphereGeometry, TriangleMesh, capi
from oracle import bindings as ob

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND_ARG = {"spheres": "1", "cylinders": "2", "curves": "3"}  # k_traverse_wide<T, STACK, STATS, KIND, ...>


def flags01(mask):
    return (np.asarray(mask) != 0).astype(np.uint8)


def check_flags(a, kind, rays, options=None, oracle_mask=None, expect_mixed=True):
    """The occlusion mask of `a` for `rays`: 0 / 1, byte-equal to (closest-hit mask != 0) from the same context and to the oracle's.
    Returns (closest-hit records, closest-hit mask, occlusion mask)."""
    h, m = a.TraverseBatch(rays, options)
    occ = a.OccludedBatch(rays, options)
    name = a.LastKernelName()
    assert name.startswith("nrt::k_traverse_wide<float, ") and name.split(", ")[3] == KIND_ARG[kind], name
    assert occ.dtype == np.uint8 and set(np.unique(occ).tolist()) <= {0, 1}
    assert occ.tobytes() == flags01(m).tobytes(), "differs from the closest-hit flags at %s" % np.nonzero(occ != flags01(m))[0][:8]
    if oracle_mask is not None:
        assert occ.tobytes() == flags01(oracle_mask).tobytes(), "differs from the CPU oracle at %s" % np.nonzero(occ != flags01(oracle_mask))[0][:8]
    if expect_mixed:
        assert of.mixed(occ), float(occ.mean())
    return h, m, occ


def check_equality_edge(a, kind, rays, h, m, options=None):
    """Every hitting ray again with max_t = the t it returned: an acceptance at exactly max_t leaves the closest-hit flag 0 and must
    not stop the occlusion ray."""
    again = rays.copy()
    hit = m != 0
    again["max_t"][hit] = h["t"][hit]
    _, m2, occ2 = check_flags(a, kind, again, options, expect_mixed=False)
    assert int(occ2.sum()) < int(flags01(m).sum())  # (the edge is met: rays that hit no longer do)


# ---- spheres ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_cases():
    return {name: (c, r, rays) for name, c, r, rays in of.sphere_cases()}


@pytest.mark.parametrize("wide4", [1, 0], ids=["two_level", "one_level"])
@pytest.mark.parametrize("case", ["scene_rays", "scene_hostile", "degenerate", "n1", "n3"])
def test_spheres(case, wide4, sphere_cases):
    c, r, rays = sphere_cases[case]
    n = r.shape[0]
    a = BVHAccel(np.float32)
    a.SetTunable("wide4", wide4)
    assert a.Build(n, SphereGeometry(c, r))
    nodes, idx = a.GetTree()
    assert (nodes.shape[0] == 1) == (n <= 3)  # (n1, n3: the root is a leaf)
    _, om = ob.SphereOracle().traverse(nodes, idx, c, r, rays)
    h, m, _ = check_flags(a, "spheres", rays, None, om)
    check_equality_edge(a, "spheres", rays, h, m)
    if case == "scene_rays":
        upper = (n // 2, n)  # the lower half of the ids cannot be hit
        _, om = ob.SphereOracle().traverse(nodes, idx, c, r, rays, prim_ids_range=upper)
        hu, mu, occ = check_flags(a, "spheres", rays, trace_options(range_=upper), om)
        assert int(occ.sum()) < int(flags01(m).sum()) and hu["prim_id"][mu != 0].min() >= n // 2
        _, _, none = check_flags(a, "spheres", rays, trace_options(range_=(7, 7)), expect_mixed=False)  # an empty range
        assert not none.any()
        for count in (1, 63, 65):  # less than a wave, one lane more than a wave
            part = rays[12000:12000 + count]
            check_flags(a, "spheres", part, expect_mixed=False)


# ---- cylinders --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cylinder_cases():
    return {name: (v, r, rays) for name, v, r, rays in of.cylinder_cases()}


@pytest.mark.parametrize("cap", [1, 0], ids=["caps", "no_caps"])
@pytest.mark.parametrize("split", [1, 32], ids=["whole_boxes", "segments"])
@pytest.mark.parametrize("case", ["random3000", "degenerate"])
def test_cylinders(case, split, cap, cylinder_cases):
    v, r, rays = cylinder_cases[case]
    n = r.shape[0]
    a = BVHAccel(np.float32)
    a.SetTunable("cyl_split", split)
    assert a.Build(n, CylinderGeometry(v, r, test_cap=bool(cap)))
    nodes, idx = a.GetTree()
    if split == 32 and case == "random3000":
        assert idx.shape[0] > n  # leaves name a cylinder once per segment
    _, om = ob.CylinderOracle().traverse(nodes, idx, v, r, rays, test_cap=bool(cap))
    h, m, _ = check_flags(a, "cylinders", rays, None, om)
    check_equality_edge(a, "cylinders", rays, h, m)
    upper = (n // 2, n)
    _, om = ob.CylinderOracle().traverse(nodes, idx, v, r, rays, prim_ids_range=upper, test_cap=bool(cap))
    check_flags(a, "cylinders", rays, trace_options(range_=upper), om)


# ---- curves -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subdiv", [1, 4, 7, 64])
@pytest.mark.parametrize("scene", list(of.CURVE_SCENES))
def test_curves(scene, subdiv):
    cps, radii = cf.scene(scene)
    rays = of.curve_rays(scene)
    n = radii.shape[0]
    for wide4 in (1, 0):
        a = BVHAccel(np.float32)
        a.SetTunable("wide4", wide4)
        assert a.Build(n, CurveGeometry(cps, radii, subdiv))
        nodes, idx = a.GetTree()
        _, om = cf.model_traverse(nodes, idx, cps, radii, rays, subdiv)
        h, m, _ = check_flags(a, "curves", rays, None, om)
        check_equality_edge(a, "curves", rays, h, m)
        if n >= 5:
            upper = (n // 2, n)
            _, om = cf.model_traverse(nodes, idx, cps, radii, rays, subdiv, upper)
            check_flags(a, "curves", rays, trace_options(range_=upper), om, expect_mixed=False)


# ---- the Device form --------------------------------------------------------------------------------------------------------
def built(kind):
    if kind == "spheres":
        _, c, r, rays = of.sphere_cases()[0]
        mesh = SphereGeometry(c, r)
    elif kind == "cylinders":
        _, v, r, rays = of.cylinder_cases()[0]
        mesh = CylinderGeometry(v, r)
    else:
        mesh, rays = CurveGeometry(*cf.fur()), of.curve_rays("fur")
    a = BVHAccel(np.float32)
    assert a.Build(mesh.num_faces, mesh)
    return a, mesh, rays


@pytest.mark.parametrize("kind", ["spheres", "cylinders", "curves"])
def test_device_form_on_a_side_stream(kind):
    import torch

    a, _, rays = built(kind)
    want = a.OccludedBatch(rays)
    assert of.mixed(want)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    side = torch.cuda.Stream()
    for timing in (0, 1):
        a.SetLaunchTiming(timing)
        d_mask = torch.full((rays.shape[0],), 0xCD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert a.OccludedBatchDevice(d_rays, d_mask, stream=side) == rays.shape[0]
        side.synchronize()
        assert d_mask.cpu().numpy().tobytes() == want.tobytes()
        assert a.LastTraverseMs() >= 0
        assert a.LastKernelName().split(", ")[3] == KIND_ARG[kind]
    with pytest.raises(ValueError):  # these intersectors have no skip id
        a.OccludedBatch(rays, skip_prim_ids=np.zeros(rays.shape[0], dtype=np.uint32))
    with pytest.raises(ValueError):
        a.OccludedBatchDevice(d_rays, d_mask, skip_prim_ids=d_mask)


# ---- the completion record --------------------------------------------------------------------------------------------------
def within(seconds, fn):
    """fn() on a thread of its own, given up after `seconds` (the library calls release the interpreter lock)."""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as e:  # noqa: BLE001
            box["error"] = e

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(seconds)
    assert not t.is_alive(), "still waiting after %d s" % seconds
    if "error" in box:
        raise box["error"]
    return box["value"]


def test_completion_record_is_closed_without_a_post_pass():
    """An occlusion launch of a curve context runs no post pass, so the walk's last wave must close the launch's completion record:
    nrtSetCurves_f32 and nrtBuild_f32 wait for that record before they touch the tree."""
    import torch

    cps, radii = cf.fur()
    rays = of.curve_rays("fur")
    a = BVHAccel(np.float32)
    assert a.Build(radii.shape[0], CurveGeometry(cps, radii))
    want = flags01(a.TraverseBatch(rays)[1])
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    d_mask = torch.full((rays.shape[0],), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    within(20, lambda: a.OccludedBatchDevice(d_rays, d_mask))  # 1. (launch_timing 0: the record, no event)
    within(20, lambda: a.SetMesh(CurveGeometry(cps, radii, 7)))  # 2. these wait for the launch
    assert within(20, a.BuildCurrent)
    h, m = within(20, lambda: a.TraverseBatch(rays))  # 3.
    fresh = BVHAccel(np.float32)
    assert fresh.Build(radii.shape[0], CurveGeometry(cps, radii, 7))
    fh, fm = fresh.TraverseBatch(rays)
    assert h.tobytes() == fh.tobytes() and m.tobytes() == fm.tobytes() and of.mixed(m)
    torch.cuda.synchronize()
    assert d_mask.cpu().numpy().tobytes() == want.tobytes()  # (the launch of step 1)
    within(20, a.close)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_refusals_write_nothing(c1_mesh):
    import torch

    L = capi.lib()
    a, _, rays = built("spheres")
    rays = np.ascontiguousarray(rays[:500])
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()

    def refused(acc, status, host_args, dev_args):
        mask = np.full(n, 0xAB, dtype=np.uint8)
        d_mask = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r_, m_ = host_args
        assert L.nrtOccludedBatchPrims_f32(acc._h, _vp(rays) if r_ else None, n, None, _vp(mask) if m_ else None) == status
        assert L.nrtLastError(acc._h)
        r_, m_ = dev_args
        assert L.nrtOccludedBatchPrimsDevice_f32(acc._h, d_rays.data_ptr() if r_ else None, n, None, d_mask.data_ptr() if m_ else None, None) == status
        assert L.nrtLastError(acc._h)
        torch.cuda.synchronize()
        assert (mask == 0xAB).all() and bool((d_mask == 0xAB).all())

    v, f = c1_mesh
    t64 = BVHAccel(np.float64)
    assert t64.Build(f.shape[0], TriangleMesh(v.astype(np.float64), f))
    refused(t64, capi.NRT_ERR_PRECISION, (True, True), (True, True))
    no_tree = BVHAccel(np.float32)
    no_tree.SetMesh(SphereGeometry(*of.sphere_cases()[0][1:3]))
    refused(no_tree, capi.NRT_ERR_INVALID, (True, True), (True, True))
    refused(a, capi.NRT_ERR_INVALID, (False, True), (False, True))  # NULL rays
    refused(a, capi.NRT_ERR_INVALID, (True, False), (True, False))  # NULL mask
    mask = np.full(n, 0xAB, dtype=np.uint8)
    assert L.nrtOccludedBatchPrims_f32(a._h, None, 0, None, None) == capi.NRT_OK
    assert L.nrtOccludedBatchPrimsDevice_f32(a._h, None, 0, None, None, None) == capi.NRT_OK
    assert L.nrtOccludedBatchPrims_f32(a._h, _vp(rays), 0, None, _vp(mask)) == capi.NRT_OK and (mask == 0xAB).all()
    # the triangle contexts' calls refuse the kind as before
    assert L.nrtOccludedBatch_f32(a._h, _vp(rays), n, None, _vp(mask)) == capi.NRT_ERR_INVALID and (mask == 0xAB).all()
    assert a.OccludedBatch(rays).tobytes() == flags01(a.TraverseBatch(rays)[1]).tobytes()


# ---- triangles --------------------------------------------------------------------------------------------------------------
def test_triangle_contexts_take_the_existing_occlusion_path(c1_mesh):
    import torch

    from nanort_amd import scenes

    L = capi.lib()
    v, f = c1_mesh
    a = BVHAccel(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    rays = scenes.camera_rays(96, 96)
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    # (38 %, 29 % and 19 % of these rays hit under the three option sets, by the CPU oracle: triangle 6 is the one hit most often)
    for o in (None, trace_options(cull=True), trace_options(range_=(2, f.shape[0]), skip=6, cull=True)):
        want = a.OccludedBatch(rays, o)  # nrtOccludedBatch_f32
        k0 = a.LastKernelName()
        assert of.mixed(want)
        op = None if o is None else np.asarray(o).reshape(1)
        mask = np.full(n, 0xAB, dtype=np.uint8)
        assert L.nrtOccludedBatchPrims_f32(a._h, _vp(rays), n, _vp(op), _vp(mask)) == capi.NRT_OK
        assert mask.tobytes() == want.tobytes() and a.LastKernelName() == k0
        d_mask = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert L.nrtOccludedBatchPrimsDevice_f32(a._h, d_rays.data_ptr(), n, _vp(op), d_mask.data_ptr(), None) == capi.NRT_OK
        torch.cuda.synchronize()
        assert d_mask.cpu().numpy().tobytes() == want.tobytes()


# ---- the header methods -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header_check(tmp_path_factory):
    from test_occluded_kinds import CXX

    exe = str(tmp_path_factory.mktemp("occluded_kinds_check_hip") / "occluded_kinds_check_hip")
    libdir = os.path.join(ROOT, "nanort_amd", "lib")
    cmd = CXX + ["-o", exe, "-DNANORT_USE_HIP_BACKEND", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include", "-L", libdir, "-lnanort_hip",
                 "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


@pytest.mark.parametrize("kind", ["spheres", "cylinders", "curves"])
def test_header_methods(header_check, tmp_path, kind):
    """tests/cpp/occluded_kinds_check.cc with the backend macro: OccludedBatchSpheres / OccludedBatchCylinders / OccludedBatchCurves
    and their Device forms against the generic host OccludedBatch, test_cap and num_subdivisions changing between calls, on an
    accel that shares its context with a copy (the program checks all of that itself)."""
    from test_occluded_kinds import run_check, small_scene

    pos, radii, rays = small_scene(kind)
    flags = run_check(header_check, tmp_path, kind, pos, radii, rays, timeout=120)
    assert of.mixed(flags)

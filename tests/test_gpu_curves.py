"""The curve primitive on the GPU: nrtSetCurves_f32 (+ Device) -> nrtBuild_f32 / nrtSetTree_f32 -> nrtTraverseBatchCurves*_f32.
Every byte of every 40-byte record {t, prim_id, u, v, tangent, normal} and of the hit mask equals the CPU model
(tests/curves_model.c, itself pinned to the unmodified reference example by tests/test_curves_model.py) walking the same node and
index arrays; on the reference-built tree of the fur fixture they equal the reference's own recorded records."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import curves_fixture as cf
from helpers import reference_answers, trace_options
from nanort_amd import BVHAccel, CurveGeometry, NrtError, SphereGeometry, TriangleMesh, capi, scenes
from nanort_amd.wire import CURVE_HIT_F32, HIT_F32, default_build_options

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rays():
    return cf.all_rays()  # the example's camera on a 64 x 64 grid, then the hostile rays


def same(h, m, mh, mm):
    assert np.array_equal(m, mm), "hit masks differ at %s" % np.nonzero(m != mm)[0][:8]
    assert h.dtype == CURVE_HIT_F32 and h.tobytes() == mh.tobytes(), "records differ at %s" % np.nonzero(h != mh)[0][:8]


def check_against_model(a, cps, radii, r, subdiv=4, rng=None):
    nodes, idx = a.GetTree()
    h, m = a.TraverseBatch(r, None if rng is None else trace_options(range_=rng))
    mh, mm = cf.model_traverse(nodes, idx, cps, radii, r, subdiv, rng)
    same(h, m, mh, mm)
    return h, m


@pytest.mark.parametrize("wide4", [1, 0], ids=["two_level", "one_level"])
@pytest.mark.parametrize("scene", ["1", "2", "5", "fur", "3000"])
def test_parity_with_the_model_on_the_gpu_built_tree(scene, wide4, rays):
    cps, radii = cf.scene(scene)
    n = radii.shape[0]
    a = BVHAccel(np.float32)
    a.SetTunable("wide4", wide4)
    assert a.Build(n, CurveGeometry(cps, radii))
    nodes, idx = a.GetTree()
    assert sorted(idx.tolist()) == list(range(n))
    assert nodes.shape[0] == int(a.GetStatistics()["num_leaf_nodes"]) + int(a.GetStatistics()["num_branch_nodes"])
    lo, hi, _ = cf.model_boxes(cps, radii)
    assert np.array_equal(nodes[0]["bmin"], lo.min(axis=0)) and np.array_equal(nodes[0]["bmax"], hi.max(axis=0))
    h, m = check_against_model(a, cps, radii, rays)
    if n > 4:  # (up to min_leaf_primitives = 4 curves make a tree of one leaf: no records to walk two levels at a time)
        assert a.LastKernelName() == ("nrt::k_traverse_wide<float, 12, false, 3, false, false, 4, 0>" if wide4
                                      else "nrt::k_traverse_wide<float, 10, false, 3, false, false, 2, 0>")
    else:
        assert nodes.shape[0] == 1 and nodes[0]["flag"] == 1
    if scene in ("fur", "3000"):
        assert int(m[:4096].sum()) > (1000 if scene == "fur" else 900)  # (1099 and 995 with the model on the reference's trees)
    for count in (1, 63, 65):  # less than a wave, one lane more than a wave
        part = rays[1500:1500 + count]  # (rows of the camera that cross the ball)
        check_against_model(a, cps, radii, part)


@pytest.mark.parametrize("min_leaf", [1, 16])
def test_leaf_sizes_and_subdivision_counts(min_leaf, rays):
    cps, radii = cf.hair(3000)
    o = default_build_options()
    o["min_leaf_primitives"] = min_leaf
    for subdiv in (1, 4, 7):
        a = BVHAccel(np.float32)
        assert a.Build(3000, CurveGeometry(cps, radii, subdiv), o)
        nodes, _ = a.GetTree()
        leaf = nodes[nodes["flag"] == 1]["data"][:, 0]
        assert (np.median(leaf) == 1 and leaf.max() <= 4) if min_leaf == 1 else 4 < leaf.max() <= 16
        _, m = check_against_model(a, cps, radii, rays, subdiv)
        assert int(m.sum()) > 500


def test_prim_ids_range(rays):
    cps, radii = cf.hair(3000)
    a = BVHAccel(np.float32)
    assert a.Build(3000, CurveGeometry(cps, radii))
    h, m = check_against_model(a, cps, radii, rays, rng=(500, 2500))
    p = h["prim_id"][m == 1]
    assert p.size > 300 and p.min() >= 500 and p.max() < 2500
    h0, m0 = check_against_model(a, cps, radii, rays)
    assert int(m0.sum()) > int(m.sum())


def test_device_forms_equal_the_host_forms(rays):
    import torch

    cps, radii = cf.hair(3000)
    a = BVHAccel(np.float32)
    assert a.Build(3000, CurveGeometry(cps, radii, 7))
    nodes, idx = a.GetTree()
    h, m = a.TraverseBatch(rays)
    b = BVHAccel(np.float32)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_c, d_r = torch.from_numpy(cps).cuda(), torch.from_numpy(radii).cuda()
        b.SetCurvesDevice(d_c, d_r, 7, stream=side)
        d_c.zero_()  # (the context owns its copy: the caller's buffers are free on return)
        d_r.zero_()
    assert b.BuildCurrent()
    bn, bi = b.GetTree()
    assert bn.tobytes() == nodes.tobytes() and bi.tobytes() == idx.tobytes()
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    d_h = torch.full((rays.shape[0] * 40,), 0xCD, dtype=torch.uint8, device="cuda")
    d_m = torch.full((rays.shape[0],), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b.TraverseBatchDevice(d_rays, d_h, d_m, stream=side)
    side.synchronize()
    same(d_h.cpu().numpy().view(CURVE_HIT_F32), d_m.cpu().numpy(), h, m)
    # refusals of the Device set call leave the context as it was
    with pytest.raises(NrtError):
        b.SetCurvesDevice(torch.from_numpy(cps).cuda(), torch.from_numpy(radii).cuda(), 65)
    with pytest.raises(NrtError):
        b._check(b._L.nrtSetCurvesDevice_f32(b._h, d_rays.data_ptr() + 2, d_rays.data_ptr(), 8, 4, None))  # misaligned
    h2, m2 = b.TraverseBatch(rays)
    same(h2, m2, h, m)


def test_adopted_reference_tree_gives_the_references_records():
    g = cf.fur_golden()
    a = BVHAccel(np.float32)
    a.SetMesh(CurveGeometry(g["cps"], g["radii"]))
    a.SetTree(g["nodes"], g["indices"])
    h, m = a.TraverseBatch(cf.camera())
    same(h, m, g["hits"], g["mask"])
    assert int(m.sum()) > 1000


@pytest.mark.parametrize("subdiv", [4, 7])
def test_degenerate_curves_and_hostile_rays_on_the_reference_tree(subdiv, rays):
    """All control points equal, radius 0, a NaN control point, a curve behind the eye, a zero-length segment: over the tree the
    reference built (its recording), against the model, NaNs compared as NaNs."""
    cps, radii = cf.degenerate()
    nodes, idx, _ = reference_answers("curves_degenerate_s%d" % subdiv)
    a = BVHAccel(np.float32)
    a.SetMesh(CurveGeometry(cps, radii, subdiv))
    a.SetTree(nodes, idx)
    h, m = a.TraverseBatch(rays)
    mh, mm = cf.model_traverse(nodes, idx, cps, radii, rays, subdiv)
    assert np.array_equal(m, mm)
    for f in CURVE_HIT_F32.names:
        assert np.array_equal(h[f], mh[f], equal_nan=True), f


def test_every_other_entry_point_refuses_a_curve_context(rays):
    import torch

    cps, radii = cf.hair(400)
    a = BVHAccel(np.float32)
    assert a.Build(400, CurveGeometry(cps, radii))
    L, c = a._L, a._h
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    r = np.ascontiguousarray(rays[:256])
    n = r.shape[0]
    hits = np.zeros(n * 4, dtype=HIT_F32)
    flags = np.zeros(n * 4, dtype=np.uint8)
    counts32 = np.zeros(n, dtype=np.uint32)
    d_r = torch.from_numpy(r.view(np.uint8).reshape(-1)).cuda()
    d_h = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    d_m = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    p = lambda x: x.ctypes.data_as(vp)  # noqa: E731
    rp, hp, mp = (vp * 1)(r.ctypes.data), (vp * 1)(hits.ctypes.data), (vp * 1)(flags.ctypes.data)
    drp, dhp, dmp = (vp * 1)(d_r.data_ptr()), (vp * 1)(d_h.data_ptr()), (vp * 1)(d_m.data_ptr())
    cnt = (u64 * 1)(n)
    ctxs = (vp * 1)(c)
    counters = capi.TraceCounters()
    xform = np.eye(4, dtype=np.float32)
    INV, PREC = capi.NRT_ERR_INVALID, capi.NRT_ERR_PRECISION
    calls = [
        ("nrtTraverseBatch_f32", INV, lambda: L.nrtTraverseBatch_f32(c, p(r), n, None, p(hits), p(flags))),
        ("nrtTraverseBatch_f64", PREC, lambda: L.nrtTraverseBatch_f64(c, p(r), n // 2, None, p(hits), p(flags))),
        ("nrtTraverseBatchDevice_f32", INV, lambda: L.nrtTraverseBatchDevice_f32(c, d_r.data_ptr(), n, None, d_h.data_ptr(), d_m.data_ptr(), None)),
        ("nrtTraverseBatchDevice_f64", PREC, lambda: L.nrtTraverseBatchDevice_f64(c, d_r.data_ptr(), n // 2, None, d_h.data_ptr(), d_m.data_ptr(), None)),
        ("nrtTraverseBatches_f32", INV, lambda: L.nrtTraverseBatches_f32(c, 1, rp, cnt, None, hp, mp, None)),
        ("nrtTraverseBatchesDevice_f32", INV, lambda: L.nrtTraverseBatchesDevice_f32(c, 1, drp, cnt, None, dhp, dmp, None, None)),
        ("nrtTraverseBatchCylinders_f32", INV, lambda: L.nrtTraverseBatchCylinders_f32(c, p(r), n, None, p(hits), p(flags))),
        ("nrtTraverseBatchCylindersDevice_f32", INV,
         lambda: L.nrtTraverseBatchCylindersDevice_f32(c, d_r.data_ptr(), n, None, d_h.data_ptr(), d_m.data_ptr(), None)),
        ("nrtOccludedBatch_f32", INV, lambda: L.nrtOccludedBatch_f32(c, p(r), n, None, p(flags))),
        ("nrtOccludedBatch_f64", PREC, lambda: L.nrtOccludedBatch_f64(c, p(r), n // 2, None, p(flags))),
        ("nrtOccludedBatchDevice_f32", INV, lambda: L.nrtOccludedBatchDevice_f32(c, d_r.data_ptr(), n, None, d_m.data_ptr(), None)),
        ("nrtMultiHitTraverseBatch_f32", INV, lambda: L.nrtMultiHitTraverseBatch_f32(c, p(r), n, 4, None, p(hits), p(counts32))),
        ("nrtMultiHitTraverseBatch_f64", PREC, lambda: L.nrtMultiHitTraverseBatch_f64(c, p(r), n // 2, 2, None, p(hits), p(counts32))),
        ("nrtMultiHitTraverseBatchDevice_f32", INV,
         lambda: L.nrtMultiHitTraverseBatchDevice_f32(c, d_r.data_ptr(), n, 4, None, d_h.data_ptr(), d_m.data_ptr(), None)),
        ("nrtRefit_f32", INV, lambda: L.nrtRefit_f32(c, p(cps), 12)),
        ("nrtRefit_f64", PREC, lambda: L.nrtRefit_f64(c, p(cps), 24)),
        ("nrtRefitDevice_f32", INV, lambda: L.nrtRefitDevice_f32(c, d_h.data_ptr(), 12, None)),
        ("nrtTraverseBatchMulti_f32", INV, lambda: L.nrtTraverseBatchMulti_f32(ctxs, 1, p(r), n, 0, None, p(hits), p(flags))),
        ("nrtTraverseCountDevice_f32", INV, lambda: L.nrtTraverseCountDevice_f32(c, d_r.data_ptr(), n, None, ctypes.byref(counters))),
        ("nrtSetCurves_f32 (num_subdivisions 0)", INV, lambda: L.nrtSetCurves_f32(c, p(cps), p(radii), 400, 0)),
        ("nrtSetCurves_f32 (num_subdivisions 65)", INV, lambda: L.nrtSetCurves_f32(c, p(cps), p(radii), 400, 65)),
        ("nrtSetCurves_f32 (NULL radii)", INV, lambda: L.nrtSetCurves_f32(c, p(cps), None, 400, 4)),
        ("nrtSetMesh_f64", PREC, lambda: L.nrtSetMesh_f64(c, p(cps), 24, p(counts32), 1)),
        ("nrtBuild_f64", PREC, lambda: L.nrtBuild_f64(c, None, None, None)),
    ]
    for name, want, call in calls:
        st = call()
        assert st == want, (name, st, L.nrtLastError(c))
        assert len(L.nrtLastError(c)) > 0, name
    # a scene refuses to instance it
    s = vp()
    assert L.nrtSceneCreate(0, ctypes.byref(s)) == capi.NRT_OK
    nid = u32(0)
    assert L.nrtSceneAddNode_f32(s, c, p(xform), ctypes.byref(nid)) == INV and b"curves" in L.nrtSceneLastError(s)
    L.nrtSceneDestroy(s)
    # a group over it is refused when it traces
    L.nrtGroupCreate.argtypes = [ctypes.POINTER(vp), u32, ctypes.POINTER(vp)]
    L.nrtGroupDestroy.argtypes = [vp]
    L.nrtGroupDestroy.restype = None
    L.nrtGroupLastError.argtypes = [vp]
    L.nrtGroupLastError.restype = ctypes.c_char_p
    L.nrtGroupTraverseGather_f32.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(u64), u64, u64, vp, u32, vp, vp]
    g = vp()
    assert L.nrtGroupCreate(ctxs, 1, ctypes.byref(g)) == capi.NRT_OK, L.nrtGroupLastError(None)
    try:
        assert L.nrtGroupTraverseGather_f32(g, drp, cnt, n, n, None, 0, d_h.data_ptr(), d_m.data_ptr()) == INV
        assert b"curve" in L.nrtGroupLastError(g)
    finally:
        L.nrtGroupDestroy(g)
    torch.cuda.synchronize()
    # ... and the context still traces, and matches
    check_against_model(a, cps, radii, rays)
    # the curve calls refuse every other kind
    v, f = scenes.load_c1_mesh()
    t = BVHAccel(np.float32)
    assert t.Build(f.shape[0], TriangleMesh(v, f))
    ch = np.zeros(n, dtype=CURVE_HIT_F32)
    assert L.nrtTraverseBatchCurves_f32(t._h, p(r), n, None, p(ch), p(flags)) == INV
    assert L.nrtTraverseBatchCurvesDevice_f32(t._h, d_r.data_ptr(), n, None, d_h.data_ptr(), d_m.data_ptr(), None) == INV
    d = BVHAccel(np.float64)
    assert d.Build(f.shape[0], TriangleMesh(v.astype(np.float64), f))
    assert L.nrtSetCurves_f32(d._h, p(cps), p(radii), 400, 4) == PREC


def test_one_context_through_triangles_curves_spheres_curves(rays):
    """No state of one kind survives into the next: the same context as a triangle mesh, curves, spheres and other curves with
    another subdivision count, then as cut cylinders, spheres and curves set from device memory, uncut cylinders and a mesh set from
    device memory, compared after every switch."""
    from oracle import bindings as ob

    v, f = scenes.load_c1_mesh()
    tri_rays = scenes.camera_rays(64, 64)
    cps, radii = cf.hair(3000)
    a = BVHAccel(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    nodes, idx = a.GetTree()
    h, m = a.TraverseBatch(tri_rays)
    oh, om = ob.Oracle().traverse(nodes, idx, v, f, tri_rays)
    assert h.tobytes() == oh.tobytes() and np.array_equal(m, om)
    assert a.Build(3000, CurveGeometry(cps, radii, 7))
    check_against_model(a, cps, radii, rays, 7)
    sc, sr = scenes.random_spheres(500)
    assert a.Build(500, SphereGeometry(sc, sr))
    nodes, idx = a.GetTree()
    srays = scenes.particle_camera_rays(64, 64)
    h, m = a.TraverseBatch(srays)
    oh, om = ob.SphereOracle().traverse(nodes, idx, sc, sr, srays)
    assert np.array_equal(m, om) and h["t"].tobytes() == oh["t"].tobytes() and np.array_equal(h["prim_id"], oh["prim_id"])
    fc, fr = cf.fur()
    assert a.Build(400, CurveGeometry(fc, fr))
    check_against_model(a, fc, fr, rays)
    # ... and on through the setters that share one path (api_geometry.hip), 64 primitives and 256 rays a stage: what one of them could leave
    # behind for the next is the segment array, the radii, the faces, test_cap and the subdivision count
    import torch

    from nanort_amd import CylinderGeometry
    from test_gpu_cylinders import check as check_cylinders
    from test_gpu_prim_kinds import aimed, box_mesh
    from test_gpu_spheres import check as check_spheres

    # 1. cylinders long enough to be cut: needles of 50 radii, so seven segments each at the default cyl_split / cyl_seg_radii
    cv, _ = scenes.random_cylinders(64)
    length = np.linalg.norm(cv[:, 1].astype(np.float64) - cv[:, 0], axis=1)
    cr = np.repeat((length / 50.0).astype(np.float32)[:, None], 2, axis=1)
    assert float((length / cr[:, 0]).min()) >= 40.0
    crays = aimed(scenes.particle_camera_rays(16, 16), cv.mean(axis=1))
    assert a.Build(64, CylinderGeometry(cv, cr))
    nodes, idx = a.GetTree()
    assert idx.shape[0] > 64 and sorted(set(idx.tolist())) == list(range(64))  # (num_segs > n)
    h, m = a.TraverseBatch(crays)
    check_cylinders(h, m, *ob.CylinderOracle().traverse(nodes, idx, cv, cr, crays))
    assert int(m.sum()) >= 32
    # 2. spheres, from device memory
    sc, sr = scenes.random_spheres(64)
    srays = aimed(scenes.particle_camera_rays(16, 16), sc)
    a.SetSpheresDevice(torch.from_numpy(sc).cuda(), torch.from_numpy(sr).cuda())
    assert a.BuildCurrent()
    nodes, idx = a.GetTree()
    assert sorted(idx.tolist()) == list(range(64))
    h, m = a.TraverseBatch(srays)
    check_spheres(h, m, *ob.SphereOracle().traverse(nodes, idx, sc, sr, srays))
    assert int(m.sum()) >= 32
    # 3. curves, from device memory, three subdivisions
    hc, hr = cf.hair(64)
    hrays = aimed(cf.camera(16, 16), (hc[:, 0] + 3 * hc[:, 1] + 3 * hc[:, 2] + hc[:, 3]) / np.float32(8))
    a.SetCurvesDevice(torch.from_numpy(hc).cuda(), torch.from_numpy(hr).cuda(), 3)
    assert a.BuildCurrent()
    check_against_model(a, hc, hr, hrays, 3)
    # 4. the same cylinders uncut (cyl_split = 1), without their caps: the tree is over the 64 whole boxes
    a.SetTunable("cyl_split", 1)
    assert a.Build(64, CylinderGeometry(cv, cr, test_cap=False))
    nodes, idx = a.GetTree()
    assert sorted(idx.tolist()) == list(range(64))
    h, m = a.TraverseBatch(crays)
    check_cylinders(h, m, *ob.CylinderOracle().traverse(nodes, idx, cv, cr, crays, test_cap=False))
    assert int(m.sum()) >= 32
    # 5. triangles, from device memory: the 12-triangle box
    bv, bf = box_mesh()
    brays = scenes.camera_rays(16, 16)
    assert a.BuildDevice(torch.from_numpy(bv).cuda(), torch.from_numpy(bf.view(np.int32).copy()).cuda())
    nodes, idx = a.GetTree()
    h, m = a.TraverseBatch(brays)
    oh, om = ob.Oracle().traverse(nodes, idx, bv, bf, brays)
    assert h.tobytes() == oh.tobytes() and np.array_equal(m, om) and m.any()


def test_header_backend_build_and_batch_equal_the_host_loop(tmp_path):
    """tests/cpp/curves_check.cc with the backend macro: Build() over (BezierCurveGeometry, BezierCurvePred) on the GPU,
    TraverseBatch(BezierCurveIntersection*) == the per-ray host Traverse with the built-in intersector on the read-back tree (the
    program checks that itself, for two subdivision counts), and the records it writes are the model's."""
    from test_curves_abi import run_check, same_hits

    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "nanort_amd", "lib")
    exe = str(tmp_path / "curves_check_hip")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-invalid-offsetof", "-I", inc,
           os.path.join(ROOT, "tests", "cpp", "curves_check.cc"), "-o", exe, "-DNANORT_USE_HIP_BACKEND", "-D__HIP_PLATFORM_AMD__", "-isystem",
           "/opt/rocm/include", "-L", libdir, "-lnanort_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    cps, radii = cf.fur()
    rays = cf.all_rays()
    nodes, idx, h, m = run_check(exe, tmp_path, cps, radii, rays, 4)
    mh, mm = cf.model_traverse(nodes, idx, cps, radii, rays, 4)
    assert same_hits(h, m, mh, mm) > 1000

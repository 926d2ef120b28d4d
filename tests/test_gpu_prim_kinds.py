"""What the setters of the four primitive kinds share (nanort_amd/csrc/api_geometry.hip: one path from the refusals to the adopted
primitives) and the pass behind a walk over spheres, cylinders and curves (prims.hip, launch_post_pass), on small sets:
  * each of the seven set entry points takes n == 0, leaves a context that builds nothing and traces nothing, and takes the same
    primitives again with the same records as before;
  * a context that has just traced on a caller's stream is set and built again at once: the setter waits for the launch through
    the completion record, which the post pass closes, and nothing of the earlier launch or of the earlier primitives shows in the
    records.  (A sphere launch without records, which the walk would close itself, cannot be asked for: the case pins the refusals.)"""
import numpy as np
import pytest

import curves_fixture as cf
from nanort_amd import BVHAccel, CurveGeometry, CylinderGeometry, NrtError, SphereGeometry, TriangleMesh, capi, scenes
from nanort_amd.wire import CURVE_HIT_F32, CYL_HIT_F32, HIT_F32

pytestmark = pytest.mark.gpu
N = 64


def box_mesh(lo=(-3.0, 2.0, -3.0), hi=(3.0, 8.0, 3.0)):
    """A box of 12 triangles in the view of scenes.camera_rays (the eye at (0, 5, 20), looking down -z)."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    v = np.array([[(hi if (i >> k) & 1 else lo)[k] for k in range(3)] for i in range(8)], dtype=np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]],
                 dtype=np.uint32)
    return v, f


def aimed(rays, targets):
    """`rays` with the first len(targets) of them turned towards `targets`: whatever the camera sees, these hit."""
    r = rays.copy()
    k = targets.shape[0]
    r["dir"][:k] = (targets - r["org"][:k]).astype(np.float32)
    return r


def triangle_set(scale=1.0):
    """64 triangles: the box and 52 more over a cloud of vertices around it."""
    rng = np.random.default_rng(3)
    v, f = box_mesh()
    cloud = rng.uniform((-8.0, -3.0, -4.0), (8.0, 13.0, 4.0), size=(40, 3)).astype(np.float32)
    more = rng.integers(8, 48, size=(N - 12, 3), dtype=np.uint32)
    return (np.concatenate([v, cloud]) * np.float32(scale)).astype(np.float32), np.concatenate([f, more])


def geometry(kind, scale=1.0):
    """(geometry, 256 rays of which the first 64 aim at one primitive each) of `kind`; `scale` != 1: another set of the same size."""
    s = np.float32(scale)
    if kind == "triangles":
        v, f = triangle_set(scale)
        return TriangleMesh(v, f), aimed(scenes.camera_rays(16, 16), v[f].mean(axis=1))
    if kind == "spheres":
        c, r = scenes.random_spheres(N)
        return SphereGeometry(c * s, r * s), aimed(scenes.particle_camera_rays(16, 16), c * s)
    if kind == "cylinders":
        v, r = scenes.random_cylinders(N)
        return CylinderGeometry(v * s, r * s), aimed(scenes.particle_camera_rays(16, 16), (v * s).mean(axis=1))
    c, r = cf.hair(N)
    mid = (c[:, 0] + 3 * c[:, 1] + 3 * c[:, 2] + c[:, 3]) / np.float32(8)  # the curve's point at u = 1/2
    return CurveGeometry(c * s, r * s, 3), aimed(cf.camera(16, 16), mid * s)


def set_device(a, g, stream=None):
    import torch

    if isinstance(g, TriangleMesh):
        a.SetMeshDevice(torch.from_numpy(g.vertices).cuda(), torch.from_numpy(g.faces.view(np.int32).copy()).cuda(), stream)
    elif isinstance(g, SphereGeometry):
        a.SetSpheresDevice(torch.from_numpy(g.centers).cuda(), torch.from_numpy(g.radii).cuda(), stream)
    else:
        a.SetCurvesDevice(torch.from_numpy(g.control_points).cuda(), torch.from_numpy(g.radii).cuda(), g.num_subdivisions, stream)


def none_of(g):
    if isinstance(g, TriangleMesh):
        return TriangleMesh(g.vertices, g.faces[:0])
    if isinstance(g, SphereGeometry):
        return SphereGeometry(g.centers[:0], g.radii[:0])
    if isinstance(g, CylinderGeometry):
        return CylinderGeometry(g.endpoints[:0], g.radii[:0])
    return CurveGeometry(g.control_points[:0], g.radii[:0], g.num_subdivisions)


ENTRY_POINTS = [("triangles", False), ("triangles", True), ("spheres", False), ("spheres", True), ("cylinders", False), ("curves", False),
                ("curves", True)]


@pytest.mark.parametrize("kind,device", ENTRY_POINTS, ids=["nrtSetMesh", "nrtSetMeshDevice", "nrtSetSpheres", "nrtSetSpheresDevice",
                                                           "nrtSetCylinders", "nrtSetCurves", "nrtSetCurvesDevice"])
def test_an_empty_set_between_two_sets_of_the_same_primitives(kind, device):
    g, rays = geometry(kind)
    put = (lambda a, x: set_device(a, x)) if device else (lambda a, x: a.SetMesh(x))
    a = BVHAccel(np.float32)
    put(a, g)
    assert a.BuildCurrent()
    h0, m0 = a.TraverseBatch(rays)
    assert int(m0[:N].sum()) >= N // 2  # (the aimed rays: a hit may be refused only where a ray grazes its target)
    put(a, none_of(g))  # NRT_OK
    assert a.BuildCurrent() is False  # NRT_ERR_EMPTY
    assert not a.IsValid()
    with pytest.raises(NrtError) as e:
        a.TraverseBatch(rays)
    assert e.value.status == capi.NRT_ERR_INVALID and "no tree" in str(e.value)
    put(a, g)
    assert a.BuildCurrent()
    h1, m1 = a.TraverseBatch(rays)
    assert h1.tobytes() == h0.tobytes() and m1.tobytes() == m0.tobytes()
    a.close()


def fresh(g, rays):
    a = BVHAccel(np.float32)
    assert a.Build(g.num_faces, g)
    h, m = a.TraverseBatch(rays)
    a.close()
    return h, m


@pytest.mark.timeout(120)  # (a completion record that nobody closes turns into an error after the library's 30 s, not into a hang)
@pytest.mark.parametrize("kind,records", [("spheres", True), ("spheres", False), ("cylinders", True), ("curves", True)],
                         ids=["spheres", "spheres_mask_only", "cylinders", "curves"])
def test_set_and_build_again_right_behind_a_trace_on_a_side_stream(kind, records):
    import torch

    g, rays = geometry(kind)
    g2, rays2 = geometry(kind, 1.5)
    dt = {"spheres": HIT_F32, "cylinders": CYL_HIT_F32, "curves": CURVE_HIT_F32}[kind]
    want, want_m = fresh(g, rays)
    want2, want2_m = fresh(g2, rays2)
    a = BVHAccel(np.float32)
    assert a.Build(N, g)
    side = torch.cuda.Stream()
    d_r = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    d_h = torch.full((rays.shape[0] * dt.itemsize,), 0xCD, dtype=torch.uint8, device="cuda")
    d_m = torch.full((rays.shape[0],), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if records:
        a.TraverseBatchDevice(d_r, d_h, d_m, stream=side)
    else:
        # Flags only would be a sphere launch without a post pass, the walk publishing the record itself: no entry point of the C ABI
        # issues one.  The closest-hit calls refuse NULL hits and occlusion queries refuse the kind, before anything is launched.
        L, n = a._L, rays.shape[0]
        assert L.nrtTraverseBatchDevice_f32(a._h, d_r.data_ptr(), n, None, None, d_m.data_ptr(), side.cuda_stream) == capi.NRT_ERR_INVALID
        assert b"NULL hits" in L.nrtLastError(a._h)
        assert L.nrtOccludedBatchDevice_f32(a._h, d_r.data_ptr(), n, None, d_m.data_ptr(), side.cuda_stream) == capi.NRT_ERR_INVALID
    assert a.Build(N, g2)  # at once: the host setter waits for the launch, then replaces what it reads
    h2, m2 = a.TraverseBatch(rays2)
    assert h2.tobytes() == want2.tobytes() and m2.tobytes() == want2_m.tobytes()
    side.synchronize()
    if records:
        assert d_m.cpu().numpy().tobytes() == want_m.tobytes() and d_h.cpu().numpy().tobytes() == want.tobytes()
    else:
        assert bool((d_m == 0xCD).all())  # (refused: nothing was written)
    assert int(want_m[:N].sum()) >= N // 2 and int(want2_m[:N].sum()) >= N // 2
    a.close()

"""nrtSignedDistanceBatch* and nrtGetFeatureNormals* on the GPU (tests/sdf_fixture.py, tests/sdf_model.cc), in fp32 and fp64: the
normals the library derives on the device against the model's and against a long-double formulation, records and found bytes
byte-identical to the model's brute force fed with the normals downloaded from the library, the signs against the winding number,
staleness across refits, mesh changes and rebuilds, refusals, and the closest-point query unchanged beside it."""
import os
import re

import numpy as np
import pytest

import closest_fixture as cf
import sdf_fixture as sf
from nanort_amd import BVHAccel, TriangleMesh, scenes
from nanort_amd.accel import MotionTriangleMesh, SphereGeometry
from nanort_amd.capi import NRT_ERR_INVALID, NRT_ERR_PRECISION, NRT_OK, NrtError
from nanort_amd.wire import point_dtype, signed_dtype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REALS = [np.float32, np.float64]
IDS = ["f32", "f64"]
ALL_NAMES = sf.CLOSED_NAMES + sf.HOSTILE_NAMES


def _sfx(real):
    return IDS[REALS.index(real)]


def built(real, v, f):
    a = BVHAccel(real)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    return a


def classes(real):
    cf.require_reference()
    d = dict(sf.closed_classes(real))
    d.update(sf.hostile_classes(real))
    return d


def to_device(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def device_query(a, pts, opts=None, stream=None, fill=0):
    import torch

    n = pts.shape[0]
    d_pts = to_device(pts)
    d_out = torch.full((n * signed_dtype(a.real).itemsize,), fill, dtype=torch.uint8, device="cuda")
    d_found = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    a.SignedDistanceBatchDevice(d_pts, d_out, d_found, options=cf.trace_options(opts), stream=stream)
    if stream is not None:
        stream.synchronize()
    return d_out.cpu().numpy().view(signed_dtype(a.real)), d_found.cpu().numpy()


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# The device's atan2 is not the host's, so a vertex normal of the library differs from the model's by what the angles differ by: the
# OpenCL bound on atan2 is 6 ulp = 3 eps of each angle (eps = 2^-23 / 2^-52, two ulp of a value below it), the product angle * n
# adds half an ulp per term, and the partial sums are rounded alike (the same terms in the same order, to within those differences).
# Per component |n| <= 1, so the difference is below 4 eps x the sum of the vertex's corner angles; asserted: 4.
VERTEX_VS_MODEL = 4.0


def assert_library_normals(real, name, v, f, normals):
    """Face and edge normals byte-identical to the model's (only + - x / sqrt, all correctly rounded on the device in this build);
    vertex normals within VERTEX_VS_MODEL of the model's and, on the closed classes, within eight times the measured error of the
    long-double reference."""
    fn, vn = normals
    mfn, mvn = sf.model_normals(v, f, v.shape[0])
    assert fn.shape == mfn.shape and vn.shape == mvn.shape
    assert same_bytes(fn, mfn), "%s: %d face / edge normal entries differ from the model's" % (name, (fn != mfn).sum())
    eps = np.finfo(real).eps
    angles = (sf.closed_reference(name)["normals"] if name in sf.CLOSED_NAMES else sf.reference_normals(v, f))[3].astype(np.float64)
    diff = np.abs(vn.astype(np.float64) - mvn.astype(np.float64)).max(axis=1)
    unit = eps * np.maximum(angles, np.finfo(np.float64).tiny)
    print("%s %s: vertex normals differ from the model's by at most %.3f eps x angles" % (_sfx(real), name, float((diff / unit).max())))
    assert (diff <= VERTEX_VS_MODEL * unit).all()
    assert (vn[angles == 0] == 0).all()
    if name in sf.CLOSED_NAMES:
        ef, ev = sf.normals_error(real, (fn, vn), sf.closed_reference(name)["normals"])
        print("%s %s: against long double: face/edge %.3f eps, vertex %.3f eps x angles" % (_sfx(real), name, ef, ev))
        assert ef <= 8 * sf.MEASURED_FACE_NORMAL_ERROR[_sfx(real)] and ev <= 8 * sf.MEASURED_VERTEX_NORMAL_ERROR[_sfx(real)]


@pytest.mark.parametrize("name", ALL_NAMES)
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_every_class(real, name):
    """Per class: the normals (twice: identical bytes), the host form and the Device form on a non-default stream byte-identical to
    the model's brute force with the library's normals, a range, a skip id and finite radii, and on the closed classes the signs
    against the winding number."""
    import torch

    v, f, pts = classes(real)[name]
    a = built(real, v, f)
    normals = a.FeatureNormals()
    assert_library_normals(real, name, v, f, normals)
    out, found = a.SignedDistanceBatch(pts)
    assert a.LastKernelName() == "nrt::k_signed_distance<%s, 32>" % ("float" if real == np.float32 else "double")
    exp = sf.brute(v, f, normals, pts)
    cf.assert_same(out, found, *exp, what="%s, host form" % name)
    sf.assert_word_is_clean(out, found)
    cf.assert_same(*device_query(a, pts, stream=torch.cuda.Stream()), *exp, what="%s, Device form" % name)
    nf = f.shape[0]
    radii = pts.copy()
    radii["max_dist"][1::2] = np.asarray(0.3, dtype=real)
    have = exp[0]["prim_id"][exp[1] != 0]
    busiest = int(np.bincount(have).argmax())
    for what, p, opts in (("radii", radii, None), ("range", pts, (nf // 3, max(nf // 3 + 1, 2 * nf // 3), 0xFFFFFFFF)), ("skip", radii, (0, 0x7FFFFFFF, busiest))):
        e = sf.brute(v, f, normals, p, opts)
        cf.assert_same(*a.SignedDistanceBatch(p, options=cf.trace_options(opts)), *e, what="%s, %s" % (name, what))
        sf.assert_word_is_clean(*e)
    again = BVHAccel(real)
    again.SetMesh(TriangleMesh(v, f))  # (the normals need a mesh, not a tree)
    n2 = again.FeatureNormals()
    assert same_bytes(n2[0], normals[0]) and same_bytes(n2[1], normals[1]), "two runs give different normal bytes"
    if name in sf.CLOSED_NAMES:
        ref, ok = sf.closed_reference(name), sf.checked(real, name)
        wrong = (sf.inside_bits(out) != ref["inside"]) & ok
        print("%s %s: %d checked, %d wrong signs" % (_sfx(real), name, ok.sum(), wrong.sum()))
        assert found.all() and wrong.sum() == 0, np.nonzero(wrong)[0][:8]
        if name == "wedge":
            short, _ = sf.brute(v, f, normals, pts, face_normal_only=True)
            assert ((sf.inside_bits(short) != ref["inside"]) & ok).sum() >= ok.sum() / 10.0


@pytest.mark.parametrize("name", sf.CLOSED_NAMES)
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_closest_point_query_is_unchanged(real, name):
    v, f, pts = classes(real)[name]
    a = built(real, v, f)
    out, found = a.ClosestPointBatch(pts)
    cf.assert_same(out, found, *cf.brute(v, f, pts), what=name)
    assert not out["_pad"].any()
    assert a.LastKernelName() == "nrt::k_closest_point<%s, 32>" % ("float" if real == np.float32 else "double")


@pytest.mark.parametrize("real", REALS, ids=IDS)
@pytest.mark.parametrize("nf", [1, 2])
def test_tiny_trees(real, nf):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], dtype=real)
    f = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.uint32)[:nf]
    a = built(real, v, f)
    rng = np.random.default_rng(3)
    xyz = np.concatenate([rng.uniform(-1, 2, size=(190, 3)), v.astype(np.float64), [[0.5, 0.5, 0.0], [0.5, 0.5, 0.25]]])
    pts = cf.make_points(real, xyz, np.where(np.arange(xyz.shape[0]) % 3 == 0, 0.4, np.inf))
    normals = a.FeatureNormals()
    assert_library_normals(real, "%d face(s)" % nf, v[:sf.num_verts(f)], f, normals)
    out, found = a.SignedDistanceBatch(pts)
    cf.assert_same(out, found, *sf.brute(v, f, normals, pts), what="%d triangle(s)" % nf)
    assert 0 < found.sum() < found.shape[0] and 0 < sf.inside_bits(out).sum() < found.sum()


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_deep_adopted_tree(oracle, real):
    """SetTree with the reference's tree of a grid mesh, deeper than the LDS stack (as tests/test_gpu_closest.py)."""
    v32, f = scenes.plane(300, 150)
    v = v32.astype(real)
    nodes, idx, st = oracle.build(v, f)
    assert st["max_tree_depth"] > 40
    a = BVHAccel(real)
    a.SetMesh(TriangleMesh(v, f))
    a.SetTree(nodes, idx)
    rng = np.random.default_rng(11)
    c = 0.5 * (v32.min(0) + v32.max(0)).astype(np.float64)
    ext = float(np.linalg.norm(v32.max(0) - v32.min(0)))
    d = rng.normal(size=(150, 3))
    far = c + d / np.linalg.norm(d, axis=1)[:, None] * ext * rng.uniform(20, 60, size=(150, 1))
    near = c + rng.uniform(-0.5, 0.5, size=(50, 3)) * ext
    pts = cf.make_points(real, np.concatenate([far, near]), np.inf)
    normals = a.FeatureNormals()
    out, found = a.SignedDistanceBatch(pts)
    cf.assert_same(out, found, *sf.brute(v, f, normals, pts), what="deep tree")
    assert found.all() and 0 < sf.inside_bits(out).sum() < found.shape[0]


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_motion_context_answers_for_keyframe_0(real):
    v, f, pts = classes(real)["torus"]
    rng = np.random.default_rng(10)
    v1 = (v + rng.normal(scale=0.3, size=v.shape)).astype(real)
    a = BVHAccel(real)
    assert a.Build(f.shape[0], MotionTriangleMesh(v, v1, f))
    normals = a.FeatureNormals()
    assert same_bytes(normals[0], sf.model_normals(v, f)[0])
    cf.assert_same(*a.SignedDistanceBatch(pts), *sf.brute(v, f, normals, pts), what="motion context")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_staleness(real, device):
    """nrtRefit to vertices that turn the cube inside out (one axis mirrored): every sign flips and the normals are the model's for
    the new vertices; nrtBuild alone changes nothing; nrtSetMesh of another class answers for that class."""
    import torch

    v, f, pts = classes(real)["cube"]
    ok = sf.checked(real, "cube")
    a = built(real, v, f)
    before, found = a.SignedDistanceBatch(pts)
    n0 = a.FeatureNormals()
    assert a.BuildCurrent()
    after_build, _ = a.SignedDistanceBatch(pts)
    assert same_bytes(before, after_build) and all(same_bytes(x, y) for x, y in zip(n0, a.FeatureNormals()))
    mirrored = (v * np.asarray([-1, 1, 1], dtype=real)).astype(real)
    if device:
        d_v = torch.from_numpy(mirrored.copy()).cuda()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        a.RefitDevice(d_v, stream=s)  # (the signed query behind it waits for the refit)
    else:
        a.Refit(mirrored)
    mpts = pts.copy()
    mpts["p"][:, 0] = -pts["p"][:, 0]
    flipped, found2 = a.SignedDistanceBatch(mpts)
    n1 = a.FeatureNormals()
    assert_library_normals(real, "cube, mirrored", mirrored, f, n1)
    cf.assert_same(flipped, found2, *sf.brute(mirrored, f, n1, mpts), what="after the refit")
    assert found.all() and found2.all()
    assert (sf.inside_bits(flipped)[ok] != sf.inside_bits(before)[ok]).all(), "a sign did not flip"
    v2, f2, pts2 = classes(real)["wedge"]
    assert a.Build(f2.shape[0], TriangleMesh(v2, f2))
    n2 = a.FeatureNormals()
    assert_library_normals(real, "wedge", v2, f2, n2)
    cf.assert_same(*a.SignedDistanceBatch(pts2), *sf.brute(v2, f2, n2, pts2), what="after SetMesh of the wedge")


def test_host_form_past_one_piece_of_its_loop():
    src = open(os.path.join(ROOT, "nanort_amd", "csrc", "api_query.hip")).read()
    piece = 1 << int(re.search(r"kClosestPiece = 1ull << (\d+);", src).group(1))
    n = piece + 777
    real = np.float32
    v, f, base = classes(real)["torus"]
    a = built(real, v, f)
    normals = a.FeatureNormals()
    ref_out, ref_found = sf.brute(v, f, normals, base)
    reps = -(-n // base.shape[0])
    out, found = a.SignedDistanceBatch(np.tile(base, reps)[:n])
    assert np.array_equal(found, np.tile(ref_found, reps)[:n]) and out.tobytes() == np.tile(ref_out, reps)[:n].tobytes()


# ---- refusals: the status, and nothing written ---------------------------------------------------------------------------------------
def _refused(a, real, status, fill=0xA5):
    import torch

    n = 130
    pts = cf.make_points(real, np.zeros((n, 3)), np.inf)
    rd = signed_dtype(real)
    out = np.full((n * rd.itemsize,), fill, dtype=np.uint8)
    found = np.full((n,), fill, dtype=np.uint8)
    s = "f32" if np.dtype(real) == np.float32 else "f64"
    assert getattr(a._L, "nrtSignedDistanceBatch_" + s)(a._h, pts.ctypes.data, n, None, out.ctypes.data, found.ctypes.data) == status
    assert (out == fill).all() and (found == fill).all()
    d_pts = to_device(pts)
    d_out = torch.full((n * rd.itemsize,), fill, dtype=torch.uint8, device="cuda")
    d_found = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    dev = getattr(a._L, "nrtSignedDistanceBatchDevice_" + s)
    assert dev(a._h, d_pts.data_ptr(), n, None, d_out.data_ptr(), d_found.data_ptr(), torch.cuda.current_stream().cuda_stream) == status
    torch.cuda.synchronize()
    assert bool((d_out == fill).all()) and bool((d_found == fill).all())


def test_refusals():
    import torch

    real = np.float32
    v, f, pts = classes(real)["wedge"]
    spheres = BVHAccel(np.float32)
    g = SphereGeometry(*scenes.random_spheres(300))
    assert spheres.Build(g.num_faces, g)
    _refused(spheres, np.float32, NRT_ERR_INVALID)
    assert "triangle contexts only" in spheres._L.nrtLastError(spheres._h).decode()
    keep = np.full((12,), 7, dtype=np.float32)
    assert spheres._L.nrtGetFeatureNormals_f32(spheres._h, keep.ctypes.data, keep.ctypes.data) == NRT_ERR_INVALID and (keep == 7).all()
    a = built(real, v, f)
    _refused(a, np.float64, NRT_ERR_PRECISION)
    assert a._L.nrtGetFeatureNormals_f64(a._h, keep.ctypes.data, None) == NRT_ERR_PRECISION and (keep == 7).all()
    no_tree = BVHAccel(real)
    no_tree.SetMesh(TriangleMesh(v, f))
    _refused(no_tree, real, NRT_ERR_INVALID)
    assert "no tree" in no_tree._L.nrtLastError(no_tree._h).decode()
    empty = BVHAccel(real)
    assert empty._L.nrtGetFeatureNormals_f32(empty._h, keep.ctypes.data, None) != NRT_OK and (keep == 7).all()
    with pytest.raises(NrtError) as e:
        no_tree.SignedDistanceBatch(np.zeros((4, 3), dtype=np.float32))
    assert e.value.status == NRT_ERR_INVALID
    host, dev = a._L.nrtSignedDistanceBatch_f32, a._L.nrtSignedDistanceBatchDevice_f32
    p = np.ascontiguousarray(pts[:130])
    out = np.zeros((130,), dtype=signed_dtype(real))
    keep_out = out.tobytes()
    assert host(a._h, None, 130, None, out.ctypes.data, None) == NRT_ERR_INVALID
    assert host(a._h, p.ctypes.data, 130, None, None, None) == NRT_ERR_INVALID
    assert host(a._h, p.ctypes.data, 1 << 31, None, out.ctypes.data, None) == NRT_ERR_INVALID
    assert out.tobytes() == keep_out
    stream = torch.cuda.current_stream().cuda_stream
    assert host(a._h, None, 0, None, None, None) == NRT_OK and dev(a._h, None, 0, None, None, None, stream) == NRT_OK
    d_pts = to_device(np.concatenate([p, p[:1]]))
    d_out = torch.full((131 * 32,), 0x5A, dtype=torch.uint8, device="cuda")
    assert dev(a._h, d_pts.data_ptr() + 4, 130, None, d_out.data_ptr(), None, stream) == NRT_ERR_INVALID
    assert dev(a._h, d_pts.data_ptr(), 130, None, d_out.data_ptr() + 4, None, stream) == NRT_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((d_out == 0x5A).all())
    assert host(a._h, p.ctypes.data, 130, None, out.ctypes.data, None) == NRT_OK  # (found_out may be NULL)
    assert out.tobytes() == sf.brute(v, f, a.FeatureNormals(), p)[0].tobytes()
    # either pointer of nrtGetFeatureNormals may be NULL
    fn = np.zeros((f.shape[0], 4, 3), dtype=real)
    vn = np.zeros((v.shape[0], 3), dtype=real)
    assert a._L.nrtGetFeatureNormals_f32(a._h, fn.ctypes.data, None) == NRT_OK and a._L.nrtGetFeatureNormals_f32(a._h, None, vn.ctypes.data) == NRT_OK
    both = a.FeatureNormals()
    assert same_bytes(fn, both[0]) and same_bytes(vn, both[1])

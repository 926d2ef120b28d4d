"""nrtClosestPointBatch* on the GPU: byte-identical records and found bytes against the model's brute force over the faces
(tests/closest_fixture.py, tests/closest_model.cc), in fp32 and fp64; on the hostile meshes also within the accuracy envelope of the
fixture's long-double reference."""
import os
import re

import numpy as np
import pytest

import closest_fixture as cf
from nanort_amd import BVHAccel, TriangleMesh, scenes
from nanort_amd.accel import CurveGeometry, CylinderGeometry, MotionTriangleMesh, SphereGeometry
from nanort_amd.capi import NRT_ERR_INVALID, NRT_ERR_PRECISION, NRT_OK, NrtError
from nanort_amd.wire import closest_dtype, point_dtype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REALS = [np.float32, np.float64]
IDS = ["f32", "f64"]


def built(real, v, f):
    a = BVHAccel(real)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    return a


def to_device(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def device_query(a, pts, opts=None, stream=None, fill=0):
    """The Device form over `pts`; returns the output tensors (nothing synchronised)."""
    import torch

    n = pts.shape[0]
    d_pts = to_device(pts)
    d_out = torch.full((n * closest_dtype(a.real).itemsize,), fill, dtype=torch.uint8, device="cuda")
    d_found = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    a.ClosestPointBatchDevice(d_pts, d_out, d_found, options=cf.trace_options(opts), stream=stream)
    return d_pts, d_out, d_found


def from_device(real, d_out, d_found):
    return d_out.cpu().numpy().view(closest_dtype(real)), d_found.cpu().numpy()


@pytest.fixture(scope="module", params=REALS, ids=IDS)
def c1(request):
    real = request.param
    v, f = cf.mesh(real)
    return real, v, f, built(real, v, f)


@pytest.mark.parametrize("name", cf.SET_NAMES)
def test_every_set_host_form(c1, name):
    real, v, f, a = c1
    out, found = a.ClosestPointBatch(cf.point_sets(real)[name])
    cf.assert_same(out, found, *cf.expected(real, name), what="set %s" % name)
    assert a.LastKernelName() == "nrt::k_closest_point<%s, 32>" % ("float" if real == np.float32 else "double")
    assert not out["_pad"].any()


@pytest.mark.parametrize("name", cf.SET_NAMES)
def test_every_set_device_form_on_a_stream_then_a_rebuild(c1, name):
    """The Device form on a non-default stream, then BuildCurrent on the same context with no synchronisation of the caller's own:
    the rebuild waits for the launch (it took a launch slot)."""
    import torch

    real, v, f, a = c1
    s = torch.cuda.Stream()
    _, d_out, d_found = device_query(a, cf.point_sets(real)[name], stream=s)
    assert a.BuildCurrent()
    s.synchronize()
    out, found = from_device(real, d_out, d_found)
    cf.assert_same(out, found, *cf.expected(real, name), what="set %s" % name)


@pytest.mark.parametrize("oname", ["range", "skip", "both"])
def test_options(c1, oname):
    real, v, f, a = c1
    opts = cf.option_cases(real)[oname]
    for name in ("a", "b", "c"):
        out, found = a.ClosestPointBatch(cf.point_sets(real)[name], options=cf.trace_options(opts))
        cf.assert_same(out, found, *cf.expected(real, name, opts), what="set %s, options %s" % (name, oname))
    _, d_out, d_found = device_query(a, cf.point_sets(real)["b"], opts)
    cf.assert_same(*from_device(real, d_out, d_found), *cf.expected(real, "b", opts), what="set b, Device form, options %s" % oname)


def test_max_dist_as_a_scalar_and_per_point(c1):
    real, v, f, a = c1
    pts = cf.point_sets(real)["b"]
    out, found = a.ClosestPointBatch(pts["p"], max_dist=pts["max_dist"])
    cf.assert_same(out, found, *cf.expected(real, "b"), what="per-point max_dist")
    out, found = a.ClosestPointBatch(pts["p"][:200])
    assert found[np.isfinite(pts["p"][:200]).all(axis=1)].all()
    ref = cf.brute(v, f, cf.make_points(real, pts["p"][:200], np.inf))
    cf.assert_same(out, found, *ref, what="max_dist = inf")


@pytest.mark.parametrize("real", REALS, ids=IDS)
@pytest.mark.parametrize("nf", [1, 2])
def test_tiny_trees(real, nf):
    """One triangle (the root is a leaf) and two."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], dtype=real)
    f = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.uint32)[:nf]
    a = built(real, v, f)
    rng = np.random.default_rng(3)
    xyz = np.concatenate([rng.uniform(-1, 2, size=(190, 3)), v.astype(np.float64), [[0.5, 0.5, 0.0], [0.5, 0.5, 0.25]]])
    md = np.where(np.arange(xyz.shape[0]) % 3 == 0, 0.4, np.inf)
    pts = cf.make_points(real, xyz, md)
    out, found = a.ClosestPointBatch(pts)
    cf.assert_same(out, found, *cf.brute(v, f, pts), what="%d triangle(s)" % nf)
    assert 0 < found.sum() < found.shape[0]


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_deep_adopted_tree_spills_past_the_lds_stack(oracle, real):
    """The reference's own tree on a grid mesh is deeper than the 32 LDS entries of a lane's stack.  Points far from the mesh with
    max_dist = inf: nothing is culled before the first leaf is reached, so the first descent leaves a sibling waiting at every level
    and the stack goes on in the overflow area (the model's walk counts 102 entries waiting at once)."""
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
    ref_out, ref_found = cf.brute(v, f, pts)
    w_out, w_found, _, deepest = cf.walk(nodes, idx, v, f, pts, count=True)
    cf.assert_same(w_out, w_found, ref_out, ref_found, what="the model's walk")
    assert deepest > 33, "fixture no longer exercises the overflow area"
    out, found = a.ClosestPointBatch(pts)
    cf.assert_same(out, found, ref_out, ref_found, what="deep tree")
    assert found.all()


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_refit_to_moved_vertices(real):
    v, f = cf.mesh(real)
    a = built(real, v, f)
    rng = np.random.default_rng(9)
    moved = (v + rng.normal(scale=0.05, size=v.shape)).astype(real)
    a.Refit(moved)
    for name in ("a", "c"):
        pts = cf.point_sets(real)[name]
        out, found = a.ClosestPointBatch(pts)
        cf.assert_same(out, found, *cf.brute(moved, f, pts), what="set %s after Refit" % name)


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_motion_context_answers_for_keyframe_0(real):
    v, f = cf.mesh(real)
    rng = np.random.default_rng(10)
    v1 = (v + rng.normal(scale=0.3, size=v.shape)).astype(real)
    a = BVHAccel(real)
    assert a.Build(f.shape[0], MotionTriangleMesh(v, v1, f))
    for name in ("a", "b"):
        out, found = a.ClosestPointBatch(cf.point_sets(real)[name])
        cf.assert_same(out, found, *cf.expected(real, name), what="set %s, motion context" % name)


# ---- accuracy on hostile meshes: byte-equal to brute force AND within the envelope of the long-double reference ------------------------
@pytest.mark.parametrize("name", cf.HOSTILE_NAMES)
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_hostile_classes_built_tree(real, name):
    """Build over every hostile class (tests/closest_fixture.py: slivers, needles, specks, collinear and repeated faces, far and
    offset points, points near the faces), then the query: the model's brute force byte for byte, and cf.assert_within_envelope.
    `mixed` goes through the Device form."""
    cf.require_reference()
    v, f, pts = cf.hostile_classes(real)[name]
    a = built(real, v, f)
    if name == "mixed":
        _, d_out, d_found = device_query(a, pts)
        out, found = from_device(real, d_out, d_found)
    else:
        out, found = a.ClosestPointBatch(pts)
    what = "%s, %s" % (IDS[REALS.index(real)], name)
    cf.assert_same(out, found, *cf.hostile_brute(real, name), what=what)
    cf.assert_within_envelope(real, v, f, pts, out, found, what, d_true=cf.hostile_reference(real, name))


@pytest.mark.parametrize("tree", ["default", "deep_leaves"])
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_hostile_mixed_adopted_trees(real, tree):
    """SetTree with the reference-built trees of `mixed` — the default build, and min_leaf = 16 with max_depth = 3, whose leaves
    hold more than 16 records (cf.mixed_trees asserts it) — under the class's radii (+inf and finite by turns), then a
    prim_ids_range and a skip_prim_id case on the first 999 points, the reference restricted to the admitted faces."""
    cf.require_reference()
    v, f, pts = cf.hostile_classes(real)["mixed"]
    nodes, idx = cf.mixed_trees(real)[tree]
    a = BVHAccel(real)
    a.SetMesh(TriangleMesh(v, f))
    a.SetTree(nodes, idx)
    what = "%s, mixed, %s tree" % (IDS[REALS.index(real)], tree)
    ref_out, ref_found = cf.hostile_brute(real, "mixed")
    out, found = a.ClosestPointBatch(pts)
    cf.assert_same(out, found, ref_out, ref_found, what=what)
    cf.assert_within_envelope(real, v, f, pts, out, found, what, d_true=cf.hostile_reference(real, "mixed"))
    some = pts[:999]
    busiest = int(np.bincount(ref_out["prim_id"][:999][ref_found[:999] != 0]).argmax())
    for oname, opts in (("range", cf.middle_third(f.shape[0])), ("skip", (0, 0x7FFFFFFF, busiest))):
        exp_out, exp_found = cf.brute(v, f, some, opts)
        assert exp_out.tobytes() != ref_out[:999].tobytes(), "the %s case changes no answer" % oname
        out, found = a.ClosestPointBatch(some, options=cf.trace_options(opts))
        cf.assert_same(out, found, exp_out, exp_found, what="%s, options %s" % (what, oname))
        cf.assert_within_envelope(real, v, f, some, out, found, "%s, options %s" % (what, oname), opts=opts)


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_refit_collapses_faces_into_slivers(real):
    """Refit of `blob` to vertices that put the third corner of every third face within a rounding or so of its first edge."""
    cf.require_reference()
    v, f, pts = cf.hostile_classes(real)["blob"]
    a = built(real, v, f)
    rng = np.random.default_rng(12)
    third = np.arange(0, f.shape[0], 3)
    moved = v.copy()
    A, B = moved[f[third, 0]], moved[f[third, 1]]
    s = rng.uniform(0.1, 0.9, size=(third.shape[0], 1)).astype(real)
    moved[f[third, 2]] = (A + s * (B - A)) + np.dtype(real).type(np.finfo(real).eps) * rng.uniform(-1.0, 1.0, size=A.shape).astype(real)
    assert moved.dtype == np.dtype(real)
    # really slivers of about one rounding, by long double alone: the third corner's height over the first edge
    ld = cf.LD
    ab, ac = (B.astype(ld) - A.astype(ld)), (moved[f[third, 2]].astype(ld) - A.astype(ld))
    height = np.sqrt((cf._cross(ab, ac) ** 2).sum(-1) / (ab * ab).sum(-1))
    assert (height <= 4 * np.finfo(real).eps).all() and (height > 0).sum() >= 0.9 * third.shape[0]
    a.Refit(moved)
    some = pts[:1499]
    out, found = a.ClosestPointBatch(some)
    what = "%s, blob after a collapsing Refit" % IDS[REALS.index(real)]
    cf.assert_same(out, found, *cf.brute(moved, f, some), what=what)
    cf.assert_within_envelope(real, moved, f, some, out, found, what)


def _tiled(real, n):
    base = np.concatenate([cf.point_sets(real)[k] for k in cf.SET_NAMES])
    ref_out = np.concatenate([cf.expected(real, k)[0] for k in cf.SET_NAMES])
    ref_found = np.concatenate([cf.expected(real, k)[1] for k in cf.SET_NAMES])
    reps = -(-n // base.shape[0])
    return np.tile(base, reps)[:n], np.tile(ref_out, reps)[:n], np.tile(ref_found, reps)[:n]


def test_host_form_past_one_piece_of_its_loop():
    """The host form stages kClosestPiece points per launch: a batch of one piece and a ragged second one, which is also more
    points than one trip of the persistent grid has threads (at most 8 blocks of 256 on each of 256 CUs)."""
    src = open(os.path.join(ROOT, "nanort_amd", "csrc", "api_query.hip")).read()
    piece = 1 << int(re.search(r"kClosestPiece = 1ull << (\d+);", src).group(1))
    n = piece + 777
    assert n > 256 * 8 * 256
    real = np.float32
    v, f = cf.mesh(real)
    a = built(real, v, f)
    pts, ref_out, ref_found = _tiled(real, n)
    out, found = a.ClosestPointBatch(pts)
    assert np.array_equal(found, ref_found) and out.tobytes() == ref_out.tobytes()


def test_device_form_past_one_trip_of_the_grid_fp64():
    n = 256 * 8 * 256 + 4321  # more points than the persistent grid can have threads: every lane is refilled
    real = np.float64
    v, f = cf.mesh(real)
    a = built(real, v, f)
    pts, ref_out, ref_found = _tiled(real, n)
    _, d_out, d_found = device_query(a, pts)
    out, found = from_device(real, d_out, d_found)
    assert np.array_equal(found, ref_found) and out.tobytes() == ref_out.tobytes()


# ---- refusals: the status, and nothing written ---------------------------------------------------------------------------------------
def _refused(a, real, status, fill=0xA5):
    """Both forms of the query are refused with `status` on accel `a` (its records of precision `real`), and the outputs stay as they were."""
    import torch

    n = 130
    pts = cf.make_points(real, np.zeros((n, 3)), np.inf)
    rd, pd = closest_dtype(real), point_dtype(real)
    out = np.full((n * rd.itemsize,), fill, dtype=np.uint8)
    found = np.full((n,), fill, dtype=np.uint8)
    s = "f32" if np.dtype(real) == np.float32 else "f64"
    host = getattr(a._L, "nrtClosestPointBatch_" + s)
    assert host(a._h, pts.ctypes.data, n, None, out.ctypes.data, found.ctypes.data) == status
    assert (out == fill).all() and (found == fill).all()
    d_pts = to_device(pts)
    d_out = torch.full((n * rd.itemsize,), fill, dtype=torch.uint8, device="cuda")
    d_found = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    dev = getattr(a._L, "nrtClosestPointBatchDevice_" + s)
    assert dev(a._h, d_pts.data_ptr(), n, None, d_out.data_ptr(), d_found.data_ptr(), torch.cuda.current_stream().cuda_stream) == status
    torch.cuda.synchronize()
    assert bool((d_out == fill).all()) and bool((d_found == fill).all())
    assert pd.itemsize * n == d_pts.numel()


@pytest.mark.parametrize("kind", ["spheres", "cylinders", "curves"])
def test_refused_on_other_primitive_kinds(kind):
    a = BVHAccel(np.float32)
    if kind == "spheres":
        g = SphereGeometry(*scenes.random_spheres(300))
    elif kind == "cylinders":
        g = CylinderGeometry(*scenes.random_cylinders(300))
    else:
        g = CurveGeometry(*scenes.synthetic_hair(300))
    assert a.Build(g.num_faces, g)
    _refused(a, np.float32, NRT_ERR_INVALID)
    assert "triangle contexts only" in a._L.nrtLastError(a._h).decode()


def test_refused_for_the_other_precision(c1):
    real, v, f, a = c1
    other = np.float64 if real == np.float32 else np.float32
    _refused(a, other, NRT_ERR_PRECISION)


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_refused_without_a_tree(real):
    v, f = cf.mesh(real)
    a = BVHAccel(real)
    a.SetMesh(TriangleMesh(v, f))
    _refused(a, real, NRT_ERR_INVALID)
    assert "no tree" in a._L.nrtLastError(a._h).decode()


def test_null_arguments_misalignment_and_zero_points(c1):
    import torch

    real, v, f, a = c1
    s = "f32" if real == np.float32 else "f64"
    host, dev = getattr(a._L, "nrtClosestPointBatch_" + s), getattr(a._L, "nrtClosestPointBatchDevice_" + s)
    pts = cf.point_sets(real)["b"][:130]
    out = np.full((130,), 0, dtype=closest_dtype(real))
    keep = out.tobytes()
    assert host(a._h, None, 130, None, out.ctypes.data, None) == NRT_ERR_INVALID
    assert host(a._h, pts.ctypes.data, 130, None, None, None) == NRT_ERR_INVALID
    assert host(a._h, pts.ctypes.data, 1 << 31, None, out.ctypes.data, None) == NRT_ERR_INVALID
    assert out.tobytes() == keep
    assert host(a._h, None, 0, None, None, None) == NRT_OK
    stream = torch.cuda.current_stream().cuda_stream
    assert dev(a._h, None, 0, None, None, None, stream) == NRT_OK
    d_pts = to_device(np.concatenate([pts, pts[:1]]))
    d_out = torch.full((131 * closest_dtype(real).itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    assert dev(a._h, d_pts.data_ptr() + 4, 130, None, d_out.data_ptr(), None, stream) == NRT_ERR_INVALID  # (off by one float)
    assert dev(a._h, d_pts.data_ptr(), 130, None, d_out.data_ptr() + 4, None, stream) == NRT_ERR_INVALID
    assert "aligned" in a._L.nrtLastError(a._h).decode()
    torch.cuda.synchronize()
    assert bool((d_out == 0x5A).all())
    # found_out may be NULL
    assert host(a._h, pts.ctypes.data, 130, None, out.ctypes.data, None) == NRT_OK
    assert out.tobytes() == cf.brute(v, f, pts)[0].tobytes()


def test_cpu_tensor_given_to_the_device_form(c1):
    import torch

    real, v, f, a = c1
    pts = cf.point_sets(real)["b"][:130]
    cpu_pts = torch.from_numpy(pts.view(np.uint8).copy())
    d_out = torch.full((130 * closest_dtype(real).itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        a.ClosestPointBatchDevice(cpu_pts, d_out)
    with pytest.raises(ValueError):
        a.ClosestPointBatchDevice(to_device(pts), torch.zeros((130 * closest_dtype(real).itemsize,), dtype=torch.uint8))
    torch.cuda.synchronize()
    assert bool((d_out == 0x5A).all())


def test_python_raises_the_library_status():
    a = BVHAccel(np.float32)
    a.SetMesh(TriangleMesh(*cf.mesh(np.float32)))  # (no tree)
    with pytest.raises(NrtError) as e:
        a.ClosestPointBatch(np.zeros((4, 3), dtype=np.float32))
    assert e.value.status == NRT_ERR_INVALID

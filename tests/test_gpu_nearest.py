"""nrtNearestFacesBatch* on the GPU: rows and counts byte-identical to the model's brute force over the faces with the K-buffer
(tests/nearest_fixture.py, tests/nearest_model.cc), in fp32 and fp64."""
import numpy as np
import pytest

import closest_fixture as cf
import nearest_fixture as nf
from nanort_amd import BVHAccel, TriangleMesh, scenes
from nanort_amd.accel import CurveGeometry, CylinderGeometry, MotionTriangleMesh, SphereGeometry
from nanort_amd.capi import NRT_ERR_INVALID, NRT_ERR_PRECISION, NRT_MAX_NEAREST, NRT_OK, NrtError
from nanort_amd.wire import closest_dtype, point_dtype

pytestmark = pytest.mark.gpu

REALS = [np.float32, np.float64]
IDS = ["f32", "f64"]


def built(real, v, f):
    a = BVHAccel(real)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    return a


def adopted(real, v, f, nodes, idx):
    a = BVHAccel(real)
    a.SetMesh(TriangleMesh(v, f))
    a.SetTree(nodes, idx)
    return a


def to_device(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def device_query(a, pts, k, opts=None, stream=None, fill=0xA5):
    """The Device form over `pts`; returns the output tensors (nothing synchronised)."""
    import torch

    n = pts.shape[0]
    d_pts = to_device(pts)
    d_out = torch.full((n * k * closest_dtype(a.real).itemsize,), fill, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((4 * n,), fill, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    assert a.NearestFacesBatchDevice(d_pts, k, d_out, d_counts, options=cf.trace_options(opts), stream=stream) == n
    return d_pts, d_out, d_counts


def from_device(real, k, d_out, d_counts):
    return d_out.cpu().numpy().view(closest_dtype(real)).reshape(-1, k), d_counts.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module", params=REALS, ids=IDS)
def c1(request):
    real = request.param
    v, f = cf.mesh(real)
    return real, v, f, built(real, v, f)


@pytest.mark.parametrize("real", REALS, ids=IDS)
@pytest.mark.parametrize("nfaces,k", [(1, 1), (1, 2), (2, 1), (2, 2), (2, 3)])
def test_tiny_trees(real, nfaces, k):
    """One triangle (the root is a leaf) and two, with fewer, as many and more slots than faces."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], dtype=real)
    f = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.uint32)[:nfaces]
    a = built(real, v, f)
    rng = np.random.default_rng(3)
    xyz = np.concatenate([rng.uniform(-1, 2, size=(190, 3)), v.astype(np.float64), [[0.5, 0.5, 0.0], [0.5, 0.5, 0.25]]])
    md = np.where(np.arange(xyz.shape[0]) % 3 == 0, 0.4, np.inf)
    pts = cf.make_points(real, xyz, md)
    out, counts = a.NearestFacesBatch(pts, k)
    nf.assert_same(out, counts, *nf.brute(v, f, pts, k), what="%d triangle(s), K = %d" % (nfaces, k))
    assert counts.max() == min(k, nfaces) and counts.min() == 0


@pytest.mark.parametrize("radii", [False, True], ids=["inf", "radii"])
@pytest.mark.parametrize("k", nf.KS)
def test_every_set_host_form(c1, k, radii):
    real, v, f, a = c1
    for name in nf.SET_NAMES:
        out, counts = a.NearestFacesBatch(nf.point_sets(real, k if radii else None)[name], k)
        nf.assert_same(out, counts, *nf.expected(real, name, k, radii), what="set %s, K = %d" % (name, k))
        assert not out["_pad"].any()
    assert a.LastKernelName() == "nrt::k_nearest_faces<%s, 32>" % ("float" if real == np.float32 else "double")


@pytest.mark.parametrize("radii", [False, True], ids=["inf", "radii"])
@pytest.mark.parametrize("k", nf.KS)
def test_every_set_device_form_on_a_stream_then_a_rebuild(c1, k, radii):
    """The Device form on a non-default stream, then BuildCurrent on the same context with no synchronisation of the caller's own:
    the rebuild waits for the launches (each took a launch slot)."""
    import torch

    real, v, f, a = c1
    s = torch.cuda.Stream()
    res = [device_query(a, nf.point_sets(real, k if radii else None)[name], k, stream=s) for name in nf.SET_NAMES]
    assert a.BuildCurrent()
    s.synchronize()
    for name, (_, d_out, d_counts) in zip(nf.SET_NAMES, res):
        nf.assert_same(*from_device(real, k, d_out, d_counts), *nf.expected(real, name, k, radii), what="set %s, K = %d" % (name, k))


def test_k1_is_the_closest_point_query(c1):
    """K = 1 against nrtClosestPointBatch's own output, under closest_fixture's radii."""
    real, v, f, a = c1
    for name in nf.SET_NAMES:
        pts = cf.point_sets(real)[name]
        out, counts = a.NearestFacesBatch(pts, 1)
        ref_out, ref_found = a.ClosestPointBatch(pts)
        assert out[:, 0].tobytes() == ref_out.tobytes() and np.array_equal(counts, ref_found.astype(np.uint32)), "set %s" % name


def test_options(c1):
    """A range of 5 faces with K = 7 (count == 5 wherever anything is looked at), a skip id, and both together."""
    real, v, f, a = c1
    pts = nf.point_sets(real)["a"]
    r0 = f.shape[0] // 2
    skip = cf.busiest_face(real)
    base = nf.expected(real, "a", 7, False)[0]
    for what, opts, count in (("range", (r0, r0 + 5, 0xFFFFFFFF), 5), ("skip", (0, 0x7FFFFFFF, skip), 7), ("both", (r0, r0 + 5, r0 + 2), 4)):
        ref_out, ref_counts = nf.brute(v, f, pts, 7, opts)
        assert (ref_counts[nf.searchable(pts)] == count).all() and ref_out.tobytes() != base.tobytes()
        out, counts = a.NearestFacesBatch(pts, 7, options=cf.trace_options(opts))
        nf.assert_same(out, counts, ref_out, ref_counts, what="options %s" % what)
        _, d_out, d_counts = device_query(a, pts, 7, opts)
        nf.assert_same(*from_device(real, 7, d_out, d_counts), ref_out, ref_counts, what="Device form, options %s" % what)
    for oname, opts in nf.restrictions(real).items():
        out, counts = a.NearestFacesBatch(nf.point_sets(real)["b"], 4, options=cf.trace_options(opts))
        nf.assert_same(out, counts, *nf.expected(real, "b", 4, False, opts), what="set b, K = 4, %s" % oname)


def test_max_dist_as_a_scalar_and_counts_left_out(c1):
    import torch

    real, v, f, a = c1
    pts = nf.point_sets(real, 4)["b"]
    out, counts = a.NearestFacesBatch(pts["p"], 4, max_dist=pts["max_dist"])
    nf.assert_same(out, counts, *nf.expected(real, "b", 4, True), what="per-point max_dist")
    out, counts = a.NearestFacesBatch(pts["p"][:200], 4)
    nf.assert_same(out, counts, *nf.brute(v, f, cf.make_points(real, pts["p"][:200], np.inf), 4), what="max_dist = inf")
    d_out = torch.zeros((pts.shape[0] * 4 * closest_dtype(real).itemsize,), dtype=torch.uint8, device="cuda")
    a.NearestFacesBatchDevice(to_device(pts), 4, d_out)  # (counts_out may be NULL)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == nf.expected(real, "b", 4, True)[0].tobytes()


@pytest.mark.parametrize("k", [2, 64])
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_hostile_duplicates(real, k):
    cf.require_reference()
    v, f, pts = cf.hostile_classes(real)["duplicates"]
    out, counts = built(real, v, f).NearestFacesBatch(pts, k)
    nf.assert_same(out, counts, *nf.brute(v, f, pts, k), what="duplicates, K = %d" % k)


@pytest.mark.parametrize("tree", ["default", "deep_leaves"])
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_hostile_mixed_adopted_trees(real, tree):
    """SetTree with the reference-built trees of `mixed`; `deep_leaves` has a leaf of more records than any K."""
    cf.require_reference()
    v, f, pts = cf.hostile_classes(real)["mixed"]
    a = adopted(real, v, f, *cf.mixed_trees(real)[tree])
    for k in (2, 64):
        out, counts = a.NearestFacesBatch(pts, k)
        nf.assert_same(out, counts, *nf.brute(v, f, pts, k), what="mixed, %s tree, K = %d" % (tree, k))


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_deep_adopted_tree_spills_past_the_lds_stack(oracle, real):
    """The reference's own tree on a grid mesh is deeper than the 32 LDS entries of a lane's stack (test_gpu_closest.py has the same
    mesh and points): with K = 4 and max_dist = inf the model's walk has more than 33 entries waiting at once."""
    v32, f = scenes.plane(300, 150)
    v = v32.astype(real)
    nodes, idx, st = oracle.build(v, f)
    assert st["max_tree_depth"] > 40
    a = adopted(real, v, f, nodes, idx)
    rng = np.random.default_rng(11)
    c = 0.5 * (v32.min(0) + v32.max(0)).astype(np.float64)
    ext = float(np.linalg.norm(v32.max(0) - v32.min(0)))
    d = rng.normal(size=(150, 3))
    far = c + d / np.linalg.norm(d, axis=1)[:, None] * ext * rng.uniform(20, 60, size=(150, 1))
    near = c + rng.uniform(-0.5, 0.5, size=(50, 3)) * ext
    pts = cf.make_points(real, np.concatenate([far, near]), np.inf)
    ref_out, ref_counts = nf.brute(v, f, pts, 4)
    w_out, w_counts, _, deepest = nf.walk(nodes, idx, v, f, pts, 4, count=True)
    nf.assert_same(w_out, w_counts, ref_out, ref_counts, what="the model's walk")
    assert deepest > 33, "fixture no longer exercises the overflow area"
    out, counts = a.NearestFacesBatch(pts, 4)
    nf.assert_same(out, counts, ref_out, ref_counts, what="deep tree")
    assert (counts == 4).all()


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_refit_to_moved_vertices(real):
    v, f = cf.mesh(real)
    a = built(real, v, f)
    rng = np.random.default_rng(9)
    moved = (v + rng.normal(scale=0.05, size=v.shape)).astype(real)
    a.Refit(moved)
    for name, k in (("a", 4), ("c", 7)):
        pts = nf.point_sets(real, k)[name]
        out, counts = a.NearestFacesBatch(pts, k)
        nf.assert_same(out, counts, *nf.brute(moved, f, pts, k), what="set %s after Refit" % name)


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_motion_context_answers_for_keyframe_0(real):
    v, f = cf.mesh(real)
    rng = np.random.default_rng(10)
    v1 = (v + rng.normal(scale=0.3, size=v.shape)).astype(real)
    a = BVHAccel(real)
    assert a.Build(f.shape[0], MotionTriangleMesh(v, v1, f))
    for name in ("a", "b"):
        out, counts = a.NearestFacesBatch(nf.point_sets(real, 4)[name], 4)
        nf.assert_same(out, counts, *nf.expected(real, name, 4, True), what="set %s, motion context" % name)


@pytest.mark.parametrize("k,n", [(3, 349525 + 777), (64, 16384 + 777)])
def test_host_form_past_one_piece_of_its_loop(c1, k, n):
    """The host form stages max(1, 2^20 / K) points per launch: one whole piece and a ragged second one."""
    real, v, f, a = c1
    assert n == (1 << 20) // k + 777
    pts, ref_out, ref_counts = nf.tiled(real, k, n)
    out, counts = a.NearestFacesBatch(pts, k)
    assert np.array_equal(counts, ref_counts) and out.tobytes() == ref_out.tobytes()


def test_device_form_past_one_trip_of_the_grid_fp64():
    n = 256 * 8 * 256 + 4321  # more points than the persistent grid can have threads: every lane is refilled
    assert n == 528609
    real = np.float64
    v, f = cf.mesh(real)
    a = built(real, v, f)
    pts, ref_out, ref_counts = nf.tiled(real, 2, n)
    _, d_out, d_counts = device_query(a, pts, 2)
    out, counts = from_device(real, 2, d_out, d_counts)
    assert np.array_equal(counts, ref_counts) and out.tobytes() == ref_out.tobytes()


# ---- refusals: the status, and nothing written ---------------------------------------------------------------------------------------
def _refused(a, real, status, k=4, fill=0xA5):
    """Both forms of the query are refused with `status` on accel `a` (records of precision `real`), and the rows and counts stay as
    they were."""
    import torch

    n = 130
    rows = max(1, min(k, 70))
    pts = cf.make_points(real, np.zeros((n, 3)), np.inf)
    rd = closest_dtype(real)
    out = np.full((n * rows * rd.itemsize,), fill, dtype=np.uint8)
    counts = np.full((4 * n,), fill, dtype=np.uint8)
    s = "f32" if np.dtype(real) == np.float32 else "f64"
    host = getattr(a._L, "nrtNearestFacesBatch_" + s)
    assert host(a._h, pts.ctypes.data, n, k, None, out.ctypes.data, counts.ctypes.data) == status
    assert (out == fill).all() and (counts == fill).all()
    d_pts = to_device(pts)
    d_out = torch.full((n * rows * rd.itemsize,), fill, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((4 * n,), fill, dtype=torch.uint8, device="cuda")
    dev = getattr(a._L, "nrtNearestFacesBatchDevice_" + s)
    assert dev(a._h, d_pts.data_ptr(), n, k, None, d_out.data_ptr(), d_counts.data_ptr(), torch.cuda.current_stream().cuda_stream) == status
    torch.cuda.synchronize()
    assert bool((d_out == fill).all()) and bool((d_counts == fill).all())
    assert point_dtype(real).itemsize * n == d_pts.numel()


@pytest.mark.parametrize("k", [0, NRT_MAX_NEAREST + 1, 0xFFFFFFFF])
def test_refused_for_a_k_outside_its_range(c1, k):
    real, v, f, a = c1
    _refused(a, real, NRT_ERR_INVALID, k=k)
    assert "max_faces" in a._L.nrtLastError(a._h).decode()
    with pytest.raises(NrtError):
        a.NearestFacesBatch(np.zeros((4, 3), dtype=real), k)


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
    host, dev = getattr(a._L, "nrtNearestFacesBatch_" + s), getattr(a._L, "nrtNearestFacesBatchDevice_" + s)
    pts = nf.point_sets(real)["b"][:130]
    out = np.full((130, 2), 0, dtype=closest_dtype(real))
    keep = out.tobytes()
    assert host(a._h, None, 130, 2, None, out.ctypes.data, None) == NRT_ERR_INVALID
    assert host(a._h, pts.ctypes.data, 130, 2, None, None, None) == NRT_ERR_INVALID
    assert host(a._h, pts.ctypes.data, 1 << 31, 2, None, out.ctypes.data, None) == NRT_ERR_INVALID
    assert out.tobytes() == keep
    assert host(a._h, None, 0, 2, None, None, None) == NRT_OK
    stream = torch.cuda.current_stream().cuda_stream
    assert dev(a._h, None, 0, 2, None, None, None, stream) == NRT_OK
    d_pts = to_device(np.concatenate([pts, pts[:1]]))
    d_out = torch.full((131 * 2 * closest_dtype(real).itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((4 * 131,), 0x5A, dtype=torch.uint8, device="cuda")
    assert dev(a._h, d_pts.data_ptr() + 4, 130, 2, None, d_out.data_ptr(), d_counts.data_ptr(), stream) == NRT_ERR_INVALID  # (off by one float)
    assert dev(a._h, d_pts.data_ptr(), 130, 2, None, d_out.data_ptr() + 4, d_counts.data_ptr(), stream) == NRT_ERR_INVALID
    assert dev(a._h, d_pts.data_ptr(), 130, 2, None, d_out.data_ptr(), d_counts.data_ptr() + 2, stream) == NRT_ERR_INVALID
    assert "aligned" in a._L.nrtLastError(a._h).decode()
    torch.cuda.synchronize()
    assert bool((d_out == 0x5A).all()) and bool((d_counts == 0x5A).all())
    # counts_out may be NULL
    assert host(a._h, pts.ctypes.data, 130, 2, None, out.ctypes.data, None) == NRT_OK
    assert out.tobytes() == nf.brute(v, f, pts, 2)[0].tobytes()


def test_cpu_tensor_given_to_the_device_form(c1):
    import torch

    real, v, f, a = c1
    pts = nf.point_sets(real)["b"][:130]
    size = 130 * 2 * closest_dtype(real).itemsize
    d_out = torch.full((size,), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        a.NearestFacesBatchDevice(torch.from_numpy(pts.view(np.uint8).copy()), 2, d_out)
    with pytest.raises(ValueError):
        a.NearestFacesBatchDevice(to_device(pts), 2, torch.zeros((size,), dtype=torch.uint8))
    with pytest.raises(ValueError):
        a.NearestFacesBatchDevice(to_device(pts), 3, d_out)  # (too few records for K = 3)
    torch.cuda.synchronize()
    assert bool((d_out == 0x5A).all())

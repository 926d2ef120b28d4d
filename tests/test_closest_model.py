"""The closest-point rule (include/nanort_closest.h) on the CPU: the bound its cull rests on, the walk against brute force on two
trees, the header's host form, an independent formulation, the accuracy envelope against a long-double reference on hostile
meshes, and the C ABI's layout and exports.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import closest_fixture as cf
from nanort_amd import capi
from nanort_amd.wire import CLOSEST_F32, CLOSEST_F64, POINT_F32, POINT_F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REALS = [np.float32, np.float64]
IDS = ["f32", "f64"]


def _bound_cases(rng, real, n):
    """n cases {p, a, b, c, bmin, bmax}: unit, 1e-3 and 1e3 scales, coordinates offset by 1000, degenerate triangles, points inside,
    near and far from the box, tight and padded boxes.  Built in the precision under test, so every box contains its vertices."""
    scale = rng.choice([1.0, 1e-3, 1e3], size=(n, 1, 1))
    offset = np.where(rng.random((n, 1, 1)) < 0.25, 1000.0, 0.0) * rng.choice([-1.0, 1.0], size=(n, 1, 1))
    tri = rng.uniform(-1.0, 1.0, size=(n, 3, 3))
    kind = rng.integers(0, 8, size=n)
    tri[kind == 0, 1] = tri[kind == 0, 0]                                 # two vertices equal
    tri[kind == 1, 2] = 0.5 * (tri[kind == 1, 0] + tri[kind == 1, 1])     # collinear
    tri[kind == 2, 1] = tri[kind == 2, 0]
    tri[kind == 2, 2] = tri[kind == 2, 0]                                 # a point
    tri[kind == 3] = np.round(tri[kind == 3] * 4) / 4                     # lattice: exact arithmetic, exact equalities
    tri = (tri * scale + offset).astype(real)
    reach = rng.choice([0.0, 0.01, 1.0, 10.0], size=(n, 1))
    p = rng.uniform(-1.0, 1.0, size=(n, 3)) * (1.0 + reach)
    p[kind == 3] = np.round(p[kind == 3] * 4) / 4
    on_vertex = rng.random(n) < 0.05
    p = (p * scale[:, 0] + offset[:, 0]).astype(real)
    p[on_vertex] = tri[on_vertex, 0]
    bmin, bmax = tri.min(axis=1), tri.max(axis=1)
    pad = (rng.choice([0.0, 0.0, 1e-6, 0.1, 3.0], size=(n, 1)) * scale[:, 0] * rng.random((n, 3))).astype(real)
    bmin, bmax = (bmin - pad).astype(real), (bmax + pad).astype(real)  # (rounded subtraction / addition of a non-negative pad: still contains)
    return np.ascontiguousarray(np.concatenate([p, tri.reshape(n, 9), bmin, bmax], axis=1), dtype=real)


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_box_distance_never_exceeds_the_triangle_distance(real):
    """BoxDist2 <= dist2 in floating point, for every box that contains the triangle's vertices: 1.2 M random cases per precision."""
    rng = np.random.default_rng(5)
    counts = np.zeros((3,), dtype=np.uint64)
    total = 0
    for _ in range(4):
        cases = _bound_cases(rng, real, 300000)
        getattr(cf.model_lib(), "clm_bound_search_" + ("f32" if real == np.float32 else "f64"))(cases.ctypes.data_as(ctypes.c_void_p), cases.shape[0],
                                                                                            counts.ctypes.data_as(ctypes.c_void_p))
        total += cases.shape[0]
    print("bound search %s: %d cases, %d violations, %d equalities, %d boxes not containing" % (np.dtype(real).name, total, counts[0], counts[1], counts[2]))
    assert total >= 1000000 and counts[2] == 0
    assert counts[1] > 1000, "the search no longer reaches the boundary case"
    assert counts[0] == 0


@pytest.fixture(scope="module", params=REALS, ids=IDS)
def trees(request, oracle):
    real = request.param
    v, f = cf.mesh(real)
    host = cf.HostAccel(v, f)
    return real, v, f, host, {"header": host.tree(), "reference": oracle.build(v, f)[:2]}


@pytest.mark.parametrize("which", ["header", "reference"])
def test_walk_equals_brute_force(trees, which):
    real, v, f, _, tr = trees
    nodes, idx = tr[which]
    for name in cf.SET_NAMES:
        out, found = cf.walk(nodes, idx, v, f, cf.point_sets(real)[name])
        cf.assert_same(out, found, *cf.expected(real, name), what="set %s, %s tree" % (name, which))
    for oname, opts in cf.option_cases(real).items():
        out, found = cf.walk(nodes, idx, v, f, cf.point_sets(real)["b"], opts)
        cf.assert_same(out, found, *cf.expected(real, "b", opts), what="set b, options %s, %s tree" % (oname, which))


def test_header_host_form_equals_brute_force(trees):
    """BVHAccel<T>::ClosestPointBatch of include/nanort.h compiled without the backend: the loop over its host walk."""
    real, v, f, host, _ = trees
    for name in cf.SET_NAMES:
        out, found = host.closest(cf.point_sets(real)[name])
        cf.assert_same(out, found, *cf.expected(real, name), what="set %s" % name)
    for oname, opts in cf.option_cases(real).items():
        out, found = host.closest(cf.point_sets(real)["a"], opts)
        cf.assert_same(out, found, *cf.expected(real, "a", opts), what="set a, options %s" % oname)


def _independent_dist2(p, a, b, c):
    """Point-triangle squared distance, numpy float64, all points against all faces: project onto the plane and take that distance if
    the foot lies inside the triangle, else the minimum over the three clamped segment projections.  [points, faces]."""
    p = p[:, None, :]
    a, b, c = a[None], b[None], c[None]

    def seg(x, y):
        d = y - x
        dd = np.maximum((d * d).sum(-1), 1e-300)
        t = np.clip(((p - x) * d).sum(-1) / dd, 0.0, 1.0)
        e = p - (x + t[..., None] * d)
        return (e * e).sum(-1)

    edge = np.minimum(np.minimum(seg(a, b), seg(b, c)), seg(c, a))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    ok = nn > 0
    h = ((p - a) * n).sum(-1)
    plane = h * h / np.where(ok, nn, 1.0)
    foot = p - (h / np.where(ok, nn, 1.0))[..., None] * n
    inside = ok
    for x, y in ((a, b), (b, c), (c, a)):
        inside = inside & ((np.cross(y - x, foot - x) * n).sum(-1) >= 0)
    return np.where(inside, plane, edge)


def test_rule_agrees_with_an_independent_formulation():
    """The rule at double against the formulation above, on the coordinates of sets a and b with max_dist = +inf: the largest
    relative difference of dist2 measured here is 1.24e-12 (set a 1.24e-12, set b 3.42e-13; the model's answer against the minimum
    of the other formulation over all faces; 1.65e-12 while the rule was Ericson's cascade).  The bound is eight times that — room
    for other meshes' conditioning, not for error in the rule."""
    measured = 1.24e-12
    v, f = cf.mesh(np.float64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    worst = 0.0
    for name in ("a", "b"):
        pts = cf.point_sets(np.float64)[name]
        pts = cf.make_points(np.float64, pts["p"], np.inf)
        out, found = cf.brute(v, f, pts)
        assert found.all()
        ind = _independent_dist2(pts["p"], a, b, c).min(axis=1)
        rel = np.abs(out["dist2"] - ind) / ind
        print("independent formulation, set %s: largest relative difference of dist2 %.3g" % (name, rel.max()))
        worst = max(worst, float(rel.max()))
    assert worst <= 8 * measured


@pytest.mark.parametrize("name", cf.HOSTILE_NAMES)
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_rule_within_envelope_of_the_reference(real, name):
    """The rule's brute force on every hostile class against the long-double reference: cf.assert_within_envelope, 8 eps(T) S.
    Largest errors of sqrt(dist2) measured here, in eps(T) S, [most below, most above] the true distance:

      class          fp32, Ericson's cascade  fp32, this rule   fp64, Ericson's cascade  fp64, this rule
      blob           [-0.48, 0.42]            [-0.41, 0.42]     [-0.42, 0.40]            [-0.42, 0.52]
      blob_far       [-0.62, 0.58]            [-0.62, 0.58]     [-0.57, 0.49]            [-0.57, 0.49]
      blob_off       [-0.96, 0.93]            [-1.05, 1.11]     [-0.84, 1.09]            [-0.84, 1.08]
      sliver1        [-0.39, 2.1e5]           [-0.45, 0.43]     [-0.46, 7.5e12]          [-0.46, 0.34]
      sliver4        [-0.44, 7.8e4]           [-0.37, 0.42]     [-0.40, 2.8e12]          [-0.40, 0.33]
      sliver16       [-0.41, 2.1e4]           [-0.40, 0.41]     [-0.38, 1.1e14]          [-0.38, 0.43]
      sliver64       [-0.47, 0.46]            [-0.47, 0.46]     [-0.34, 1.01]            [-0.38, 0.41]
      needle         [-0.32, 0.37]            [-0.37, 0.48]     [-0.40, 0.39]            [-0.34, 0.39]
      speck          [-0.43, 0.29]            [-0.43, 0.29]     [-0.31, 0.28]            [-0.31, 0.28]
      collinear      [-0.48, 2.3e5]           [-0.48, 0.23]     [-0.67, 4.8e13]          [-0.67, 0.25]
      duplicates     [-0.45, 0.50]            [-0.51, 0.50]     [-0.49, 0.47]            [-0.49, 0.47]
      blob_near      [-0.41, 47.6]            [-0.40, 0.41]     [-0.48, 0.35]            [-0.41, 0.47]
      sliver_ladder  [-0.32, 3.4e5]           [-0.29, 0.32]     [-0.27, 1.6e14]          [-0.26, 0.35]
      mixed          [-0.70, 238]             [-0.68, 0.86]     [-0.78, 1.2e12]          [-0.65, 0.56]

    "Ericson's cascade" is the rule as it stood before ClosestPointOnTriangle (the region test alone): this test failed on the
    slivers, `collinear` (a face whose third corner lies on the line beyond the second), the ladder and `mixed` in both precisions,
    and on `blob_near` in fp32 — off by a few hundredths in absolute terms on coordinates of size 1.  All rows are now below 1.2 of 8."""
    cf.require_reference()
    v, f, pts = cf.hostile_classes(real)[name]
    out, found = cf.hostile_brute(real, name)
    cf.assert_within_envelope(real, v, f, pts, out, found, "%s, %s" % (IDS[REALS.index(real)], name), d_true=cf.hostile_reference(real, name))


@pytest.fixture(scope="module", params=REALS, ids=IDS)
def mixed(request):
    cf.require_reference()
    real = request.param
    v, f, pts = cf.hostile_classes(real)["mixed"]
    return real, v, f, pts, cf.mixed_trees(real)


@pytest.mark.parametrize("tree", ["default", "deep_leaves"])
def test_walk_over_the_mixed_mesh_within_envelope(mixed, tree):
    """The model's walk over both reference-built trees of `mixed`: byte-equal to brute force, and within the envelope."""
    real, v, f, pts, trees = mixed
    nodes, idx = trees[tree]
    out, found = cf.walk(nodes, idx, v, f, pts)
    cf.assert_same(out, found, *cf.hostile_brute(real, "mixed"), what="mixed, %s tree" % tree)
    cf.assert_within_envelope(real, v, f, pts, out, found, "mixed, walk of the %s tree" % tree, d_true=cf.hostile_reference(real, "mixed"))


def test_header_host_form_over_the_mixed_mesh_within_envelope(mixed):
    """BVHAccel<T>::ClosestPointBatch of include/nanort.h without the backend, over its own host-built tree of `mixed`."""
    real, v, f, pts, _ = mixed
    out, found = cf.HostAccel(v, f).closest(pts)
    cf.assert_same(out, found, *cf.hostile_brute(real, "mixed"), what="mixed, header's host form")
    cf.assert_within_envelope(real, v, f, pts, out, found, "mixed, header's host form", d_true=cf.hostile_reference(real, "mixed"))


def test_layout_and_exports():
    assert POINT_F32.itemsize == 16 and POINT_F64.itemsize == 32 and CLOSEST_F32.itemsize == 32 and CLOSEST_F64.itemsize == 56
    assert CLOSEST_F32.fields["prim_id"][1] == 24 and CLOSEST_F64.fields["prim_id"][1] == 48
    header = open(os.path.join(ROOT, "include", "nanort_hip.h")).read()
    for t, size in (("nrt_point_f32", 16), ("nrt_point_f64", 32), ("nrt_closest_f32", 32), ("nrt_closest_f64", 56)):
        assert re.search(r"sizeof\(%s\) == %d\b" % (t, size), header), t
    L = capi.lib()
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    for s in ("f32", "f64"):
        for name, argtypes in (("nrtClosestPointBatch_" + s, [vp, vp, u64, vp, vp, vp]), ("nrtClosestPointBatchDevice_" + s, [vp, vp, u64, vp, vp, vp, vp])):
            assert name in capi.SYMBOLS and name in header
            fn = getattr(L, name)
            assert list(fn.argtypes) == argtypes and fn.restype == ctypes.c_int

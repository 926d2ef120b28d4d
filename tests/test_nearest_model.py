"""The K-nearest rule (include/nanort_closest.h) on the CPU: the model against an independent numpy sort of per-face distances, the
model's walk against its brute force on the header's, the reference's and the hostile trees, the header's host form, K = 1 against
the closest-point brute force, and the C ABI's layout, exports and binding table.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import closest_fixture as cf
import nearest_fixture as nf
from nanort_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REALS = [np.float32, np.float64]
IDS = ["f32", "f64"]


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_fixture_conditions(real):
    nf.check_sets(real)


@pytest.mark.parametrize("radii", [False, True], ids=["inf", "radii"])
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_model_equals_an_independent_sort(real, radii):
    """Ids, order, counts and the bits of dist2 of the model's brute force against np.lexsort over the per-face distances of the
    EXISTING closest-point brute force (nf.face_dist2): every set and every K, and the two restricted option cases on set b."""
    for k in nf.KS:
        for name in nf.SET_NAMES:
            cases = [None] + (list(nf.restrictions(real).values()) if name == "b" and not radii else [])
            for opts in cases:
                pts = nf.point_sets(real, k if radii else None)[name]
                out, counts = nf.expected(real, name, k, radii, opts)
                ids, d2, ind_counts = nf.independent_rows(real, name, pts, k, opts)
                what = "K = %d, set %s, options %s" % (k, name, opts)
                assert np.array_equal(counts, ind_counts), what
                assert np.array_equal(out["prim_id"], ids), what
                assert out["dist2"].tobytes() == d2.tobytes(), what


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_held_set_does_not_depend_on_the_order_of_the_faces(real):
    v, f = cf.mesh(real)
    for k in (2, 4, 7):
        for name in ("a", "c"):
            out, counts = nf.brute(v, f, nf.point_sets(real, k)[name], k, reversed_order=True)
            nf.assert_same(out, counts, *nf.expected(real, name, k, True), what="K = %d, set %s, faces in descending order" % (k, name))


@pytest.fixture(scope="module", params=REALS, ids=IDS)
def trees(request, oracle):
    real = request.param
    v, f = cf.mesh(real)
    return real, v, f, {"header": cf.HostAccel(v, f).tree(), "reference": oracle.build(v, f)[:2]}


@pytest.mark.parametrize("which", ["header", "reference"])
def test_walk_equals_brute_force(trees, which):
    real, v, f, tr = trees
    nodes, idx = tr[which]
    for k in nf.KS:
        for radii in (False, True):
            for name in nf.SET_NAMES:
                out, counts = nf.walk(nodes, idx, v, f, nf.point_sets(real, k if radii else None)[name], k)
                nf.assert_same(out, counts, *nf.expected(real, name, k, radii), what="K = %d, set %s, radii %s, %s tree" % (k, name, radii, which))
    for oname, opts in nf.restrictions(real).items():
        out, counts = nf.walk(nodes, idx, v, f, nf.point_sets(real)["b"], 7, opts)
        nf.assert_same(out, counts, *nf.expected(real, "b", 7, False, opts), what="K = 7, set b, %s, %s tree" % (oname, which))


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_header_host_form_equals_brute_force(real):
    """BVHAccel<T>::NearestFacesBatch of include/nanort.h compiled without the backend: the loop over its host walk."""
    v, f = cf.mesh(real)
    host = nf.HostAccel(v, f)
    for k in nf.KS:
        for radii in (False, True):
            for name in nf.SET_NAMES:
                out, counts = host.nearest(nf.point_sets(real, k if radii else None)[name], k)
                nf.assert_same(out, counts, *nf.expected(real, name, k, radii), what="K = %d, set %s, radii %s" % (k, name, radii))
    for oname, opts in nf.restrictions(real).items():
        out, counts = host.nearest(nf.point_sets(real)["a"], 4, opts)
        nf.assert_same(out, counts, *nf.expected(real, "a", 4, False, opts), what="K = 4, set a, %s" % oname)


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_k1_is_the_closest_point_query(real):
    """K = 1 under closest_fixture's own radii: the record is the closest-point brute force's byte for byte, count its found byte."""
    v, f = cf.mesh(real)
    for name in nf.SET_NAMES:
        out, counts = nf.brute(v, f, cf.point_sets(real)[name], 1)
        ref_out, ref_found = cf.expected(real, name)
        assert out[:, 0].tobytes() == ref_out.tobytes() and np.array_equal(counts, ref_found.astype(np.uint32)), "set %s" % name
    for oname, opts in cf.option_cases(real).items():
        out, counts = nf.brute(v, f, cf.point_sets(real)["b"], 1, opts)
        ref_out, ref_found = cf.expected(real, "b", opts)
        assert out[:, 0].tobytes() == ref_out.tobytes() and np.array_equal(counts, ref_found.astype(np.uint32)), oname


@pytest.mark.parametrize("name", ["duplicates", "collinear", "mixed"])
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_hostile_classes(real, name):
    """Repeated faces and faces with two equal corners (equal dist2: the prim_id orders them), faces without area, and the mixed
    mesh, K in {2, 7}: the header's host form over its own tree equals the model's brute force, the first record is the closest-point
    brute force's, and a row's keys ascend strictly."""
    cf.require_reference()
    v, f, pts = cf.hostile_classes(real)[name]
    host = nf.HostAccel(v, f)
    for k in (2, 7):
        ref_out, ref_counts = nf.brute(v, f, pts, k)
        out, counts = host.nearest(pts, k)
        nf.assert_same(out, counts, ref_out, ref_counts, what="%s, K = %d" % (name, k))
        one, found = cf.hostile_brute(real, name)
        assert ref_out[:, 0].tobytes() == one.tobytes() and np.array_equal(ref_counts != 0, found != 0)
        for j in range(1, k):
            held = ref_counts > j
            d0, d1 = ref_out[held, j - 1]["dist2"], ref_out[held, j]["dist2"]
            assert ((d0 < d1) | ((d0 == d1) & (ref_out[held, j - 1]["prim_id"] < ref_out[held, j]["prim_id"]))).all()


@pytest.mark.parametrize("tree", ["default", "deep_leaves"])
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_walk_over_the_mixed_trees(real, tree):
    """The model's walk over both reference-built trees of `mixed`; `deep_leaves` has a leaf of 256 faces, more than any K."""
    cf.require_reference()
    v, f, pts = cf.hostile_classes(real)["mixed"]
    nodes, idx = cf.mixed_trees(real)[tree]
    if tree == "deep_leaves":
        assert nodes[nodes["flag"] != 0]["data"][:, 0].max() > capi.NRT_MAX_NEAREST
    for k in (2, 7, 64):
        out, counts = nf.walk(nodes, idx, v, f, pts, k)
        nf.assert_same(out, counts, *nf.brute(v, f, pts, k), what="mixed, %s tree, K = %d" % (tree, k))


def test_layout_exports_and_the_binding_table():
    header = open(os.path.join(ROOT, "include", "nanort_hip.h")).read()
    assert "#define NRT_MAX_NEAREST 64u" in header and capi.NRT_MAX_NEAREST == 64
    L = capi.lib()
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    for s in ("f32", "f64"):
        for name, argtypes in (("nrtNearestFacesBatch_" + s, [vp, vp, u64, u32, vp, vp, vp]),
                               ("nrtNearestFacesBatchDevice_" + s, [vp, vp, u64, u32, vp, vp, vp, vp])):
            assert name in capi.SYMBOLS and name in header
            fn = getattr(L, name)
            assert list(fn.argtypes) == argtypes and fn.restype == ctypes.c_int
    from nanort_amd import BVHAccel

    assert hasattr(BVHAccel, "NearestFacesBatch") and hasattr(BVHAccel, "NearestFacesBatchDevice")

"""The signed-distance rule (include/nanort_sdf.h) on the CPU: ClosestFeatureOnTriangle against ClosestPointOnTriangle bit for bit,
the signs against the winding number in long double, the walk and the header's host form against brute force, the normals against a
long-double formulation, and the C ABI's layout and exports.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import closest_fixture as cf
import sdf_fixture as sf
from nanort_amd import capi
from nanort_amd.wire import SIGNED_F32, SIGNED_F64, closest_dtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REALS = [np.float32, np.float64]
IDS = ["f32", "f64"]


def _sfx(real):
    return IDS[REALS.index(real)]


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_feature_rule_is_the_closest_point_rule_bit_for_bit(real):
    """Every point of every hostile class of the closest fixture against 40 of its faces: (u, v, q, dist2) of
    ClosestFeatureOnTriangle are ClosestPointOnTriangle's bytes, the code is one of 0..6 and agrees with what (u, v) allow."""
    cf.require_reference()
    rng = np.random.default_rng(3)
    seen = np.zeros(7, dtype=np.int64)
    for name in cf.HOSTILE_NAMES:
        v, f, pts = cf.hostile_classes(real)[name]
        pick = rng.choice(f.shape[0], size=40, replace=False)
        tri = v[f[pick]].reshape(40, 9)
        p = pts["p"][::7]
        cases = np.concatenate([np.repeat(p, 40, axis=0), np.tile(tri, (p.shape[0], 1))], axis=1)
        a, b, codes = sf.feature_cases(real, cases)
        assert a.tobytes() == b.tobytes(), name
        assert (codes <= 6).all(), name
        u, w = a[:, 0], a[:, 1]
        ok = np.ones(codes.shape, dtype=bool)
        ok &= (codes != 4) | ((u == 0) & (w == 0))
        ok &= (codes != 5) | ((u == 1) & (w == 0))
        ok &= (codes != 6) | ((u == 0) & (w == 1))
        ok &= (codes != 1) | (w == 0)
        ok &= (codes != 2) | (u == 0)
        assert ok.all(), "%s: %d codes contradict their (u, v)" % (name, (~ok).sum())
        seen += np.bincount(codes, minlength=7)
    assert (seen > 0).all(), seen


def test_fixture_is_sharp():
    """From the model's codes: on cube and wedge each of the seven features wins for at least 40 points (the reference-only
    conditions — a tenth inside and outside, at most 5 % left out, the wedge's face normals wrong for a tenth — are asserted by the
    fixture itself when a class is first used)."""
    cf.require_reference()
    for name in ("cube", "wedge"):
        v, f, pts = sf.closed_classes(np.float32)[name]
        sf.closed_reference(name)
        out, _ = sf.brute(v, f, sf.model_normals(v, f), pts)
        counts = np.bincount(sf.codes(out), minlength=7)
        print(name, "feature codes won:", counts)
        assert (counts >= 40).all(), (name, counts)


@pytest.fixture(scope="module", params=REALS, ids=IDS)
def closed(request):
    cf.require_reference()
    real = request.param
    d = {}
    for name in sf.CLOSED_NAMES:
        v, f, pts = sf.closed_classes(real)[name]
        nrm = sf.model_normals(v, f)
        d[name] = (v, f, pts, nrm, sf.brute(v, f, nrm, pts))
    return real, d


@pytest.mark.parametrize("name", sf.CLOSED_NAMES)
def test_signs_equal_the_winding_number(closed, name):
    """Nothing may be wrong among the checked points (those farther than 8 eps S from the surface).  Measured here: 0 wrong in every
    class and both precisions; signing by the face normal alone is wrong for 896 (fp32) / 883 (fp64) of the wedge's 4003 points."""
    real, d = closed
    v, f, pts, nrm, (out, found) = d[name]
    ref = sf.closed_reference(name)
    ok = sf.checked(real, name)
    assert found.all()
    sf.assert_word_is_clean(out, found)
    wrong = (sf.inside_bits(out) != ref["inside"]) & ok
    print("%s %s: %d checked, %d left out, %d wrong" % (_sfx(real), name, ok.sum(), (~ok).sum(), wrong.sum()))
    assert wrong.sum() == 0, "%s: wrong signs at points %s" % (name, np.nonzero(wrong)[0][:8])
    if name == "wedge":  # the test can tell the rule from the shortcut
        short, _ = sf.brute(v, f, nrm, pts, face_normal_only=True)
        assert ((sf.inside_bits(short) != ref["inside"]) & ok).sum() >= ok.sum() / 10.0


@pytest.mark.parametrize("name", sf.CLOSED_NAMES)
def test_signed_record_extends_the_closest_record(closed, name):
    """The first 28 (fp32) / 52 (fp64) bytes of a signed record are the closest-point model's record."""
    real, d = closed
    v, f, pts, _, (out, found) = d[name]
    c_out, c_found = cf.brute(v, f, pts)
    k = closest_dtype(real).itemsize - 4
    assert k == (28 if real == np.float32 else 52)
    a = out.view(np.uint8).reshape(-1, k + 4)[:, :k]
    b = c_out.view(np.uint8).reshape(-1, k + 4)[:, :k]
    assert np.array_equal(a, b) and np.array_equal(found, c_found)


def test_walk_and_host_form_equal_brute_force(closed, oracle):
    """The model's walk over two trees (the header's own and the reference builder's), and BVHAccel<T>::SignedDistanceBatch of
    include/nanort.h without the backend with FeatureNormals<T>, are byte-equal to brute force — also with a range, a skip id and
    finite radii; the header's normals are the model's bytes."""
    real, d = closed
    for name in ("wedge", "torus", "cube_grid"):
        v, f, pts, nrm, (out, found) = d[name]
        host = sf.HostAccel(v, f)
        hn = host.normals()
        assert hn[0].tobytes() == nrm[0].tobytes() and hn[1].tobytes() == nrm[1].tobytes()
        trees = {"header": cf.HostAccel(v, f).tree(), "reference": oracle.build(v, f)[:2]}
        radii = pts.copy()
        radii["max_dist"][1::2] = np.asarray(0.3, dtype=real)
        nf = f.shape[0]
        for what, p, opts in (("plain", pts, None), ("radii", radii, None), ("range", pts, (nf // 3, nf, 0xFFFFFFFF)), ("skip", radii, (0, 0x7FFFFFFF, 1))):
            exp = (out, found) if what == "plain" else sf.brute(v, f, nrm, p, opts)
            for tname, (nodes, idx) in trees.items():
                cf.assert_same(*sf.walk(nodes, idx, v, f, nrm, p, opts), *exp, what="%s, %s, %s tree" % (name, what, tname))
            cf.assert_same(*host.signed(p, opts), *exp, what="%s, %s, header's host form" % (name, what))
            sf.assert_word_is_clean(*exp)


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_hostile_classes_walk_equals_brute_force(real, oracle):
    """Outside the sign's guarantee the answer is still one answer: walk and host form byte-equal to brute force."""
    cf.require_reference()
    for name in sf.HOSTILE_NAMES:
        v, f, pts = sf.hostile_classes(real)[name]
        nrm = sf.model_normals(v, f, v.shape[0])
        exp = sf.brute(v, f, nrm, pts)
        sf.assert_word_is_clean(*exp)
        nodes, idx = oracle.build(v, f)[:2]
        cf.assert_same(*sf.walk(nodes, idx, v, f, nrm, pts), *exp, what="%s, reference tree" % name)
        cf.assert_same(*sf.HostAccel(v, f).signed(pts), *exp, what="%s, header's host form" % name)
    v, f, _ = sf.hostile_classes(real)["unreferenced"]
    assert (sf.model_normals(v, f, v.shape[0])[1][3] == 0).all(), "an unreferenced vertex gets the zero normal"


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_normals_against_a_long_double_formulation(real):
    """max |n_T - n_ref| (infinity norm) in eps(T) per face summed (face and edge normals) and in eps(T) x the sum of the corner
    angles (vertex normals), over the closed classes.  Measured here:

      class        fp32 face/edge  fp32 vertex   fp64 face/edge  fp64 vertex
      cube         0               0.134         0               0.059
      wedge        0.838           0.421         0.533           0.522
      torus        1.208           0.866         0.698           1.100
      torus_fine   0.854           1.044         1.095           1.182

    The bound is eight times the largest measured value of the precision (sdf_fixture.MEASURED_*)."""
    cf.require_reference()
    worst = [0.0, 0.0]
    for name in sf.CLOSED_NAMES[:4]:
        v, f, _ = sf.closed_classes(real)[name]
        e = sf.normals_error(real, sf.model_normals(v, f), sf.closed_reference(name)["normals"])
        print("%s %s: face/edge normals %.3f eps, vertex normals %.3f eps x angles" % (_sfx(real), name, e[0], e[1]))
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    assert worst[0] <= 8 * sf.MEASURED_FACE_NORMAL_ERROR[_sfx(real)]
    assert worst[1] <= 8 * sf.MEASURED_VERTEX_NORMAL_ERROR[_sfx(real)]


def test_layout_and_exports():
    assert SIGNED_F32.itemsize == 32 and SIGNED_F64.itemsize == 56
    assert SIGNED_F32.fields["feature"][1] == 28 and SIGNED_F64.fields["feature"][1] == 52
    assert SIGNED_F32.fields["prim_id"][1] == 24 and SIGNED_F64.fields["prim_id"][1] == 48
    header = open(os.path.join(ROOT, "include", "nanort_hip.h")).read()
    for t, size in (("nrt_signed_f32", 32), ("nrt_signed_f64", 56)):
        assert re.search(r"sizeof\(%s\) == %d\b" % (t, size), header), t
    L = capi.lib()
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    for s in ("f32", "f64"):
        for name, argtypes in (("nrtSignedDistanceBatch_" + s, [vp, vp, u64, vp, vp, vp]), ("nrtSignedDistanceBatchDevice_" + s, [vp, vp, u64, vp, vp, vp, vp]),
                               ("nrtGetFeatureNormals_" + s, [vp, vp, vp])):
            assert name in capi.SYMBOLS and name in header
            assert not any(w in name for w in ("Skip", "Masked", "Motion", "Closest"))
            fn = getattr(L, name)
            assert list(fn.argtypes) == argtypes and fn.restype == ctypes.c_int

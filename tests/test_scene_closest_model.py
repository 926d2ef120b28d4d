"""CPU proof-by-test of the closest-point query on instanced scenes (include/nanort_closest.h "instanced scenes"):
the two properties of XformBox that the cull inside an instance rests on, searched in numpy float32; the C++ model of the
two-level walk (tests/scene_closest_model.cc) byte for byte against the brute force over the concatenated world mesh, whatever the
trees and the order of the instances; and the interface (record layout, symbols, bindings, the header's text)."""
import ctypes
import os
import re

import numpy as np
import pytest

import closest_fixture as cf
import scene_closest_fixture as sf
from nanort_amd import capi
from nanort_amd.wire import POINT_F32, SCENE_CLOSEST_F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
PAIRS, PER_PAIR = 3000, 400  # 3 000 matrix / box pairs, 1.2 M points


def _pairs():
    """Matrices of mixed signs with entries of 1e-3 .. 1e3, zero and -0 entries and large translations; boxes of any size, a fifth of
    them flat in one axis."""
    rng = np.random.default_rng(20261021)
    m = np.zeros((PAIRS, 4, 4), dtype=F32)
    mag = 10.0 ** rng.uniform(-3, 3, size=(PAIRS, 3, 3))
    m[:, :3, :3] = (mag * rng.choice([-1.0, 1.0], size=(PAIRS, 3, 3))).astype(F32)
    zero = rng.random(size=(PAIRS, 3, 3)) < 0.15
    m[:, :3, :3][zero] = np.where(rng.random(size=int(zero.sum())) < 0.5, F32(0.0), F32(-0.0))
    m[:, 3, :3] = (10.0 ** rng.uniform(-2, 6, size=(PAIRS, 3)) * rng.choice([-1.0, 1.0], size=(PAIRS, 3))).astype(F32)
    m[:, 3, 3] = 1
    c = 10.0 ** rng.uniform(-2, 3, size=(PAIRS, 3)) * rng.choice([-1.0, 1.0], size=(PAIRS, 3))
    h = 10.0 ** rng.uniform(-3, 2, size=(PAIRS, 3))
    bmin, bmax = (c - h).astype(F32), (c + h).astype(F32)
    flat = np.arange(PAIRS) % 5 == 0
    axis = rng.integers(0, 3, size=PAIRS)
    bmax[flat, axis[flat]] = bmin[flat, axis[flat]]
    assert (bmin <= bmax).all() and (np.signbit(m[:, :3, :3]) & (m[:, :3, :3] == 0)).any()
    return rng, m, bmin, bmax


def _points_in(rng, bmin, bmax):
    """PER_PAIR points inside each box: uniform, the eight corners, and points one ulp inside a face of the box."""
    lo, hi = bmin[:, None, :], bmax[:, None, :]
    v = (lo + (hi - lo) * rng.random(size=(PAIRS, PER_PAIR, 3)).astype(F32)).astype(F32)
    v = np.minimum(np.maximum(v, lo), hi)
    for i in range(8):
        v[:, i] = np.stack([np.where(i & (1 << j), bmax[:, j], bmin[:, j]) for j in range(3)], axis=-1)
    up, down = np.nextafter(lo, hi), np.nextafter(hi, lo)  # (a flat axis: lo == hi, and both stay there)
    v[:, 8:40] = np.where(rng.random(size=(PAIRS, 32, 3)) < 0.5, up, down)
    assert ((v >= lo) & (v <= hi)).all() and v.dtype == F32
    return v


def test_xform_box_is_the_corner_box_and_contains_every_image():
    rng, m, bmin, bmax = _pairs()
    lo, hi = sf.xform_box(m, bmin, bmax)
    clo, chi = sf.corner_box(m, bmin, bmax)
    assert np.isfinite(lo).all() and np.isfinite(hi).all()
    # (a) bit for bit the min / max over the eight corner images in mult_v's order: what Commit stores for an instance
    assert lo.tobytes() == clo.tobytes() and hi.tobytes() == chi.tobytes()
    # (b) it contains XformPoint(m, v) for every v inside the local box
    v = _points_in(rng, bmin, bmax)
    w = sf.xform_point(m[:, None], v)
    outside = (w < lo[:, None, :]) | (w > hi[:, None, :])
    assert v.shape[0] * v.shape[1] == 1200000 and not outside.any(), "%d images lie outside XformBox" % outside.sum()
    # the header's functions are these, bit for bit
    L = sf.model_lib()
    hlo, hhi = np.zeros_like(lo), np.zeros_like(hi)
    L.scm_xform_boxes(sf._p(m), sf._p(bmin), sf._p(bmax), PAIRS, sf._p(hlo), sf._p(hhi))
    assert hlo.tobytes() == lo.tobytes() and hhi.tobytes() == hi.tobytes()
    some_v = np.ascontiguousarray(v[:, :16].reshape(-1, 3))
    some_m = np.ascontiguousarray(np.repeat(m, 16, axis=0))
    hw = np.zeros_like(some_v)
    L.scm_xform_points(sf._p(some_m), sf._p(some_v), some_v.shape[0], sf._p(hw))
    assert hw.tobytes() == np.ascontiguousarray(w[:, :16].reshape(-1, 3)).tobytes()


def test_box_distance_never_exceeds_a_face_inside_the_box():
    """BoxDist2(p, XformBox(box)) <= dist2 for faces whose local vertices lie in the box, in floating point: 40 faces and points per
    pair, the points near the world box and far from it."""
    rng, m, bmin, bmax = _pairs()
    v = _points_in(rng, bmin, bmax)[:, :120].reshape(PAIRS, 40, 3, 3)  # (corners and one-ulp points among the vertices)
    lo, hi = sf.xform_box(m, bmin, bmax)
    ext = np.maximum((hi - lo).astype(np.float64), 1e-3)[:, None, :]
    p = (0.5 * (lo.astype(np.float64) + hi)[:, None, :] + ext * rng.normal(scale=2.0, size=(PAIRS, 40, 3)) * 10.0 ** rng.uniform(-2, 2, size=(PAIRS, 40, 1))).astype(F32)
    p[:, ::5] = sf.xform_point(m[:, None], v[:, ::5, 0])  # a fifth of the points ON a world vertex: dist2 is 0
    cases = np.zeros((PAIRS, 40, 34), dtype=F32)
    cases[:, :, :16] = m.reshape(PAIRS, 1, 16)
    cases[:, :, 16:19], cases[:, :, 19:22] = bmin[:, None], bmax[:, None]
    cases[:, :, 22:31] = v.reshape(PAIRS, 40, 9)
    cases[:, :, 31:34] = p
    counts = np.zeros((3,), dtype=np.uint64)
    sf.model_lib().scm_bound_search(sf._p(np.ascontiguousarray(cases)), PAIRS * 40, sf._p(counts))
    assert counts[2] == 0
    assert counts[0] == 0, "%d faces lie nearer than the world box of their local box" % counts[0]
    assert counts[1] > 0  # (equality is reached: Culled must be strict)


SCENE_NAMES = ["five", "twelve", "one_triangle", "two", "twice", "shared_face"]


def _points(name):
    inst = sf.scene(name)
    if name in ("five", "twelve"):
        sets = sf.point_sets(name, inst)
        return np.concatenate([sets[k] for k in ("surface", "bounds", "far")])
    return sf.tie_points(inst)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_the_two_level_walk_is_the_brute_force(name):
    """Two different bottom trees per mesh, the scan in node order and reversed, and two different top-level trees: the bytes of
    the brute force over the concatenated world mesh, every time."""
    inst = sf.scene(name)
    pts = _points(name)
    ref_out, ref_found = sf.expected(inst, pts)
    assert 0 < ref_found.sum()
    opened = []
    for which in ("default", "deep_leaves"):
        trees = sf.bottom_trees(inst, which)
        xbmin, xbmax = sf.world_boxes(inst, trees)
        tops = [None, None] + ([sf.top_tree(xbmin, xbmax, 1), sf.top_tree(xbmin, xbmax, 3, flip=True)] if len(inst) > 1 else [])
        orders = [None, np.arange(len(inst), dtype=np.uint32)[::-1]]
        for k, top in enumerate(tops):
            out, found, stats = sf.model_walk(inst, trees, pts, top=top, scan_order=orders[k] if k < 2 else None)
            sf.assert_same(out, found, ref_out, ref_found, what="%s, %s trees, form %d" % (name, which, k))
            opened.append(int(stats[2]))
    if name in ("five", "twelve"):  # the walk culls: it tests far fewer faces than the brute force
        assert max(opened) < 0.5 * pts.shape[0] * sf.world_mesh(inst)[1].shape[0]


def test_ties_go_to_the_smaller_node_then_the_smaller_prim():
    out, found = sf.expected(sf.scene("twice"), sf.tie_points(sf.scene("twice")))
    assert found.all() and (out["node_id"] == 0).all()
    inst = sf.scene("shared_face")
    pts = cf.make_points(F32, np.array([[0.5, 0.5, 0.0], [0.25, 0.5, 1.0], [0, 0, 0], [2, 0, -1]], dtype=F32), np.inf)
    out, found = sf.expected(inst, pts)
    assert found.all() and (out["node_id"] == 0).all() and (out["prim_id"] == 1).all()  # (node 1 holds the same face as prim 0)
    trees = sf.bottom_trees(inst, "default")
    sf.assert_same(*sf.model_walk(inst, trees, pts, scan_order=[1, 0])[:2], out, found, what="shared face")
    inst, p = sf.shared_vertex()
    out, found = sf.expected(inst, cf.make_points(F32, p, np.inf))
    assert found.all() and out["dist2"][0] == 0 and out["node_id"][0] == 0
    assert out["point"].tobytes() == p.tobytes()


def test_masks_in_the_model():
    inst = sf.scene("five")
    pts = sf.point_sets("five", inst)["bounds"]
    rng = np.random.default_rng(3)
    node_words = np.array([1, 2, 4, 8, 0x10], dtype=np.uint32)
    point_words = rng.choice(np.array([0, 1, 6, 0x18, 0x1F, 0xFFFFFFFF, 0x20], dtype=np.uint32), size=pts.shape[0])
    ref_out, ref_found = sf.expected(inst, pts, node_words, point_words)
    plain_out, _ = sf.expected(inst, pts)
    assert ref_out.tobytes() != plain_out.tobytes()
    hidden = (point_words == 0) | (point_words == 0x20)
    assert not ref_found[hidden].any() and (ref_out["node_id"][hidden] == sf.MISS).all()
    trees = sf.bottom_trees(inst, "default")
    out, found, _ = sf.model_walk(inst, trees, pts, node_words=node_words, point_words=point_words)
    sf.assert_same(out, found, ref_out, ref_found, what="masked")
    full = point_words == 0xFFFFFFFF
    assert ref_out[full].tobytes() == plain_out[full].tobytes()


# ---- the interface -----------------------------------------------------------------------------------------------------------------------
def test_record_layout():
    assert SCENE_CLOSEST_F32.itemsize == 32
    assert [SCENE_CLOSEST_F32.fields[k][1] for k in ("point", "dist2", "u", "v", "prim_id", "node_id")] == [0, 12, 16, 20, 24, 28]
    src = open(os.path.join(ROOT, "include", "nanort_hip.h")).read()
    assert re.search(r"typedef struct \{ float point\[3\]; float dist2; float u, v; uint32_t prim_id; uint32_t node_id; \} nrt_scene_closest_f32;", src)
    assert POINT_F32.itemsize == 16


def test_symbols_are_exported_and_bound():
    L = capi.lib()
    for name in ("nrtSceneClosestPointBatch_f32", "nrtSceneClosestPointBatchDevice_f32"):
        assert name in capi.SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == 6 and fn.restype is ctypes.c_int32
    from nanort_amd import Scene

    assert callable(Scene.ClosestPointBatch) and callable(Scene.ClosestPointBatchDevice)
    sg = open(os.path.join(ROOT, "include", "nanosg_hip.h")).read()
    assert "bool ClosestPoint(const nrt_point_f32 *points, size_t num_points, const uint32_t *point_masks, nrt_scene_closest_f32 *out" in sg


def test_the_header_no_longer_excludes_scenes_for_this_query_only():
    src = open(os.path.join(ROOT, "include", "nanort_hip.h")).read()
    sections = dict((m.group(1), m.start()) for m in re.finditer(r"/\* ---- ([a-z\- ]+?) -{10,}", src))
    order = sorted(sections.items(), key=lambda kv: kv[1])

    def not_covered(title):
        k = [t for t, _ in order].index(title)
        body = src[order[k][1]:order[k + 1][1] if k + 1 < len(order) else len(src)]
        return re.search(r"Not covered:(.*?)\*/", body, flags=re.S).group(1)

    assert "scenes" not in not_covered("closest-point queries").split("(")[0]
    assert "scenes" in not_covered("signed distance queries") and "scenes" in not_covered("nearest-faces queries")
    scene_part = not_covered("closest-point queries on scenes")
    assert "signed distance" in scene_part and "skip pairs" in scene_part and "fp64" in scene_part


def test_the_staging_piece_is_named_in_the_source():
    src = open(os.path.join(ROOT, "nanort_amd", "csrc", "scene.hip")).read()
    found = re.findall(r"const uint64_t kSceneClosestPiece = 1ull << (\d+);", src)
    assert found == ["20"]
    assert "in pieces of 2^20 points" in open(os.path.join(ROOT, "include", "nanort_hip.h")).read().split("closest-point queries on scenes")[1]

"""nrtSceneClosestPointBatch* on the GPU (nanort_amd/csrc/scene_closest.hip; include/nanort_hip.h, "closest-point queries on scenes";
DESIGN.md 3.20): every record and found byte identical to the brute force over the ONE mesh a scene's answer is defined over — the
world vertices of all instances concatenated in node order (tests/scene_closest_fixture.py) — in the host and the Device form."""
import os
import re

import numpy as np
import pytest

import closest_fixture as cf
import scene_closest_fixture as sf
from nanort_amd import BVHAccel, Scene, TriangleMesh
from nanort_amd.capi import NRT_ERR_INVALID, NRT_OK, NrtError
from nanort_amd.wire import CLOSEST_F32, POINT_F32, SCENE_CLOSEST_F32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FORMS = ["host", "device"]


def make_scene(instances, adopt=None):
    """(scene, the BVHAccel of every distinct mesh): built trees, or `adopt` = (nodes, indices) set on every mesh."""
    sc, accels = Scene(), {}
    for v, f, m in instances:
        key = (id(v), id(f))
        if key not in accels:
            a = BVHAccel(F32)
            if adopt is None:
                assert a.Build(f.shape[0], TriangleMesh(v, f))
            else:
                a.SetMesh(TriangleMesh(v, f))
                a.SetTree(*adopt)
            accels[key] = a
        sc.AddNode(accels[key], m)
    assert sc.Commit()
    return sc, accels


def to_device(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def query(sc, pts, words=None, form="host", fill=0xA5):
    """(records, found) of either form; the Device form's outputs start filled with a pattern."""
    if form == "host":
        return sc.ClosestPointBatch(pts, point_masks=words)
    import torch

    n = pts.shape[0]
    d_out = torch.full((n * SCENE_CLOSEST_F32.itemsize,), fill, dtype=torch.uint8, device="cuda")
    d_found = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    d_words = None if words is None else to_device(np.ascontiguousarray(words, dtype=np.uint32))
    assert sc.ClosestPointBatchDevice(to_device(pts), d_out, d_found, d_words) == n
    return d_out.cpu().numpy().view(SCENE_CLOSEST_F32), d_found.cpu().numpy()


_SCENES = {}


def gpu_scene(name):
    if name not in _SCENES:
        _SCENES[name] = make_scene(sf.scene(name))
    return _SCENES[name][0]


def test_one_identity_instance_is_the_single_mesh_query():
    """Bytes equal nrtClosestPointBatch_f32 on the same context, node_id = 0 in the place of _pad where found, 0xFFFFFFFF where not."""
    v, f = cf.mesh(F32)
    sc, accels = make_scene([(v, f, sf.IDENT)])
    a = list(accels.values())[0]
    for name in ("b", "c", "e"):
        pts = cf.point_sets(F32)[name]
        single, single_found = a.ClosestPointBatch(pts)
        want = single.copy().view(SCENE_CLOSEST_F32)
        want["node_id"] = np.where(single_found != 0, 0, 0xFFFFFFFF)
        for form in FORMS:
            out, found = query(sc, pts, form=form)
            sf.assert_same(out, found, want, single_found, what="set %s, %s form" % (name, form))
    assert CLOSEST_F32.itemsize == SCENE_CLOSEST_F32.itemsize


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["surface", "bounds", "far"])
def test_five_nodes_scan_path(which, form):
    """The 5-node scene_fixture (at most scan_max = 8 nodes: no top-level tree): byte-identical to the expectation."""
    inst = sf.scene("five")
    sc = gpu_scene("five")
    pts = sf.point_sets("five", inst)[which]
    out, found = query(sc, pts, form=form)
    ref_out, ref_found = sf.expected_sets("five", inst, which)
    sf.assert_same(out, found, ref_out, ref_found, what="five nodes, %s, %s form" % (which, form))
    assert sc.LastPath() == 2  # (nrt::k_scene_closest_point<32>)
    if which == "surface":
        assert 0 < found.sum() < found.shape[0] and not found[~np.isfinite(pts["p"]).all(axis=1)].any()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["surface", "bounds", "far"])
def test_five_nodes_within_the_tolerance_of_long_double(which, form):
    """The same records within closest_fixture.tolerance of the long-double distance over the world vertices (needs a long double
    of at least 61 bits: skipped as a whole where there is none)."""
    cf.require_reference()
    inst = sf.scene("five")
    pts = sf.point_sets("five", inst)[which]
    out, found = query(gpu_scene("five"), pts, form=form)
    wv, wf, _, _ = sf.world_mesh(inst)
    sel = found != 0
    d_true = cf.reference_distance(wv, wf, pts["p"][sel])
    tol = cf.tolerance(F32, wv, pts["p"][sel])
    err = np.abs(np.sqrt(out["dist2"][sel].astype(cf.LD)) - d_true)
    print("five nodes, %s: %d found, largest error %.3g of the tolerance %.3g" % (which, sel.sum(), float(err.max() / tol), float(tol)))
    assert sel.any() and (err <= tol).all()


def test_scene_bounds_hold_the_bounds_set():
    """The `bounds` set is uniform in nrtSceneBounds of the scene as the GPU committed it."""
    inst = sf.scene("five")
    lo, hi = gpu_scene("five").GetBoundingBox()
    wlo, whi = sf.scene_bounds(inst)
    assert (lo <= wlo + 1e-6).all() and (hi >= whi - 1e-6).all()
    p = sf.point_sets("five", inst)["bounds"]["p"]
    assert (p >= lo).all() and (p <= hi).all()


@pytest.mark.parametrize("form", FORMS)
def test_twelve_nodes_top_level_tree_path(form):
    """More than scan_max = 8 nodes: rotation x non-uniform scale, a shear, a mirror, entries of both signs in every column, and an
    instance flattened by a singular matrix (Commit takes it: the query reads xform only)."""
    inst = sf.scene("twelve")
    sc = gpu_scene("twelve")
    for which in ("surface", "bounds", "far"):
        out, found = query(sc, sf.point_sets("twelve", inst)[which], form=form)
        sf.assert_same(out, found, *sf.expected_sets("twelve", inst, which), what="twelve nodes, %s, %s form" % (which, form))
    ref = sf.expected_sets("twelve", inst, "surface")[0]
    assert set(range(12)) <= set(int(x) for x in np.unique(ref["node_id"])), "some node is never the answer"


@pytest.mark.parametrize("form", FORMS)
def test_ties(form):
    inst = sf.scene("twice")
    pts = sf.tie_points(inst)
    out, found = query(gpu_scene("twice"), pts, form=form)
    sf.assert_same(out, found, *sf.expected(inst, pts), what="the same mesh twice")
    assert found.all() and (out["node_id"] == 0).all()
    inst = sf.scene("shared_face")
    pts = cf.make_points(F32, np.array([[0.5, 0.5, 0.0], [0.25, 0.5, 1.0], [0, 0, 0], [2, 0, -1], [5, 5, 5.5], [-5, -5, 4]], dtype=F32), np.inf)
    out, found = query(gpu_scene("shared_face"), pts, form=form)
    sf.assert_same(out, found, *sf.expected(inst, pts), what="a shared world face")
    assert (out["node_id"][:4] == 0).all() and (out["prim_id"][:4] == 1).all()  # (node before prim: node 1 holds the face as prim 0)
    assert out["node_id"][5] == 1


@pytest.mark.parametrize("form", FORMS)
def test_smallest_shapes(form):
    for name in ("one_triangle", "two"):
        inst = sf.scene(name)
        pts = sf.tie_points(inst, n=200)
        pts = np.concatenate([pts, cf.make_points(F32, pts["p"][:60] + F32(0.5), 0.4)])
        out, found = query(gpu_scene(name), pts, form=form)
        sf.assert_same(out, found, *sf.expected(inst, pts), what=name)
        assert 0 < found.sum() < found.shape[0]
    inst, p = sf.shared_vertex()
    sc, _keep = make_scene(inst)
    pts = cf.make_points(F32, np.concatenate([p, p + F32(0.25)]), np.inf)
    out, found = query(sc, pts, form=form)
    sf.assert_same(out, found, *sf.expected(inst, pts), what="a shared vertex")
    assert out["dist2"][0] == 0 and out["node_id"][0] == 0 and out["point"][0].tobytes() == p.tobytes()


@pytest.mark.parametrize("form", FORMS)
def test_stack_across_both_levels_goes_on_in_the_overflow_area(form):
    """300 instances of an adopted 47-level tree: the model counts 47 entries of an instance's tree waiting at once, on top of the
    top level's — past the 32 LDS entries of a lane's stack."""
    inst, tree, pts = sf.deep_scene()
    ref_out, ref_found = sf.expected(inst, pts)
    _, _, stats = sf.model_walk(inst, [tree] * len(inst), pts[:12])
    assert stats[3] > 33, "fixture no longer exercises the overflow area"
    if "deep" not in _SCENES:
        _SCENES["deep"] = make_scene(inst, adopt=tree)
    out, found = query(_SCENES["deep"][0], pts, form=form)
    sf.assert_same(out, found, ref_out, ref_found, what="deep trees, %s form" % form)
    assert found.all()


def test_masks():
    inst = sf.scene("five")
    sc, _keep = make_scene(inst)
    pts = sf.point_sets("five", inst)["bounds"]
    rng = np.random.default_rng(3)
    node_words = np.array([1, 2, 4, 8, 0x10], dtype=np.uint32)
    words = rng.choice(np.array([0, 1, 6, 0x18, 0x1F, 0xFFFFFFFF, 0x20], dtype=np.uint32), size=pts.shape[0])
    plain = sf.expected_sets("five", inst, "bounds")
    # unset node words are all-ones: all-ones point words, and NULL, give the unmasked bytes
    for form in FORMS:
        sf.assert_same(*query(sc, pts, np.full(pts.shape, 0xFFFFFFFF, np.uint32), form), *plain, what="all-ones words")
    sc.SetNodeMasks(node_words)  # (no Commit)
    ref = sf.expected(inst, pts, node_words, words)
    assert ref[0].tobytes() != plain[0].tobytes()
    for form in FORMS:
        sf.assert_same(*query(sc, pts, words, form), *ref, what="a subset per point, %s form" % form)
        sf.assert_same(*query(sc, pts, None, form), *plain, what="NULL: every node")
    # every node hidden: not found
    out, found = query(sc, pts, np.full(pts.shape, 0x20, np.uint32), "device")
    assert not found.any() and (out["node_id"] == sf.MISS).all() and (out["prim_id"] == sf.MISS).all()
    sf.assert_same(out, found, *sf.expected(inst, pts, node_words, np.full(pts.shape, 0x20, np.uint32)), what="every node hidden")
    # a change of the node words, no Commit
    node_words2 = np.array([0x18, 1, 1, 6, 2], dtype=np.uint32)
    sc.SetNodeMasks(node_words2)
    sf.assert_same(*query(sc, pts, words, "host"), *sf.expected(inst, pts, node_words2, words), what="changed node words")
    # the same on the top-level tree path
    inst = sf.scene("twelve")
    sc, _keep2 = make_scene(inst)
    pts = sf.point_sets("twelve", inst)["surface"]
    node_words = (np.uint32(1) << (np.arange(12, dtype=np.uint32) % 5)).astype(np.uint32)
    words = rng.choice(np.array([0, 1, 6, 0x18, 0x1F, 0x20], dtype=np.uint32), size=pts.shape[0])
    sc.SetNodeMasks(node_words)
    for form in FORMS:
        sf.assert_same(*query(sc, pts, words, form), *sf.expected(inst, pts, node_words, words), what="twelve nodes, masked, %s form" % form)


def test_a_stale_scene_is_refused_until_committed_again():
    inst = [tuple(x) for x in sf.scene("two")]
    sc, accels = make_scene(inst)
    pts = sf.tie_points(inst, n=150)
    sf.assert_same(*query(sc, pts), *sf.expected(inst, pts), what="before the refit")
    v, f, m = inst[0]
    moved = (v + np.random.default_rng(9).normal(scale=0.05, size=v.shape)).astype(F32)
    accels[(id(v), id(f))].Refit(moved)
    for form in FORMS:
        with pytest.raises(NrtError) as e:
            query(sc, pts, form=form)
        assert e.value.status == NRT_ERR_INVALID and "commit the scene again" in str(e.value)
    # ... and writes nothing: both forms over pre-filled outputs
    import torch

    n, fill = pts.shape[0], 0xA5
    out, found = np.full((n * 32,), fill, dtype=np.uint8), np.full((n,), fill, dtype=np.uint8)
    assert sc._L.nrtSceneClosestPointBatch_f32(sc._h, pts.ctypes.data, n, None, out.ctypes.data, found.ctypes.data) == NRT_ERR_INVALID
    d_pts = to_device(pts)
    d_out = torch.full((n * 32,), fill, dtype=torch.uint8, device="cuda")
    d_found = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    assert sc._L.nrtSceneClosestPointBatchDevice_f32(sc._h, d_pts.data_ptr(), n, None, d_out.data_ptr(), d_found.data_ptr()) == NRT_ERR_INVALID
    torch.cuda.synchronize()
    assert (out == fill).all() and (found == fill).all() and bool((d_out == fill).all()) and bool((d_found == fill).all())
    assert sc.Commit()
    after = [(moved, f, m), inst[1]]
    for form in FORMS:
        sf.assert_same(*query(sc, pts, form=form), *sf.expected(after, pts), what="after Commit, %s form" % form)


# ---- capped loops: the second piece of the host form's loop, the second trip of the persistent grid ----------------------------------
def _tiled(n):
    inst = sf.scene("two")
    base = np.concatenate([sf.tie_points(inst, n=333), cf.make_points(F32, sf.tie_points(inst, n=130, seed=6)["p"] + F32(0.3), 0.35)])
    ref_out, ref_found = sf.expected(inst, base)
    reps = -(-n // base.shape[0])
    return np.tile(base, reps)[:n], np.tile(ref_out, reps)[:n], np.tile(ref_found, reps)[:n]


def piece_constant():
    src = open(os.path.join(ROOT, "nanort_amd", "csrc", "scene.hip")).read()
    return 1 << int(re.search(r"const uint64_t kSceneClosestPiece = 1ull << (\d+);", src).group(1))


def test_host_form_past_one_staging_piece():
    n = piece_constant() + 777
    pts, ref_out, ref_found = _tiled(n)
    out, found = gpu_scene("two").ClosestPointBatch(pts)
    assert np.array_equal(found, ref_found) and out.tobytes() == ref_out.tobytes()


def test_device_form_past_one_trip_of_the_grid():
    n = 256 * 8 * 256 + 4321  # more points than the persistent grid can have threads (at most 8 blocks of 256 on each of 256 CUs)
    pts, ref_out, ref_found = _tiled(n)
    words = np.full((n,), 3, dtype=np.uint32)
    out, found = query(gpu_scene("two"), pts, words, form="device")
    assert np.array_equal(found, ref_found) and out.tobytes() == ref_out.tobytes()


# ---- refusals: the status, the message, and nothing written ----------------------------------------------------------------------------
def test_refusals_write_nothing():
    import torch

    inst = sf.scene("two")
    sc = gpu_scene("two")
    L, h = sc._L, sc._h
    host, dev = L.nrtSceneClosestPointBatch_f32, L.nrtSceneClosestPointBatchDevice_f32
    n, fill = 130, 0xA5
    pts = sf.tie_points(inst, n=n)
    words = np.full((n,), 0xFFFFFFFF, np.uint32)
    out = np.full((n * 32,), fill, dtype=np.uint8)
    found = np.full((n,), fill, dtype=np.uint8)
    d_pts = to_device(np.concatenate([pts, pts[:1]]))
    d_words = to_device(np.concatenate([words, words[:1]]))
    d_out = torch.full((n * 32 + 32,), fill, dtype=torch.uint8, device="cuda")
    d_found = torch.full((n,), fill, dtype=torch.uint8, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return (out == fill).all() and (found == fill).all() and bool((d_out == fill).all()) and bool((d_found == fill).all())

    # a NULL scene
    assert host(None, pts.ctypes.data, n, None, out.ctypes.data, found.ctypes.data) == NRT_ERR_INVALID
    assert "scene == NULL" in L.nrtSceneLastError(None).decode()
    assert dev(None, d_pts.data_ptr(), n, None, d_out.data_ptr(), d_found.data_ptr()) == NRT_ERR_INVALID
    # a scene that is not committed
    raw, _keep = Scene(), None
    a = BVHAccel(F32)
    assert a.Build(1, TriangleMesh(sf._TRI_V, sf._TRI_F))
    raw.AddNode(a, sf.IDENT)
    assert host(raw._h, pts.ctypes.data, n, None, out.ctypes.data, found.ctypes.data) == NRT_ERR_INVALID
    assert "commit the scene first" in L.nrtSceneLastError(raw._h).decode()
    assert dev(raw._h, d_pts.data_ptr(), n, None, d_out.data_ptr(), d_found.data_ptr()) == NRT_ERR_INVALID
    assert untouched()
    # NULL points or closest_out with points present; too many points
    assert host(h, None, n, None, out.ctypes.data, found.ctypes.data) == NRT_ERR_INVALID
    assert host(h, pts.ctypes.data, n, None, None, found.ctypes.data) == NRT_ERR_INVALID
    assert "NULL points/closest_out" in L.nrtSceneLastError(h).decode()
    assert dev(h, None, n, None, d_out.data_ptr(), d_found.data_ptr()) == NRT_ERR_INVALID
    assert dev(h, d_pts.data_ptr(), n, None, None, d_found.data_ptr()) == NRT_ERR_INVALID
    assert host(h, pts.ctypes.data, 1 << 31, None, out.ctypes.data, found.ctypes.data) == NRT_ERR_INVALID
    assert dev(h, d_pts.data_ptr(), 1 << 31, None, d_out.data_ptr(), d_found.data_ptr()) == NRT_ERR_INVALID
    assert "2^31-1" in L.nrtSceneLastError(h).decode()
    # a device array that is not aligned: 16 bytes for points and closest_out, 4 for the words
    assert dev(h, d_pts.data_ptr() + 4, n, None, d_out.data_ptr(), d_found.data_ptr()) == NRT_ERR_INVALID
    assert dev(h, d_pts.data_ptr(), n, None, d_out.data_ptr() + 8, d_found.data_ptr()) == NRT_ERR_INVALID
    assert "16 bytes" in L.nrtSceneLastError(h).decode()
    assert dev(h, d_pts.data_ptr(), n, d_words.data_ptr() + 2, d_out.data_ptr(), d_found.data_ptr()) == NRT_ERR_INVALID
    assert "4-byte aligned" in L.nrtSceneLastError(h).decode()
    assert untouched()
    # no points: NRT_OK, nothing read or written
    assert host(h, None, 0, None, None, None) == NRT_OK and dev(h, None, 0, None, None, None) == NRT_OK
    assert untouched()
    # found_out may be NULL
    assert host(h, pts.ctypes.data, n, None, out.ctypes.data, None) == NRT_OK
    assert out.tobytes() == sf.expected(inst, pts)[0].tobytes() and (found == fill).all()


def test_python_checks_its_tensors():
    import torch

    sc = gpu_scene("two")
    pts = sf.tie_points(sf.scene("two"), n=130)
    d_out = torch.full((130 * 32,), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        sc.ClosestPointBatchDevice(torch.from_numpy(pts.view(np.uint8).copy()), d_out)
    with pytest.raises(ValueError):
        sc.ClosestPointBatchDevice(to_device(pts), d_out[:-32])
    torch.cuda.synchronize()
    assert bool((d_out == 0x5A).all())
    assert POINT_F32.itemsize == 16

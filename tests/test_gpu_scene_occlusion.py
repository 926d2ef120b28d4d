"""Occlusion queries on instanced scenes (nrtSceneOccludedBatch*, Scene.OccludedBatch*): the flags are exactly the closest-hit
call's and the restatement's (oracle/nanosg_oracle.c), on every path — the fused scan, the listing launches, the pruning walk,
the single-pass walk with its own certificate — on material built to separate them: rays that enter more than 64 boxes with the
only blocker ranked 71st (flag 0) or 61st (flag 1), crowds, coincident copies, axis-parallel rays, 10 000 instances."""
import ctypes

import numpy as np
import pytest

from nanort_amd import BVHAccel, NrtError, Scene, TriangleMesh, capi, scenes
from nanort_amd.wire import RAY_F32, SCENE_HIT_F32
from oracle import bindings as ob
from scene_fixture import instances, xform

pytestmark = pytest.mark.gpu


def check(sc, rays, om, what=None):
    """occluded mask == closest-hit mask == the restatement's."""
    occ = sc.OccludedBatch(rays)
    path = (sc.LastPath(), sc.LastRedone())
    _, m = sc.TraverseBatch(rays)
    assert np.array_equal(occ, m), what
    assert np.array_equal(occ, om), what
    assert 0.05 < om.mean() < 0.95, om.mean()
    return occ, path


def test_five_node_fixture_host_and_device_forms(oracle):
    import torch

    sc = Scene()
    O = ob.SceneOracle(oracle)
    keep = []
    for v, f, x in instances():
        a = BVHAccel(np.float32)
        assert a.Build(f.shape[0], TriangleMesh(v, f))
        keep.append(a)
        sc.AddNode(a, x)
        O.add_node(v, f, x, tree=a.GetTree())
    assert sc.Commit() and O.commit()
    cam = scenes.camera_rays(160, 90)
    away = cam.copy()  # the plane fills the camera's view (99 % of the wave is blocked): the same wave shot backwards misses
    away["dir"] = -away["dir"]
    rays = np.concatenate([cam, away])
    n = rays.shape[0]
    _, om = O.traverse(rays)
    assert om[:cam.shape[0]].mean() > 0.5 > om[cam.shape[0]:].mean()
    occ, _ = check(sc, rays, om)
    # Device form: the same bytes; nothing is written where the closest-hit call writes its records, nor past the n flags
    d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    d_hits = torch.zeros(n * SCENE_HIT_F32.itemsize, dtype=torch.uint8, device="cuda")
    d_mask = torch.full((n + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    sc.TraverseBatchDevice(d_rays, d_hits, d_mask[:n])  # (the record buffer the scene saw last)
    d_hits.fill_(0xA5)
    d_mask.fill_(0xA5)
    sc.OccludedBatchDevice(d_rays, d_mask)
    torch.cuda.synchronize()
    assert d_mask[:n].cpu().numpy().tobytes() == occ.tobytes()
    assert (d_mask[n:] == 0xA5).all().item()
    assert (d_hits == 0xA5).all().item()
    sc.SetTunable("single_pass", 2)  # the walk over a five-leaf top-level tree: at most 64 nodes, a hit ends the ray
    d_mask.fill_(0xA5)
    sc.OccludedBatchDevice(d_rays, d_mask)
    assert sc.LastPath() == 1 and sc.LastRedone() == 0
    assert d_mask[:n].cpu().numpy().tobytes() == occ.tobytes()
    assert (d_mask[n:] == 0xA5).all().item() and (d_hits == 0xA5).all().item()


@pytest.fixture(scope="module")
def small_sphere(oracle):
    sv, sf = scenes.sphere(32, 16)
    sv = (sv - np.array([0, 5, 0], dtype=np.float32)).astype(np.float32)
    nodes, idx, _ = oracle.build(sv, sf)
    a = BVHAccel(np.float32)
    a.SetMesh(TriangleMesh(sv, sf))
    a.SetTree(nodes, idx)
    return sv, sf, a


def small_scene(oracle, small_sphere, count):
    sv, sf, a = small_sphere
    rng = np.random.default_rng(300 + count)
    lo, hi, far = (0.6, 1.2, 1.5) if count == 1 else (0.15, 0.5, 4)  # (a lone node: large and central, or 2 % of the wave hits it)
    xs = [xform(tuple(rng.uniform(lo, hi, 3)), rng.uniform(0, 6.28), rng.uniform(0, 6.28), tuple(rng.uniform(-far, far, 3) + np.array([0, 5, 0])))
          for _ in range(count)]
    O = ob.SceneOracle(oracle)
    for x in xs:
        O.add_node(sv, sf, x)
    assert O.commit()
    rays = scenes.camera_rays(211, 97)  # ragged batch size
    rays["org"] += rng.uniform(-0.2, 0.2, size=(rays.shape[0], 3)).astype(np.float32)
    return a, xs, rays, O.traverse(rays)[1]


@pytest.mark.parametrize("count", [1, 3, 8, 9, 20, 63])
def test_small_scenes_every_listing_form(oracle, small_sphere, count):
    """The fused scan (<= scan_max nodes), the scan in a launch of its own (fuse_scan = 0), the scan raised past the node
    count, the top-level tree forced: the occlusion flags are the closest-hit flags and the restatement's."""
    a, xs, rays, om = small_scene(oracle, small_sphere, count)
    for tun in ({}, {"fuse_scan": 0}, {"scan_max": 64}, {"scan_max": 1}, {"scan_max": 64, "fuse_scan": 0}):
        sc = Scene()
        for k, v in tun.items():
            sc.SetTunable(k, v)
        for x in xs:
            sc.AddNode(a, x)
        assert sc.Commit()
        _, path = check(sc, rays, om, tun)
        assert path == (0, 0), tun


@pytest.mark.parametrize("count", [64, 65])
@pytest.mark.parametrize("single_pass", [0, 2])
def test_the_boundary_of_the_walks_small_scene_shortcut(oracle, small_sphere, count, single_pass):
    """64 nodes: every entered box is listed, the walk ends a ray at its first hit; 65: it has to count."""
    a, xs, rays, om = small_scene(oracle, small_sphere, count)
    sc = Scene()
    sc.SetTunable("single_pass", single_pass)
    for x in xs:
        sc.AddNode(a, x)
    assert sc.Commit()
    _, path = check(sc, rays, om)
    assert path[0] == (1 if single_pass else 0)
    if count == 64:
        assert path[1] == 0


def line_fixture():
    """Mesh A: a unit-cube box whose only triangles are two tiny ones in opposite corners (rays through the middle enter the box
    and miss).  Mesh B: a full (tilted) plane across the cube.  70 A along x, one B behind them, 10 more A."""
    av = np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0], [1, 1, 1], [0.99, 1, 1], [1, 0.99, 1]], dtype=np.float32)
    af = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.uint32)
    bv = np.array([[0.4, 0, 0], [0.6, 1, 0], [0.6, 1, 1], [0.4, 0, 1]], dtype=np.float32)
    bf = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)
    step, x0, y0, z0 = 1.5, -60.0, 4.5, 2.0
    place = [("A", k) for k in range(70)] + [("B", 70)] + [("A", k) for k in range(71, 81)]
    nodes = [(w, xform(trans=(x0 + step * k, y0, z0))) for w, k in place]
    rng = np.random.default_rng(17)

    def shoot(x_from, sign, m):
        r = np.zeros(m, dtype=RAY_F32)
        r["org"][:, 0] = x_from
        r["org"][:, 1] = y0 + rng.uniform(0.3, 0.7, m)
        r["org"][:, 2] = z0 + rng.uniform(0.3, 0.7, m)
        d = np.stack([np.full(m, float(sign)), rng.uniform(-1e-3, 1e-3, m), rng.uniform(-1e-3, 1e-3, m)], axis=1)
        r["dir"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        r["max_t"] = 1.0e30
        return r

    front = shoot(x0 - 1.0, +1, 300)                 # enters all 81 boxes, B ranks 71st: 0
    mid = shoot(x0 + step * 9 + 1.25, +1, 300)       # between the 10th and the 11th A: 60 boxes, then B, 61st: 1
    back = shoot(x0 + step * 81 + 1.0, -1, 300)      # the mirrored set: ten A, then B
    back_mid = shoot(x0 + step * 70 - 0.25, -1, 300)  # from just in front of B backwards: 70 A, no B: 0
    axis = shoot(x0 - 1.0, +1, 60)                   # exactly axis-parallel, some with -0.0 components
    axis["dir"][:, 1:] = 0.0
    axis["dir"][:, 0] = 1.0
    axis["dir"][:20, 1] = -0.0
    axis["org"][30:, 0] = x0 + step * 9 + 1.25
    rays = np.concatenate([front, mid, back, back_mid, axis, scenes.camera_rays(64, 36)])
    return (av, af), (bv, bf), nodes, rays, slice(0, 300), slice(300, 600), (x0, y0, z0, step)


def boxes_entered(rays, geo):
    """How many of the 81 unit boxes of the line a ray enters (float64 slab test; the fixture's rays pass far from any edge)."""
    x0, y0, z0, step = geo
    o, d = rays["org"].astype(np.float64), rays["dir"].astype(np.float64)
    cnt = np.zeros(rays.shape[0], dtype=int)
    for k in range(81):
        lo, hi = np.array([x0 + step * k, y0, z0]), np.array([x0 + step * k + 1, y0 + 1, z0 + 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - o) / d, (hi - o) / d
        tn, tf = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
        cnt += (tn <= tf) & (tf >= 0)
    return cnt


@pytest.mark.parametrize("mode", ["listing", "walk", "pruning_listing"])
def test_the_64_nearest_rule(oracle, monkeypatch, mode):
    """A blocker that ranks 71st among the entered boxes does not occlude; one that ranks 61st does."""
    if mode == "pruning_listing":
        monkeypatch.setenv("NRT_ALLOW_ENV", "1")
        monkeypatch.setenv("NRT_SCENE_PRUNE_MIN", "1")
    (av, af), (bv, bf), nodes, rays, front, mid, geo = line_fixture()
    accel = {}
    for w, (v, f) in (("A", (av, af)), ("B", (bv, bf))):
        a = BVHAccel(np.float32)
        assert a.Build(f.shape[0], TriangleMesh(v, f))
        accel[w] = (v, f, a, a.GetTree())
    sc = Scene()
    O = ob.SceneOracle(oracle)
    for w, x in nodes:
        v, f, a, tree = accel[w]
        sc.AddNode(a, x)
        O.add_node(v, f, x, tree=tree)
    assert sc.Commit() and O.commit()
    _, om = O.traverse(rays)
    # the fixture yields both classes, by the restatement's own flags
    assert (boxes_entered(rays[front], geo) == 81).all()
    assert int((om[front] == 0).sum()) >= 100 and (om[front] == 0).all()  # enters > 64 boxes, B out of reach -> 0
    assert (boxes_entered(rays[mid], geo) == 71).all()
    assert int((om[mid] == 1).sum()) >= 100 and (om[mid] == 1).all()      # B within reach -> 1
    sc.SetTunable("single_pass", 2 if mode == "walk" else 0)
    _, path = check(sc, rays, om)
    if mode == "walk":
        assert path[0] == 1 and 0 < path[1] < len(rays)
    else:
        assert path == (0, 0)


def crowd(oracle):
    rng = np.random.default_rng(21)
    sv, sf = scenes.sphere(12, 6)
    sv = (sv - np.array([0, 5, 0], dtype=np.float32)).astype(np.float32)
    pv, pf = scenes.plane(8, 8)
    pv = pv.copy()
    pv[:, 1] = 0.0
    meshes = []
    for v, f in ((sv, sf), (pv, pf)):
        a = BVHAccel(np.float32)
        assert a.Build(f.shape[0], TriangleMesh(v, f))
        meshes.append((v, f, a, a.GetTree()))
    sc = Scene()
    O = ob.SceneOracle(oracle)

    def add(which, x):
        v, f, a, tree = meshes[which]
        sc.AddNode(a, x)
        O.add_node(v, f, x, tree=tree)

    for k in range(300):
        s = rng.uniform(0.05, 0.35, 3)
        x = xform(tuple(s), rng.uniform(0, 6.28), rng.uniform(0, 6.28), tuple(rng.uniform(-4, 4, 3) + np.array([0, 5, 0])))
        add(0, x)
        if k % 10 == 0:
            add(0, x)  # a coincident copy
    for k in range(6):
        x = xform((0.5, 1, 0.5), 0.3 * (k % 2), 0, (0, 1.0 + k, 0))
        add(1, x)
        add(1, x)  # flat, doubled
    assert sc.Commit() and O.commit()
    return sc, O, rng, meshes


@pytest.mark.parametrize("dir_scale", [1.0, 0.25, 4.0])
def test_crowd_walk_equals_listing_equals_restatement(oracle, dir_scale):
    sc, O, rng, keep = crowd(oracle)
    n = 6000
    rays = np.zeros(n, dtype=RAY_F32)
    org = rng.uniform(-7, 7, size=(n, 3)) + np.array([0, 5, 0])
    tgt = rng.uniform(-4, 4, size=(n, 3)) + np.array([0, 5, 0])
    # Aimed into the crowd, 99 % of the rays are blocked.  So a third is aimed wide (grazing the crowd or past it), a third reaches
    # only 0.1 .. 3 units and a third starts 2 .. 14 units out: the world interval acts on the box listing only, so these rays
    # list few boxes, or none, and yet are blocked wherever a listed instance has a hit at any distance.
    tgt[2::3] = rng.uniform(-10, 10, size=(n // 3, 3)) + np.array([0, 5, 0])
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays["org"] = org.astype(np.float32)
    rays["dir"] = (d * dir_scale).astype(np.float32)
    rays["max_t"] = 3.0e38
    rays["dir"][:50, 0] = 0.0  # axis-parallel
    rays["dir"][50:80, 1] = -0.0
    rays["max_t"][::3] = (rng.uniform(0.1, 3.0, size=n // 3) / dir_scale).astype(np.float32)
    rays["min_t"][1::3] = (rng.uniform(2.0, 14.0, size=n // 3) / dir_scale).astype(np.float32)
    _, om = O.traverse(rays)
    sc.SetTunable("single_pass", 2)
    _, path = check(sc, rays, om)
    assert path[0] == 1 and path[1] < len(rays)
    # the closest-hit back-off is neither consulted nor updated by occlusion calls
    sc.SetTunable("single_pass", 1)
    sc.SetTunable("walk_min", 2)
    sc.SetTunable("walk_backoff_pct", 0)
    sc.TraverseBatch(rays)  # any ray handed over: the next closest-hit calls skip the walk ...
    handed = sc.LastRedone()
    occ = sc.OccludedBatch(rays)
    assert sc.LastPath() == 1 and np.array_equal(occ, om)  # ... an occlusion call does not, and does not end the back-off either
    sc.TraverseBatch(rays)
    assert sc.LastPath() == (0 if handed else 1)
    sc.SetTunable("single_pass", 0)
    _, path0 = check(sc, rays, om)
    assert path0 == (0, 0)
    sc.SetTunable("single_pass", 2)
    for name, value in (("walk_trav_min", 1), ("walk_trav_min", 48), ("walk_refill_min", 1), ("walk_refill_min", 64), ("cand_min", 16)):
        sc.SetTunable(name, value)
        assert np.array_equal(sc.OccludedBatch(rays), om), (name, value)


def test_ten_thousand_instances_default_path(oracle):
    rng = np.random.default_rng(5)
    sv, sf = scenes.sphere(16, 8)
    sv = sv - np.array([0, 5, 0], dtype=np.float32)
    pv, pf = scenes.plane(6, 4)
    pv = (pv - pv.mean(axis=0)).astype(np.float32)
    meshes = []
    for v, f in ((sv, sf), (pv, pf)):
        a = BVHAccel(np.float32)
        assert a.Build(f.shape[0], TriangleMesh(v, f))
        meshes.append((v, f, a, a.GetTree()))
    sc = Scene()
    O = ob.SceneOracle(oracle)
    for k in range(10000):
        v, f, a, tree = meshes[k % 2]
        s = rng.uniform(0.004, 0.02, 3) if k % 2 == 0 else rng.uniform(0.008, 0.03, 3)
        x = xform(tuple(s), rng.uniform(0, 6.28), rng.uniform(0, 6.28), tuple(rng.uniform(-8, 8, 3) + np.array([0, 5, 0])))
        sc.AddNode(a, x)
        O.add_node(v, f, x, tree=tree)
    assert sc.Commit() and O.commit()
    rays = scenes.camera_rays(256, 192)
    rays["org"] += rng.uniform(-0.5, 0.5, size=(rays.shape[0], 3)).astype(np.float32)
    _, om = O.traverse(rays)
    _, path = check(sc, rays, om)
    assert path[0] == 1 and path[1] < len(rays) // 4  # the walk's, and it certified the bulk


def test_lifecycle_and_errors(oracle):
    L = capi.lib()
    v, f = scenes.sphere(24, 12)
    a = BVHAccel(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    sc = Scene()
    sc.AddNode(a, np.eye(4))
    sc.AddNode(a, xform(trans=(2.5, 0, 0)))
    rays = scenes.camera_rays(64, 48)
    mask = np.zeros(rays.shape[0], dtype=np.uint8)
    rp, mp = rays.ctypes.data_as(ctypes.c_void_p), mask.ctypes.data_as(ctypes.c_void_p)
    n = rays.shape[0]
    for fn in (L.nrtSceneOccludedBatch_f32, L.nrtSceneOccludedBatchDevice_f32):
        assert fn(None, rp, n, mp) == capi.NRT_ERR_INVALID
        assert fn(sc._h, rp, n, mp) == capi.NRT_ERR_INVALID  # not committed
        assert b"commit the scene first" in L.nrtSceneLastError(sc._h)
    with pytest.raises(NrtError):
        sc.OccludedBatch(rays)
    assert sc.Commit()
    for fn in (L.nrtSceneOccludedBatch_f32, L.nrtSceneOccludedBatchDevice_f32):
        assert fn(sc._h, None, n, mp) == capi.NRT_ERR_INVALID
        assert fn(sc._h, rp, n, None) == capi.NRT_ERR_INVALID
        assert fn(sc._h, None, 0, None) == capi.NRT_OK
        assert fn(sc._h, rp, 1 << 31, mp) == capi.NRT_ERR_INVALID  # more rays than the closest-hit call accepts
    assert L.nrtSceneTraverseBatch_f32(sc._h, rp, 1 << 31, mp, mp) == capi.NRT_ERR_INVALID

    def restated(vv, ff):
        O = ob.SceneOracle(oracle)
        O.add_node(vv, ff, np.eye(4, dtype=np.float32), tree=a.GetTree())
        O.add_node(vv, ff, xform(trans=(2.5, 0, 0)), tree=a.GetTree())
        assert O.commit()
        return O.traverse(rays)

    oh, om = restated(v, f)
    assert 0.05 < om.mean() < 0.95
    # shared scratch does not leak state: occlusion, closest hit, occlusion — each equals the restatement
    assert np.array_equal(sc.OccludedBatch(rays), om)
    h, m = sc.TraverseBatch(rays)
    assert np.array_equal(m, om) and h.tobytes() == oh.tobytes()
    assert np.array_equal(sc.OccludedBatch(rays), om)
    h, m = sc.TraverseBatch(rays)
    assert np.array_equal(m, om) and h.tobytes() == oh.tobytes()
    # a refit mesh: refused until committed again, then the new flags
    v2 = (v * np.array([1.0, 0.5, 1.0], dtype=np.float32) + np.array([0, 2.0, 0], dtype=np.float32)).astype(np.float32)
    a.Refit(v2)
    with pytest.raises(NrtError, match="commit the scene again"):
        sc.OccludedBatch(rays)
    assert L.nrtSceneOccludedBatchDevice_f32(sc._h, rp, n, mp) == capi.NRT_ERR_INVALID
    assert sc.Commit()
    oh2, om2 = restated(v2, f)
    assert not np.array_equal(om2, om)
    assert np.array_equal(sc.OccludedBatch(rays), om2)
    # a rebuilt mesh: the same
    v3, f3 = scenes.sphere(16, 8)
    assert a.Build(f3.shape[0], TriangleMesh(v3, f3))
    with pytest.raises(NrtError, match="commit the scene again"):
        sc.OccludedBatch(rays)
    assert sc.Commit()
    oh3, om3 = restated(v3, f3)
    assert np.array_equal(sc.OccludedBatch(rays), om3)
    h, m = sc.TraverseBatch(rays)
    assert np.array_equal(m, om3) and h.tobytes() == oh3.tobytes()


def test_embree_occluded_sets_geomid_only():
    """rtcOccluded1M: geomID = 0 exactly on the rays rtcIntersect1M reports a hit for; tfar, u, v, primID, instID keep their
    input bits."""
    import os

    import embree_fixture as ef

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    E = ctypes.CDLL(os.path.join(root, "nanort_amd", "lib", "libnanort_embree.so"))
    vp, u32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
    E.rtcNewDevice.restype, E.rtcNewDevice.argtypes = vp, [ctypes.c_char_p]
    E.rtcDeleteDevice.argtypes = [vp]
    E.rtcDeviceGetError.restype, E.rtcDeviceGetError.argtypes = ctypes.c_int, [vp]
    E.rtcDeviceNewScene.restype, E.rtcDeviceNewScene.argtypes = vp, [vp, ctypes.c_int, ctypes.c_int]
    E.rtcCommit.argtypes = [vp]
    E.rtcNewTriangleMesh.restype, E.rtcNewTriangleMesh.argtypes = u32, [vp, ctypes.c_int, sz, sz, sz]
    E.rtcMapBuffer.restype, E.rtcMapBuffer.argtypes = vp, [vp, u32, ctypes.c_int]
    E.rtcUnmapBuffer.argtypes = [vp, u32, ctypes.c_int]
    E.rtcIntersect1M.argtypes = [vp, vp, vp, sz, sz]
    E.rtcOccluded1M.argtypes = [vp, vp, vp, sz, sz]
    INDEX, VERTEX = 0x01000000, 0x02000000
    dev = E.rtcNewDevice(None)
    scn = E.rtcDeviceNewScene(dev, 0, 1)
    for v, f in ef.meshes():
        gid = E.rtcNewTriangleMesh(scn, 0, f.shape[0], v.shape[0], 1)
        vb = np.ctypeslib.as_array(ctypes.cast(E.rtcMapBuffer(scn, gid, VERTEX), ctypes.POINTER(ctypes.c_float)), (v.shape[0], 4))
        ib = np.ctypeslib.as_array(ctypes.cast(E.rtcMapBuffer(scn, gid, INDEX), ctypes.POINTER(ctypes.c_int32)), (f.shape[0], 3))
        vb[:, :3] = v
        vb[:, 3] = 0.0
        ib[:] = f.astype(np.int32)
        E.rtcUnmapBuffer(scn, gid, VERTEX)
        E.rtcUnmapBuffer(scn, gid, INDEX)
    E.rtcCommit(scn)
    assert E.rtcDeviceGetError(dev) == 0
    r = ef.rays()
    n = r.shape[0]
    src = np.frombuffer(b"\xa5" * (96 * n), dtype=ef.RTC_RAY).copy()
    src["org"], src["dir"], src["tnear"], src["tfar"] = r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7]
    a, b = src.copy(), src.copy()
    E.rtcIntersect1M(scn, None, a.ctypes.data, n, 96)
    E.rtcOccluded1M(scn, None, b.ctypes.data, n, 96)
    assert E.rtcDeviceGetError(dev) == 0
    hit = a["geomID"] != ef.INVALID
    assert 0.05 < hit.mean() < 0.95
    assert (b["geomID"][hit] == 0).all() and (b["geomID"][~hit] == 0xA5A5A5A5).all()
    for name in ("tfar", "u", "v", "primID", "instID", "org", "dir", "tnear", "Ng", "time", "mask"):
        assert b[name].tobytes() == src[name].tobytes(), name
    E.rtcDeleteDevice(dev)

"""Instance visibility masks on scenes (nrtSceneSetNodeMasks, nrtScene*BatchMasked*, Scene.*Masked*): an instance exists for a ray
iff (node word & ray word) != 0, and every field of every record is that of the restatement on the scene of the visible nodes
(tests/scene_masks_fixture.py), on every kernel family — the fused scan, the listing launches, the pruning walk, the single-pass
walk in both forms.  Ray words are interleaved by ray index, so every wave mixes visible sets.  The line fixture is the case an
implementation fails that lists a hidden instance and skips it when reached: there a hidden instance must take no place among
the 64 nearest."""
import ctypes

import numpy as np
import pytest

from nanort_amd import BVHAccel, NrtError, Scene, TriangleMesh, capi, scenes
from nanort_amd.wire import RAY_F32, SCENE_HIT_F32
from oracle import bindings as ob
from scene_fixture import instances, xform
from scene_masks_fixture import ALL, LINE_B, check_line_table, expect_masked, line_node_masks, line_ray_words, scene_nodes
from test_gpu_scene_occlusion import crowd, line_fixture, small_scene, small_sphere  # noqa: F401 (small_sphere: a fixture)

pytestmark = pytest.mark.gpu

WORDS = np.array([ALL, 0, 1, 2, 4, 8], dtype=np.uint32)


def interleaved(n, words=WORDS):
    return np.ascontiguousarray(words[np.arange(n) % len(words)])


def check_masked(sc, rays, words, eh, em, what=None):
    """Masked closest hit == the expectation in every byte; masked occlusion flags == masked closest-hit flags == the expectation."""
    h, m = sc.TraverseBatchMasked(rays, words)
    path = (sc.LastPath(), sc.LastRedone())
    assert np.array_equal(m, em), what
    assert h.tobytes() == eh.tobytes(), what
    occ = sc.OccludedBatchMasked(rays, words)
    assert np.array_equal(occ, m), what
    return h, m, path


def hit_share_per_word(em, words):
    for w in np.unique(words):
        share = em[words == w].mean()
        if w == 0:
            assert share == 0.0
        else:
            assert 0.0 < share < 1.0, (hex(int(w)), share)


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
    rays = scenes.camera_rays(211, 97)
    n = rays.shape[0]
    h0, m0 = sc.TraverseBatch(rays)
    occ0 = sc.OccludedBatch(rays)
    ones = np.full(n, ALL, dtype=np.uint32)

    def same_as_unmasked(what):
        for rw in (None, ones):
            h, m = sc.TraverseBatchMasked(rays, rw)
            assert h.tobytes() == h0.tobytes() and m.tobytes() == m0.tobytes(), what
            assert sc.OccludedBatchMasked(rays, rw).tobytes() == occ0.tobytes(), what

    same_as_unmasked("no node masks")
    sc.SetNodeMasks(np.full(5, ALL, dtype=np.uint32))
    same_as_unmasked("all-ones node masks")
    # the plane (node 0) hidden from bit 0
    masks = np.full(5, ALL, dtype=np.uint32)
    masks[0] &= ~np.uint32(1)
    sc.SetNodeMasks(masks)
    same_as_unmasked("all-ones ray words see every node that keeps a bit")
    words = interleaved(n, np.array([ALL, 1, 0], dtype=np.uint32))
    eh, em = expect_masked(oracle, scene_nodes(O), masks, rays, words)
    assert (h0["node_id"][words == 1] == 0).mean() > 0.5 and (eh["node_id"][words == 1] != 0).all()  # camera rays lose the plane
    hit_share_per_word(em, words)
    h, m, _ = check_masked(sc, rays, words, eh, em)
    # Device forms: the same bytes, nothing written past the n records / n flags; the occlusion form leaves the records alone
    rec = SCENE_HIT_F32.itemsize
    d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    d_words = torch.from_numpy(words.view(np.int32)).cuda()
    d_hits = torch.full((n * rec + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    d_mask = torch.full((n + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    for single_pass in (1, 2):  # the fused scan; the walk over a five-leaf top-level tree
        sc.SetTunable("single_pass", single_pass)
        d_hits.fill_(0xA5)
        d_mask.fill_(0xA5)
        sc.TraverseBatchMaskedDevice(d_rays, d_words, d_hits, d_mask)
        torch.cuda.synchronize()
        assert sc.LastPath() == (1 if single_pass == 2 else 0)
        assert d_hits[:n * rec].cpu().numpy().tobytes() == eh.tobytes()
        assert d_mask[:n].cpu().numpy().tobytes() == em.tobytes()
        assert (d_hits[n * rec:] == 0xA5).all().item() and (d_mask[n:] == 0xA5).all().item()
        d_hits.fill_(0xA5)
        d_mask.fill_(0xA5)
        sc.OccludedBatchMaskedDevice(d_rays, d_words, d_mask)
        torch.cuda.synchronize()
        assert d_mask[:n].cpu().numpy().tobytes() == em.tobytes()
        assert (d_mask[n:] == 0xA5).all().item() and (d_hits == 0xA5).all().item()
        # NULL words on the device: every ray all ones
        sc.TraverseBatchMaskedDevice(d_rays, None, d_hits, d_mask)
        torch.cuda.synchronize()
        assert d_hits[:n * rec].cpu().numpy().tobytes() == h0.tobytes() and d_mask[:n].cpu().numpy().tobytes() == m0.tobytes()


def random_nibbles(rng, count):
    """Random 4-bit node words (0 included: a node nobody sees), every bit kept by at least one node."""
    masks = rng.integers(0, 16, size=count).astype(np.uint32)
    for b in range(4):
        if not (masks & (1 << b)).any():
            masks[rng.integers(0, count)] |= np.uint32(1 << b)
    return masks


def small_case(oracle, small_sphere, count):
    sv, sf, a = small_sphere
    a, xs, rays, _ = small_scene(oracle, small_sphere, count)
    tree = a.GetTree()
    nodes = [(sv, sf, x, tree) for x in xs]
    masks = random_nibbles(np.random.default_rng(900 + count), count)
    words = interleaved(rays.shape[0])
    eh, em = expect_masked(oracle, nodes, masks, rays, words)
    hit_share_per_word(em, words)
    return a, xs, rays, masks, words, eh, em


@pytest.mark.parametrize("count", [1, 3, 8, 9, 20, 63])
def test_small_scenes_every_listing_form(oracle, small_sphere, count):
    """The fused scan, the scan in a launch of its own, the scan raised past the node count, the top-level tree forced."""
    a, xs, rays, masks, words, eh, em = small_case(oracle, small_sphere, count)
    for tun in ({}, {"fuse_scan": 0}, {"scan_max": 64}, {"scan_max": 1}, {"scan_max": 64, "fuse_scan": 0}):
        sc = Scene()
        for k, v in tun.items():
            sc.SetTunable(k, v)
        for x in xs:
            sc.AddNode(a, x)
        sc.SetNodeMasks(masks)  # (before Commit)
        assert sc.Commit()
        _, _, path = check_masked(sc, rays, words, eh, em, tun)
        assert path == (0, 0), tun


@pytest.mark.parametrize("count", [64, 65])
@pytest.mark.parametrize("single_pass", [0, 2])
def test_the_boundary_of_the_walks_small_scene_shortcut(oracle, small_sphere, count, single_pass):
    a, xs, rays, masks, words, eh, em = small_case(oracle, small_sphere, count)
    sc = Scene()
    sc.SetTunable("single_pass", single_pass)
    for x in xs:
        sc.AddNode(a, x)
    assert sc.Commit()
    sc.SetNodeMasks(masks)  # (after Commit)
    _, _, path = check_masked(sc, rays, words, eh, em)
    assert path[0] == (1 if single_pass else 0)
    occ = sc.OccludedBatchMasked(rays, words)
    assert sc.LastPath() == (1 if single_pass else 0) and np.array_equal(occ, em)
    if count == 64:
        assert sc.LastRedone() == 0


@pytest.mark.parametrize("mode", ["listing", "walk", "pruning_listing"])
def test_hidden_instances_take_no_place_among_the_64_nearest(oracle, monkeypatch, mode):
    if mode == "pruning_listing":
        monkeypatch.setenv("NRT_ALLOW_ENV", "1")
        monkeypatch.setenv("NRT_SCENE_PRUNE_MIN", "1")
    (av, af), (bv, bf), nodes, rays, front, mid, _ = line_fixture()
    accel = {}
    for w, (v, f) in (("A", (av, af)), ("B", (bv, bf))):
        a = BVHAccel(np.float32)
        assert a.Build(f.shape[0], TriangleMesh(v, f))
        accel[w] = (v, f, a, a.GetTree())
    sc = Scene()
    spec = []
    for w, x in nodes:
        v, f, a, tree = accel[w]
        sc.AddNode(a, x)
        spec.append((v, f, x, tree))
    assert sc.Commit()
    masks = line_node_masks()
    sc.SetNodeMasks(masks)
    words = line_ray_words(rays.shape[0], front, mid)
    eh, em = expect_masked(oracle, spec, masks, rays, words)
    check_line_table(em, words, front, mid)
    sc.SetTunable("single_pass", 2 if mode == "walk" else 0)
    h, m, path = check_masked(sc, rays, words, eh, em)
    check_line_table(m, words, front, mid)
    assert (h["node_id"][front][m[front] == 1] == LINE_B).all()
    if mode == "walk":
        assert path[0] == 1
        sc.OccludedBatchMasked(rays, words)
        assert sc.LastPath() == 1
    else:
        assert path == (0, 0)


@pytest.mark.parametrize("dir_scale", [1.0, 0.25])
def test_crowd_walk_equals_listing_equals_expectation(oracle, dir_scale):
    sc, O, rng, keep = crowd(oracle)
    nodes = scene_nodes(O)
    n = 6000
    rays = np.zeros(n, dtype=RAY_F32)
    org = rng.uniform(-7, 7, size=(n, 3)) + np.array([0, 5, 0])
    tgt = rng.uniform(-4, 4, size=(n, 3)) + np.array([0, 5, 0])
    tgt[2::3] = rng.uniform(-10, 10, size=(n // 3, 3)) + np.array([0, 5, 0])  # a third aimed wide
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays["org"] = org.astype(np.float32)
    rays["dir"] = (d * dir_scale).astype(np.float32)
    rays["max_t"] = 3.0e38
    rays["dir"][:50, 0] = 0.0  # axis-parallel
    rays["dir"][50:80, 1] = -0.0
    rays["max_t"][::3] = (rng.uniform(0.1, 3.0, size=n // 3) / dir_scale).astype(np.float32)
    rays["min_t"][1::3] = (rng.uniform(2.0, 14.0, size=n // 3) / dir_scale).astype(np.float32)
    masks = np.full(len(nodes), ALL, dtype=np.uint32)
    for b in range(4):  # each of four bits is absent from a random half of the instances
        masks[rng.random(len(nodes)) < 0.5] &= ~np.uint32(1 << b)
    sc.SetNodeMasks(masks)
    words = interleaved(n)
    eh, em = expect_masked(oracle, nodes, masks, rays, words)
    hit_share_per_word(em, words)
    assert len(nodes) >= 64  # the default rule (walk_min) sends this scene through the walk
    for single_pass in (2, 1, 0):
        sc.SetTunable("single_pass", single_pass)
        h, m = sc.TraverseBatchMasked(rays, words)
        if single_pass:
            assert sc.LastPath() == 1 and sc.LastRedone() < n, single_pass
        else:
            assert (sc.LastPath(), sc.LastRedone()) == (0, 0)
        assert np.array_equal(m, em) and h.tobytes() == eh.tobytes(), single_pass
        occ = sc.OccludedBatchMasked(rays, words)
        assert sc.LastPath() == (1 if single_pass else 0)
        assert np.array_equal(occ, em), single_pass


def two_spheres(oracle):
    v, f = scenes.sphere(24, 12)
    a = BVHAccel(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    xs = [np.eye(4, dtype=np.float32), xform(trans=(2.5, 0, 0))]
    sc = Scene()
    for x in xs:
        sc.AddNode(a, x)
    return sc, a, v, f, xs


def test_lifecycle(oracle):
    sc, a, v, f, xs = two_spheres(oracle)
    rays = scenes.camera_rays(64, 48)
    n = rays.shape[0]
    words = interleaved(n, np.array([ALL, 1, 2, 0], dtype=np.uint32))

    def expected(masks, xforms=xs):
        return expect_masked(oracle, [(v, f, x, a.GetTree()) for x in xforms], masks, rays, words)

    assert sc.Commit()
    h0, m0 = sc.TraverseBatch(rays)
    assert 0.05 < m0.mean() < 0.95
    # a change after Commit, with no Commit: the next query answers for the new words
    seen = []
    for masks in (np.array([1, 2], dtype=np.uint32), np.array([2, 1], dtype=np.uint32), np.array([3, 0], dtype=np.uint32)):
        sc.SetNodeMasks(masks)
        eh, em = expected(masks)
        h, m = sc.TraverseBatchMasked(rays, words)
        assert h.tobytes() == eh.tobytes() and m.tobytes() == em.tobytes(), masks
        assert np.array_equal(sc.OccludedBatchMasked(rays, words), em), masks
        seen.append(eh.tobytes())
    assert len(set(seen)) == 3  # (the three settings do differ)
    # nrtSceneCommit keeps the masks
    masks = np.array([1, 2], dtype=np.uint32)
    sc.SetNodeMasks(masks)
    assert sc.Commit()
    eh, em = expected(masks)
    h, m = sc.TraverseBatchMasked(rays, words)
    assert h.tobytes() == eh.tobytes() and m.tobytes() == em.tobytes()
    # a node added after SetNodeMasks is visible to every non-zero word
    x3 = xform(trans=(-2.5, 0.5, 0))
    sc.AddNode(a, x3)
    assert sc.Commit()
    masks3 = np.array([1, 2, ALL], dtype=np.uint32)
    eh, em = expected(masks3, xs + [x3])
    h, m = sc.TraverseBatchMasked(rays, words)
    assert h.tobytes() == eh.tobytes() and m.tobytes() == em.tobytes()
    assert (eh["node_id"][words == 1] == 2).any() and (eh["node_id"][words == 2] == 2).any()
    # unmasked calls ignore node masks entirely: identical bytes before and after masks that hide everything
    hu, mu = sc.TraverseBatch(rays)
    ou = sc.OccludedBatch(rays)
    sc.SetNodeMasks(np.zeros(3, dtype=np.uint32))
    h, m = sc.TraverseBatchMasked(rays, words)
    assert not m.any() and (h["node_id"] == ALL).all() and (h["t"] == rays["max_t"]).all()
    assert not sc.OccludedBatchMasked(rays, None).any()
    h, m = sc.TraverseBatch(rays)
    assert h.tobytes() == hu.tobytes() and m.tobytes() == mu.tobytes() and sc.OccludedBatch(rays).tobytes() == ou.tobytes()
    # SetNodeMasks(None) restores the unmasked bytes
    sc.SetNodeMasks(None)
    h, m = sc.TraverseBatchMasked(rays, None)
    assert h.tobytes() == hu.tobytes() and m.tobytes() == mu.tobytes()
    assert sc.OccludedBatchMasked(rays, np.full(n, ALL, dtype=np.uint32)).tobytes() == ou.tobytes()


def test_refusals(oracle):
    import torch

    L = capi.lib()
    sc, a, v, f, xs = two_spheres(oracle)
    rays = scenes.camera_rays(64, 48)
    n = rays.shape[0]
    words = interleaved(n)
    hits = np.frombuffer(b"\xa5" * (n * SCENE_HIT_F32.itemsize), dtype=SCENE_HIT_F32).copy()
    mask = np.full(n, 0xA5, dtype=np.uint8)
    rp, wp, hp, mp = (x.ctypes.data_as(ctypes.c_void_p) for x in (rays, words, hits, mask))
    trav = (L.nrtSceneTraverseBatchMasked_f32, L.nrtSceneTraverseBatchMaskedDevice_f32)
    occl = (L.nrtSceneOccludedBatchMasked_f32, L.nrtSceneOccludedBatchMaskedDevice_f32)

    def untouched():
        return (hits.view(np.uint8) == 0xA5).all() and (mask == 0xA5).all()

    def refused(st, text):
        assert st == capi.NRT_ERR_INVALID
        assert text in L.nrtSceneLastError(sc._h), L.nrtSceneLastError(sc._h)
        assert untouched()

    # the setter: count must equal the number of nodes added so far; nothing changes otherwise
    two = np.array([1, 2], dtype=np.uint32)
    assert L.nrtSceneSetNodeMasks(None, two.ctypes.data_as(ctypes.c_void_p), 2) == capi.NRT_ERR_INVALID
    for bad in (1, 3):
        refused(L.nrtSceneSetNodeMasks(sc._h, np.zeros(3, dtype=np.uint32).ctypes.data_as(ctypes.c_void_p), bad), b"nrtSceneSetNodeMasks")
    with pytest.raises(NrtError):
        sc.SetNodeMasks(np.zeros(5, dtype=np.uint32))
    # an uncommitted scene
    for fn in trav:
        assert fn(None, rp, wp, n, hp, mp) == capi.NRT_ERR_INVALID
        refused(fn(sc._h, rp, wp, n, hp, mp), b"commit the scene first")
    for fn in occl:
        assert fn(None, rp, wp, n, mp) == capi.NRT_ERR_INVALID
        refused(fn(sc._h, rp, wp, n, mp), b"commit the scene first")
    with pytest.raises(NrtError):
        sc.TraverseBatchMasked(rays, words)
    assert sc.Commit()
    # the refused setter calls above changed nothing: every node is still all ones
    hu, mu = sc.TraverseBatch(rays)
    h, m = sc.TraverseBatchMasked(rays, None)
    assert h.tobytes() == hu.tobytes() and m.tobytes() == mu.tobytes()
    # NULL rays / outputs, too many rays; zero rays are fine
    for fn in trav:
        refused(fn(sc._h, None, wp, n, hp, mp), b"NULL")
        refused(fn(sc._h, rp, wp, n, None, mp), b"NULL")
        refused(fn(sc._h, rp, wp, 1 << 31, hp, mp), b"too many rays")
        assert fn(sc._h, None, None, 0, None, None) == capi.NRT_OK
    for fn in occl:
        refused(fn(sc._h, None, wp, n, mp), b"NULL")
        refused(fn(sc._h, rp, wp, n, None), b"NULL")
        refused(fn(sc._h, rp, wp, 1 << 31, mp), b"too many rays")
        assert fn(sc._h, None, None, 0, None) == capi.NRT_OK
    # a misaligned d_ray_masks (Device forms): refused before anything is read or written
    d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    d_words = torch.zeros(4 * n + 8, dtype=torch.uint8, device="cuda")
    d_hits = torch.full((n * SCENE_HIT_F32.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    d_mask = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    for off in (1, 2, 3):
        refused(trav[1](sc._h, d_rays.data_ptr(), d_words.data_ptr() + off, n, d_hits.data_ptr(), d_mask.data_ptr()), b"4-byte aligned")
        refused(occl[1](sc._h, d_rays.data_ptr(), d_words.data_ptr() + off, n, d_mask.data_ptr()), b"4-byte aligned")
    torch.cuda.synchronize()
    assert (d_hits == 0xA5).all().item() and (d_mask == 0xA5).all().item()
    # a stale mesh context: refused until the scene is committed again
    v2 = (v * np.array([1.0, 0.5, 1.0], dtype=np.float32)).astype(np.float32)
    a.Refit(v2)
    for fn in trav:
        refused(fn(sc._h, rp, wp, n, hp, mp), b"commit the scene again")
    for fn in occl:
        refused(fn(sc._h, rp, wp, n, mp), b"commit the scene again")
    with pytest.raises(NrtError, match="commit the scene again"):
        sc.OccludedBatchMasked(rays, words)
    assert sc.Commit()
    masks = np.array([1, 2], dtype=np.uint32)
    sc.SetNodeMasks(masks)
    eh, em = expect_masked(oracle, [(v2, f, x, a.GetTree()) for x in xs], masks, rays, words)
    h, m = sc.TraverseBatchMasked(rays, words)
    assert h.tobytes() == eh.tobytes() and m.tobytes() == em.tobytes()

"""Per-ray skip (node, primitive) pairs on scenes (nrtSceneQueryBatch*, Scene.QueryBatch*): a ray whose pair is (p, n) does not see
primitive p of node n, and every field of every record is that of the restatement with that one face collapsed for that one ray
(tests/scene_query_fixture.py) — on every kernel family: the fused scan, the listing launches, the single-pass walk in both forms
and with both leaf phases, and the listing path over the rays the walk hands over.  The waves are bounce waves: rays that start ON
the triangle they name, consecutive rays naming different triangles of different nodes, so every wave mixes pairs and a lane that
is refilled gets another pair.  After each closest-hit check the OCCLUSION flags must equal the closest-hit flags."""
import ctypes

import numpy as np
import pytest

from nanort_amd import BVHAccel, NrtError, Scene, TriangleMesh, capi, scenes
from nanort_amd.wire import RAY_F32, SCENE_HIT_F32
from oracle import bindings as ob
from scene_fixture import instances, xform
from scene_masks_fixture import ALL, scene_nodes
from scene_query_fixture import bounce_wave, expect_query, own_pair_share, pairs_of, stacked_planes
from test_gpu_scene_masks import interleaved, random_nibbles
from test_gpu_scene_occlusion import crowd, small_scene, small_sphere  # noqa: F401 (small_sphere: a fixture)

pytestmark = pytest.mark.gpu

REC = SCENE_HIT_F32.itemsize


def check_query(sc, rays, pairs, eh, em, words=None, what=None):
    """SKIP closest hit == the expectation in every byte; the OCCLUSION flags of the same descriptor == the closest-hit flags."""
    h, m = sc.QueryBatch(rays, ray_masks=words, skip_pairs=pairs)
    path = (sc.LastPath(), sc.LastRedone())
    assert np.array_equal(m, em), what
    assert h.tobytes() == eh.tobytes(), what
    occ = sc.QueryBatch(rays, ray_masks=words, skip_pairs=pairs, occlusion=True)
    assert np.array_equal(occ, m), what
    return h, m, path


def five_nodes(oracle):
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
    return sc, O, keep


def five_node_bounce(O, limit=6000, seed=5):
    """A bounce wave from the CPU primary wave; every fifth ray carries a pair that skips nothing, so valid and invalid pairs and
    the five nodes are interleaved ray by ray."""
    rays = scenes.camera_rays(211, 97)
    oh, om = O.traverse(rays)
    b, pairs, records = bounce_wave(rays, oh, om, np.random.default_rng(seed), limit=limit)
    k = np.arange(b.shape[0])
    records["prim_id"][k % 5 == 1] = ALL
    records["node_id"][k % 10 == 6] = 5 + k[k % 10 == 6] % 3
    return b, pairs_of(records), records


def test_five_node_fixture_host_and_device_forms_records_and_packed_pairs(oracle):
    import torch

    sc, O, keep = five_nodes(oracle)
    nodes = scene_nodes(O)
    b, pairs, records = five_node_bounce(O)
    n = b.shape[0]
    assert n >= 5000 and n % 64 != 0
    uh, um = O.traverse(b)
    eh, em = expect_query(oracle, nodes, b, pairs, committed=O)
    assert own_pair_share(uh, um, pairs) >= 0.3 and own_pair_share(eh, em, pairs) == 0.0 and 0.05 < em.mean() < 0.95
    assert (eh["node_id"][em == 1] != 0).any() and (eh["node_id"][em == 1] == 0).any()
    # host form: packed pairs (stride 8), and the previous wave's records as they lie (stride 20): identical results
    check_query(sc, b, pairs, eh, em, what="packed")
    assert (sc.LastPath(), sc.LastRedone()) == (0, 0)  # five nodes: the fused scan
    check_query(sc, b, records, eh, em, what="records")
    # Device form, both layouts, on the fused scan and on the walk over a five-leaf top-level tree
    d_rays = torch.from_numpy(b.view(np.uint8)).cuda()
    d_pairs = torch.from_numpy(pairs.view(np.int32)).cuda()
    d_records = torch.from_numpy(records.view(np.uint8).copy()).cuda()
    d_hits = torch.full((n * REC + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    d_mask = torch.full((n + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    for single_pass in (1, 2):
        sc.SetTunable("single_pass", single_pass)
        for d_skip in (d_pairs, d_records):
            d_hits.fill_(0xA5)
            d_mask.fill_(0xA5)
            sc.QueryBatchDevice(d_rays, d_hits, d_mask, skip_pairs=d_skip)
            torch.cuda.synchronize()
            assert sc.LastPath() == (1 if single_pass == 2 else 0)
            assert d_hits[:n * REC].cpu().numpy().tobytes() == eh.tobytes()
            assert d_mask[:n].cpu().numpy().tobytes() == em.tobytes()
            assert (d_hits[n * REC:] == 0xA5).all().item() and (d_mask[n:] == 0xA5).all().item()
            d_hits.fill_(0xA5)
            d_mask.fill_(0xA5)
            sc.QueryBatchDevice(d_rays, None, d_mask, skip_pairs=d_skip, occlusion=True)
            torch.cuda.synchronize()
            assert d_mask[:n].cpu().numpy().tobytes() == em.tobytes()
            assert (d_mask[n:] == 0xA5).all().item() and (d_hits == 0xA5).all().item()
        assert d_records.cpu().numpy().tobytes() == records.tobytes()  # the pairs are read, never written
        check_query(sc, b, records, eh, em, what=single_pass)


def small_case(oracle, small_sphere, count):
    sv, sf, a = small_sphere
    a, xs, rays, _ = small_scene(oracle, small_sphere, count)
    tree = a.GetTree()
    nodes = [(sv, sf, x, tree) for x in xs]
    O = ob.SceneOracle(oracle)
    for v, f, x, t in nodes:
        O.add_node(v, f, x, tree=t)
    assert O.commit()
    oh, om = O.traverse(rays)
    b, pairs, records = bounce_wave(rays, oh, om, np.random.default_rng(700 + count), limit=3000)
    assert b.shape[0] >= (300 if count > 1 else 150)
    uh, um = O.traverse(b)
    eh, em = expect_query(oracle, nodes, b, pairs, committed=O)
    assert own_pair_share(uh, um, pairs) >= 0.3 and own_pair_share(eh, em, pairs) == 0.0 and eh.tobytes() != uh.tobytes()
    return a, xs, b, pairs, records, eh, em


@pytest.mark.parametrize("count", [1, 8, 9, 63])
def test_small_scenes_every_listing_form(oracle, small_sphere, count):
    """The fused scan, the scan in a launch of its own, the scan raised past the node count, the top-level tree forced."""
    a, xs, b, pairs, records, eh, em = small_case(oracle, small_sphere, count)
    for tun in ({}, {"fuse_scan": 0}, {"scan_max": 64}, {"scan_max": 1}, {"scan_max": 64, "fuse_scan": 0}):
        sc = Scene()
        for k, v in tun.items():
            sc.SetTunable(k, v)
        for x in xs:
            sc.AddNode(a, x)
        assert sc.Commit()
        _, _, path = check_query(sc, b, records if count % 2 else pairs, eh, em, what=tun)
        assert path == (0, 0), tun


@pytest.mark.parametrize("count", [64, 65])
@pytest.mark.parametrize("single_pass", [0, 2])
def test_the_boundary_of_the_walks_small_scene_shortcut(oracle, small_sphere, count, single_pass):
    a, xs, b, pairs, records, eh, em = small_case(oracle, small_sphere, count)
    sc = Scene()
    sc.SetTunable("single_pass", single_pass)
    for x in xs:
        sc.AddNode(a, x)
    assert sc.Commit()
    _, _, path = check_query(sc, b, pairs, eh, em)
    assert path[0] == (1 if single_pass else 0)
    occ = sc.QueryBatch(b, skip_pairs=records, occlusion=True)
    assert sc.LastPath() == (1 if single_pass else 0) and np.array_equal(occ, em)
    if count == 64:
        assert sc.LastRedone() == 0


def crowd_primary(rng, n=6000):
    rays = np.zeros(n, dtype=RAY_F32)
    org = rng.uniform(-7, 7, size=(n, 3)) + np.array([0, 5, 0])
    tgt = rng.uniform(-4, 4, size=(n, 3)) + np.array([0, 5, 0])
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays["org"] = org.astype(np.float32)
    rays["dir"] = d.astype(np.float32)
    rays["max_t"] = 3.0e38
    return rays


def crowd_bounce(O, rng, dir_scale):
    rays = crowd_primary(rng)
    oh, om = O.traverse(rays)
    b, pairs, records = bounce_wave(rays, oh, om, rng, dir_scale=dir_scale, limit=3000)
    assert 2500 <= b.shape[0] <= 3000
    return b, pairs, records


@pytest.mark.parametrize("dir_scale", [1.0, 0.25])
def test_crowd_walk_equals_listing_equals_expectation(oracle, dir_scale):
    """310 + 12 instances of two meshes, coincident copies among them.  Direction vectors of length 0.25 make the reference's cull
    fire early, which the walk cannot certify: those rays go through `redo`, the listing path over a subset, with their pairs."""
    sc, O, rng, keep = crowd(oracle)
    nodes = scene_nodes(O)
    b, pairs, records = crowd_bounce(O, rng, dir_scale)
    n = b.shape[0]
    uh, um = O.traverse(b)
    eh, em = expect_query(oracle, nodes, b, pairs, committed=O)
    assert own_pair_share(uh, um, pairs) >= 0.3 and own_pair_share(eh, em, pairs) == 0.0 and 0.05 < em.mean() < 0.999
    assert len(nodes) >= 64
    for leaf_items in (1, 0):
        sc.SetTunable("walk_leaf_items", leaf_items)
        for single_pass in (2, 1, 0):
            sc.SetTunable("single_pass", single_pass)
            _, _, path = check_query(sc, b, records if leaf_items else pairs, eh, em, what=(leaf_items, single_pass))
            if single_pass == 2:
                assert path[0] == 1 and path[1] < n
                if dir_scale == 0.25:
                    assert path[1] > 0  # the redo path carried the skip
            elif single_pass == 0:
                assert path == (0, 0)
            occ = sc.QueryBatch(b, skip_pairs=pairs, occlusion=True)
            if single_pass != 1:
                assert sc.LastPath() == (1 if single_pass else 0)
            assert np.array_equal(occ, em), (leaf_items, single_pass)


@pytest.mark.parametrize("single_pass", [1, 2], ids=["listing", "walk"])
def test_stacked_planes_name_the_next_copy_of_the_same_mesh(oracle, single_pass):
    """Three instances of ONE mesh context: (p, 0) leaves face p of nodes 1 and 2 alone.  Comparing the primitive id alone misses."""
    (pv, pf), xs, rays, pairs = stacked_planes(np.random.default_rng(11))
    a = BVHAccel(np.float32)
    assert a.Build(pf.shape[0], TriangleMesh(pv, pf))
    sc = Scene()
    sc.SetTunable("single_pass", single_pass)
    for x in xs:
        sc.AddNode(a, x)
    assert sc.Commit()
    nodes = [(pv, pf, x, a.GetTree()) for x in xs]
    eh, em = expect_query(oracle, nodes, rays, pairs)
    assert em.all() and (eh["node_id"] == 1).all() and np.array_equal(eh["prim_id"], pairs[:, 0])
    h, m, path = check_query(sc, rays, pairs, eh, em)
    assert path[0] == (1 if single_pass == 2 else 0)
    assert (h["node_id"] == 1).all() and np.array_equal(h["prim_id"], pairs[:, 0])
    uh, um = sc.TraverseBatch(rays)
    assert own_pair_share(uh, um, pairs) > 0.0  # unskipped, some of these rays stop on the face they start on


def test_skip_and_masked_on_the_five_node_fixture(oracle):
    sc, O, keep = five_nodes(oracle)
    nodes = scene_nodes(O)
    b, pairs, records = five_node_bounce(O, limit=4000, seed=6)
    n = b.shape[0]
    masks = random_nibbles(np.random.default_rng(43), 5)  # (as in the masks tests: 4-bit node words; this seed leaves one node at 0)
    assert (masks == 0).sum() == 1
    sc.SetNodeMasks(masks)
    words = interleaved(n)
    eh, em = expect_query(oracle, nodes, b, pairs, masks, words)
    uh, um = expect_query(oracle, nodes, b, None, masks, words)
    assert eh.tobytes() != uh.tobytes() and own_pair_share(eh, em, pairs) == 0.0 and not em[words == 0].any()
    assert all(em[words == w].any() for w in (ALL, 1, 2, 4, 8))
    # MASKED | SKIP with ray_masks == NULL: every ray carries all ones, and the node words still count
    ones = np.full(n, ALL, dtype=np.uint32)
    eh1, em1 = expect_query(oracle, nodes, b, pairs, masks, ones)
    for single_pass in (1, 2):
        sc.SetTunable("single_pass", single_pass)
        _, _, path = check_query(sc, b, records, eh, em, words=words, what=single_pass)
        assert path[0] == (1 if single_pass == 2 else 0)
        check_query(sc, b, pairs, eh1, em1, words=ones, what=single_pass)
        hits = np.zeros(n, dtype=SCENE_HIT_F32)
        mask = np.full(n, 0xA5, dtype=np.uint8)
        flags = capi.NRT_SCENE_QUERY_MASKED | capi.NRT_SCENE_QUERY_SKIP
        assert raw_query(sc, flags, b, None, pairs, 8, hits, mask) == capi.NRT_OK
        assert hits.tobytes() == eh1.tobytes() and mask.tobytes() == em1.tobytes(), single_pass
        mask[:] = 0xA5
        assert raw_query(sc, flags | capi.NRT_SCENE_QUERY_OCCLUSION, b, None, records.ctypes.data + 12, REC, None, mask) == capi.NRT_OK
        assert mask.tobytes() == em1.tobytes(), single_pass


def test_skip_and_masked_on_the_crowd(oracle):
    sc, O, rng, keep = crowd(oracle)
    nodes = scene_nodes(O)
    b, pairs, records = crowd_bounce(O, rng, 0.25)
    n = b.shape[0]
    masks = random_nibbles(np.random.default_rng(33), len(nodes)) | np.uint32(0xF0)
    masks[rng.random(len(nodes)) < 0.5] &= ~np.uint32(0xF0)
    sc.SetNodeMasks(masks)
    words = interleaved(n)
    eh, em = expect_query(oracle, nodes, b, pairs, masks, words)
    uh, um = expect_query(oracle, nodes, b, None, masks, words)
    assert eh.tobytes() != uh.tobytes() and 0.05 < em.mean() < 0.95
    for single_pass in (2, 0):
        sc.SetTunable("single_pass", single_pass)
        _, _, path = check_query(sc, b, pairs, eh, em, words=words, what=single_pass)
        assert path[0] == (1 if single_pass else 0)
    # a SKIP query without MASKED never reads the node words: the unmasked skip expectation
    eh0, em0 = expect_query(oracle, nodes, b, pairs, committed=O)
    check_query(sc, b, pairs, eh0, em0)
    sc.SetTunable("single_pass", 2)
    check_query(sc, b, pairs, eh0, em0)


def raw_query(sc, flags, rays, words, pairs, stride, hits, mask, device=False, struct_size=None, reserved=0, n=None, scene=True):
    L = capi.lib()
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
    q = capi.SceneQuery(ctypes.sizeof(capi.SceneQuery) if struct_size is None else struct_size, flags, ptr(rays),
                        rays.shape[0] if n is None else n, ptr(words), ptr(pairs), stride, reserved, ptr(hits), ptr(mask))
    fn = L.nrtSceneQueryBatchDevice_f32 if device else L.nrtSceneQueryBatch_f32
    return fn(sc._h if scene else None, ctypes.addressof(q))


def test_routing_a_descriptor_without_skip_is_the_existing_call(oracle):
    sc, O, rng, keep = crowd(oracle)
    b, pairs, records = crowd_bounce(O, rng, 0.25)
    n = b.shape[0]
    masks = random_nibbles(np.random.default_rng(34), len(O.nodes))
    sc.SetNodeMasks(masks)
    words = interleaved(n)
    invalid = pairs.copy()
    invalid[0::3, 0] = ALL
    invalid[1::3, 1] = ALL
    invalid[2::3, 1] += np.uint32(len(O.nodes))
    OCC, MSK, SKP = capi.NRT_SCENE_QUERY_OCCLUSION, capi.NRT_SCENE_QUERY_MASKED, capi.NRT_SCENE_QUERY_SKIP
    for single_pass in (2, 0):
        sc.SetTunable("single_pass", single_pass)
        existing = {
            0: lambda: sc.TraverseBatch(b),
            OCC: lambda: (None, sc.OccludedBatch(b)),
            MSK: lambda: sc.TraverseBatchMasked(b, words),
            MSK | OCC: lambda: (None, sc.OccludedBatchMasked(b, words)),
        }
        for flags, call in existing.items():
            h0, m0 = call()
            path0 = (sc.LastPath(), sc.LastRedone())
            if single_pass == 2 and not flags & OCC:
                assert path0[1] > 0
            # without SKIP (the pair fields are then not read: garbage in them), and with SKIP and no array
            for fl, pp, stride in ((flags, 0x10, 3), (flags | SKP, None, 0)):
                hits = np.zeros(n, dtype=SCENE_HIT_F32)
                mask = np.full(n, 0xA5, dtype=np.uint8)
                assert raw_query(sc, fl, b, words, pp, stride, None if flags & OCC else hits, mask) == capi.NRT_OK
                assert (sc.LastPath(), sc.LastRedone()) == path0, (flags, fl)
                assert mask.tobytes() == m0.tobytes(), (flags, fl)
                if not flags & OCC:
                    assert hits.tobytes() == h0.tobytes(), (flags, fl)
            # SKIP with pairs that skip nothing: the unskipped bytes
            r = sc.QueryBatch(b, ray_masks=words if flags & MSK else None, skip_pairs=invalid, occlusion=bool(flags & OCC))
            if flags & OCC:
                assert r.tobytes() == m0.tobytes(), flags
            else:
                assert r[0].tobytes() == h0.tobytes() and r[1].tobytes() == m0.tobytes(), flags
    # the Python wrapper routes the same way
    h0, m0 = sc.TraverseBatch(b)
    h, m = sc.QueryBatch(b)
    assert h.tobytes() == h0.tobytes() and m.tobytes() == m0.tobytes()
    assert sc.QueryBatch(b, occlusion=True).tobytes() == sc.OccludedBatch(b).tobytes()


def two_planes(oracle):
    pv, pf = scenes.plane(12, 6)
    a = BVHAccel(np.float32)
    assert a.Build(pf.shape[0], TriangleMesh(pv, pf))
    xs = [xform(trans=(0, 0, 0)), xform(trans=(0, 0, 3.0))]
    sc = Scene()
    for x in xs:
        sc.AddNode(a, x)
    return sc, a, pv, pf, xs


def test_lifecycle(oracle):
    (pv, pf), _, rays, pairs = stacked_planes(np.random.default_rng(12), count=500)
    sc, a, pv, pf, xs = two_planes(oracle)
    assert sc.Commit()
    nodes = [(pv, pf, x, a.GetTree()) for x in xs]
    eh, em = expect_query(oracle, nodes, rays, pairs)
    assert (eh["node_id"] == 1).all()
    check_query(sc, rays, pairs, eh, em)
    # after nrtSceneSetNodeMasks (no new Commit): node 1 hidden from bit 0 — those rays skip their own face and then miss
    masks = np.array([ALL, ALL & ~1], dtype=np.uint32)
    sc.SetNodeMasks(masks)
    words = interleaved(rays.shape[0], np.array([ALL, 1], dtype=np.uint32))
    eh2, em2 = expect_query(oracle, nodes, rays, pairs, masks, words)
    assert not em2[words == 1].any() and em2[words == ALL].all()
    check_query(sc, rays, pairs, eh2, em2, words=words)
    check_query(sc, rays, pairs, eh, em)  # the query without MASKED ignores the node words
    # a mesh rebuild makes the scene stale: refused, nothing written, until it is committed again
    pv2 = (pv * np.array([1.0, 1.0, 0.5], dtype=np.float32)).astype(np.float32)
    assert a.Build(pf.shape[0], TriangleMesh(pv2, pf))
    hits = np.frombuffer(b"\xa5" * (rays.shape[0] * REC), dtype=SCENE_HIT_F32).copy()
    mask = np.full(rays.shape[0], 0xA5, dtype=np.uint8)
    st = raw_query(sc, capi.NRT_SCENE_QUERY_SKIP, rays, None, pairs, 8, hits, mask)
    assert st == capi.NRT_ERR_INVALID and b"commit the scene again" in capi.lib().nrtSceneLastError(sc._h)
    assert (hits.view(np.uint8) == 0xA5).all() and (mask == 0xA5).all()
    with pytest.raises(NrtError, match="commit the scene again"):
        sc.QueryBatch(rays, skip_pairs=pairs, occlusion=True)
    assert sc.Commit()
    rays2 = rays.copy()
    rays2["org"][:, 2] *= np.float32(0.5)  # the start points follow the squashed mesh (0.5 * z is exact)
    nodes2 = [(pv2, pf, x, a.GetTree()) for x in xs]
    eh3, em3 = expect_query(oracle, nodes2, rays2, pairs)
    assert (eh3["node_id"] == 1).all() and eh3.tobytes() != eh.tobytes()
    sc.SetNodeMasks(None)
    check_query(sc, rays2, pairs, eh3, em3)


def test_refusals(oracle):
    import torch

    L = capi.lib()
    (pv, pf), _, rays, pairs = stacked_planes(np.random.default_rng(13), count=300)
    sc, a, pv, pf, xs = two_planes(oracle)
    n = rays.shape[0]
    words = interleaved(n)
    hits = np.frombuffer(b"\xa5" * (n * REC), dtype=SCENE_HIT_F32).copy()
    mask = np.full(n, 0xA5, dtype=np.uint8)
    OCC, MSK, SKP = capi.NRT_SCENE_QUERY_OCCLUSION, capi.NRT_SCENE_QUERY_MASKED, capi.NRT_SCENE_QUERY_SKIP

    def refused(st, text):
        assert st == capi.NRT_ERR_INVALID
        assert text in L.nrtSceneLastError(sc._h), L.nrtSceneLastError(sc._h)
        assert (hits.view(np.uint8) == 0xA5).all() and (mask == 0xA5).all()

    for device in (False, True):
        # a NULL scene or descriptor
        assert raw_query(sc, SKP, rays, None, pairs, 8, hits, mask, device=device, scene=False) == capi.NRT_ERR_INVALID
        fn = L.nrtSceneQueryBatchDevice_f32 if device else L.nrtSceneQueryBatch_f32
        refused(fn(sc._h, None), b"descriptor == NULL")
    # an uncommitted scene
    refused(raw_query(sc, SKP, rays, None, pairs, 8, hits, mask), b"commit the scene first")
    assert sc.Commit()
    # the descriptor itself
    refused(raw_query(sc, SKP, rays, None, pairs, 8, hits, mask, struct_size=56), b"struct_size")
    refused(raw_query(sc, SKP, rays, None, pairs, 8, hits, mask, struct_size=0), b"struct_size")
    refused(raw_query(sc, SKP | 8, rays, None, pairs, 8, hits, mask), b"unknown flag bits")
    refused(raw_query(sc, 1 << 31, rays, None, pairs, 8, hits, mask), b"unknown flag bits")
    refused(raw_query(sc, SKP, rays, None, pairs, 8, hits, mask, reserved=1), b"reserved")
    # NULL rays, the kind's output missing, too many rays; zero rays are fine
    refused(raw_query(sc, SKP, None, None, pairs, 8, hits, mask, n=n), b"NULL")
    refused(raw_query(sc, SKP, rays, None, pairs, 8, None, mask), b"NULL")
    refused(raw_query(sc, SKP | OCC, rays, None, pairs, 8, hits, None), b"NULL")
    refused(raw_query(sc, SKP | MSK, rays, words, pairs, 8, hits, mask, n=1 << 31), b"too many rays")
    assert raw_query(sc, SKP, None, None, None, 0, None, None, n=0) == capi.NRT_OK
    # the stride: a pair is 8 bytes of 4-byte words
    for stride in (0, 4, 7, 9, 10, 22):
        refused(raw_query(sc, SKP, rays, None, pairs, stride, hits, mask), b"skip_stride_bytes")
        refused(raw_query(sc, SKP | OCC | MSK, rays, words, pairs, stride, None, mask), b"skip_stride_bytes")
    # ... which is not read without SKIP, or without an array
    assert raw_query(sc, 0, rays, None, pairs, 7, hits, mask) == capi.NRT_OK
    assert raw_query(sc, SKP, rays, None, None, 7, hits, mask) == capi.NRT_OK
    h0, m0 = sc.TraverseBatch(rays)
    assert hits.tobytes() == h0.tobytes() and mask.tobytes() == m0.tobytes()
    hits.view(np.uint8)[:] = 0xA5
    mask[:] = 0xA5
    # Device form: misaligned pairs or words; pairs that overlap an output
    d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    d_words = torch.zeros(4 * n + 8, dtype=torch.uint8, device="cuda")
    d_pairs = torch.full((8 * n + 8,), 0xFF, dtype=torch.uint8, device="cuda")
    d_hits = torch.full((n * REC + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    d_mask = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    R, W, P, H, M = (t.data_ptr() for t in (d_rays, d_words, d_pairs, d_hits, d_mask))
    for off in (1, 2, 3):
        refused(raw_query(sc, SKP, R, None, P + off, 8, H, M, device=True, n=n), b"skip_pairs is not 4-byte aligned")
        refused(raw_query(sc, SKP | OCC, R, None, P + off, 8, None, M, device=True, n=n), b"skip_pairs is not 4-byte aligned")
        refused(raw_query(sc, SKP | MSK, R, W + off, P, 8, H, M, device=True, n=n), b"4-byte aligned")
    # the records being written as the pairs (the natural mistake), a range that ends inside hits_out, one that starts in its last
    # record, one inside mask_out; a range that ends exactly where an output begins is fine
    refused(raw_query(sc, SKP, R, None, H + 12, REC, H, M, device=True, n=n), b"overlaps hits_out")
    refused(raw_query(sc, SKP, R, None, H - 8 * n + 8, 8, H, M, device=True, n=n), b"overlaps hits_out")
    refused(raw_query(sc, SKP, R, None, H + n * REC - 4, 8, H, M, device=True, n=n), b"overlaps hits_out")
    assert n % 4 == 0
    refused(raw_query(sc, SKP, R, None, M + n - 4, 8, H, M, device=True, n=n), b"overlaps mask_out")
    refused(raw_query(sc, SKP | OCC, R, None, M, 8, None, M, device=True, n=n), b"overlaps mask_out")
    torch.cuda.synchronize()
    assert (d_hits == 0xA5).all().item() and (d_mask == 0xA5).all().item()
    # with OCCLUSION hits_out is not read: pairs taken from the buffer it names are no overlap
    d_prev = torch.from_numpy(np.ascontiguousarray(np.zeros(n, dtype=SCENE_HIT_F32)).view(np.uint8)).cuda()
    assert raw_query(sc, SKP | OCC, R, None, d_prev.data_ptr() + 12, REC, d_prev.data_ptr(), M, device=True, n=n) == capi.NRT_OK
    # pairs that end exactly where hits_out begins: no overlap
    d_both = torch.full((8 * n + n * REC,), 0xFF, dtype=torch.uint8, device="cuda")
    B = d_both.data_ptr()
    assert raw_query(sc, SKP, R, None, B, 8, B + 8 * n, M, device=True, n=n) == capi.NRT_OK
    torch.cuda.synchronize()
    assert d_both[8 * n:].cpu().numpy().tobytes() == h0.tobytes() and (d_both[:8 * n] == 0xFF).all().item()

"""The end of a launch at the pinned default (tail_quad = 4) and around it: waves that enter the four-lanes-to-a-ray tail (traverse.hip)
with ONE TO FOUR rays — at the top of the loop on their first trip (batches of 1 .. 4 rays) or through the inner-node loop's extra
exit with finished, unwritten results in their idle lanes (5, 17, 65, 129 rays) — under thresholds 1, 2, 3 and the default beside
5, 8 and 16, for bounce and shadow waves, launches over two batches, per-ray skip ids, the rejecting options, leaves of more than
sixteen records and stacks that start beyond the LDS depth and cross it in both directions.  The same small batches are the leaf
phase's smallest inputs: with leaf items (walk_dev.h leaf_items_one_trip, its owner / record arrays addressed as LDS) one to four
owners share a trip.  Every comparison is bit for bit on every field, against the same accelerator with the tail off
(tail_quad = 0) and, where the oracle covers the case, against the restated reference on the same node array."""
import numpy as np
import pytest

from helpers import assert_hits_identical, deep_stack_case, first_leaf_stack_bound
from nanort_amd import BVHAccel, TriangleMesh, scenes
from nanort_amd.wire import default_build_options, default_trace_options

pytestmark = pytest.mark.gpu

DEFAULT = 4
FIRST_TRIP = (1, 2, 3, 4)  # out of rays at the first refill with at most four live lanes
EXTRA_EXIT = (5, 17, 65, 129)  # the main loop first
SIZES = FIRST_TRIP + EXTRA_EXIT
FEW = (1, 2, 3, DEFAULT)  # a wave enters the tail with at most four rays
MANY = (5, 8, 16)  # ... with up to sixteen
THRESHOLDS = FEW + MANY


@pytest.fixture(scope="module")
def plane():
    v, f = scenes.plane(120, 80)
    a = BVHAccel(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    fresh = a.GetTunable("tail_quad")
    rays1 = scenes.camera_rays(160, 90)
    a.SetTunable("tail_quad", 0)
    h, m = a.TraverseBatch(rays1)
    bounce = scenes.secondary_rays("bounce", v, f, rays1, h, m)
    shadow = scenes.secondary_rays("shadow", v, f, rays1, h, m)
    off = {"primary": (h, m), "bounce": a.TraverseBatch(bounce), "shadow": a.TraverseBatch(shadow), "occluded": a.OccludedBatch(shadow)}
    a.SetTunable("tail_quad", fresh)
    return v, f, a, rays1, bounce, shadow, off, fresh


def test_batch_sizes_and_thresholds(oracle, plane):
    v, f, a, rays1, bounce, shadow, off, fresh = plane
    assert fresh == DEFAULT
    nodes, idx = a.GetTree()
    try:
        for name, rays in (("primary", rays1), ("bounce", bounce)):
            want_h, want_m = off[name]
            oh, om = oracle.traverse(nodes, idx, v, f, rays[: max(SIZES)])
            assert_hits_identical(oh, om, want_h[: max(SIZES)], want_m[: max(SIZES)])
            assert want_m[: max(SIZES)].any()
            for tq in (0,) + THRESHOLDS:
                a.SetTunable("tail_quad", tq)
                for k in SIZES:
                    h, m = a.TraverseBatch(rays[:k])
                    assert_hits_identical(want_h[:k], want_m[:k], h, m)
                    assert a.LastKernelName().endswith("<float, 12, false, 0, true, false, 4, 2>"), a.LastKernelName()
    finally:
        a.SetTunable("tail_quad", fresh)


def test_waves_that_never_enter_the_tail(plane):
    """Every ray misses at its first step: the live count goes from all to none and the loop is left through its own exit."""
    v, f, a, rays1, bounce, shadow, off, fresh = plane
    away = rays1[:70].copy()
    away["dir"] = -away["dir"]
    try:
        for k in (3, 70):
            a.SetTunable("tail_quad", 0)
            h0, m0 = a.TraverseBatch(away[:k])
            assert not m0.any() and np.array_equal(h0["t"], away["max_t"][:k]) and (h0["prim_id"] == 0xFFFFFFFF).all()
            for tq in THRESHOLDS:
                a.SetTunable("tail_quad", tq)
                h, m = a.TraverseBatch(away[:k])
                assert_hits_identical(h0, m0, h, m)
    finally:
        a.SetTunable("tail_quad", fresh)


def test_bounce_and_shadow_waves(oracle, plane):
    v, f, a, rays1, bounce, shadow, off, fresh = plane
    nodes, idx = a.GetTree()
    oh, om = oracle.traverse(nodes, idx, v, f, shadow[::7])
    assert_hits_identical(oh, om, off["shadow"][0][::7], off["shadow"][1][::7])
    assert np.array_equal(off["occluded"], off["shadow"][1])
    try:
        for tq in THRESHOLDS:
            a.SetTunable("tail_quad", tq)
            for name, rays in (("bounce", bounce), ("shadow", shadow)):
                h, m = a.TraverseBatch(rays)
                assert_hits_identical(off[name][0], off[name][1], h, m)
            assert np.array_equal(off["occluded"], a.OccludedBatch(shadow))  # the any-hit query
            for k in SIZES:
                assert np.array_equal(off["occluded"][:k], a.OccludedBatch(shadow[:k]))
    finally:
        a.SetTunable("tail_quad", fresh)


def _dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()


def test_one_launch_over_two_batches(plane):
    """40 + 3 rays, the second batch an any-hit query: one wave holds both, so the rays it finishes belong to different batches."""
    import torch

    v, f, a, rays1, bounce, shadow, off, fresh = plane

    def launch():
        d_h = torch.zeros(40 * 16, dtype=torch.uint8, device="cuda")
        d_m0 = torch.zeros(40, dtype=torch.uint8, device="cuda")
        d_m1 = torch.full((3,), 9, dtype=torch.uint8, device="cuda")
        a.TraverseBatchesDevice([(_dev(bounce[100:140]), d_h, d_m0, 40), (_dev(shadow[200:203]), None, d_m1, 3, "occlusion")])
        torch.cuda.synchronize()
        return d_h.cpu().numpy().view(off["bounce"][0].dtype), d_m0.cpu().numpy(), d_m1.cpu().numpy()

    try:
        a.SetTunable("tail_quad", 0)
        h0, m0, occ0 = launch()
        assert_hits_identical(off["bounce"][0][100:140], off["bounce"][1][100:140], h0, m0)
        assert np.array_equal(occ0, off["occluded"][200:203])
        for tq in THRESHOLDS:
            a.SetTunable("tail_quad", tq)
            h, m, occ = launch()
            assert_hits_identical(h0, m0, h, m)
            assert np.array_equal(occ0, occ)
    finally:
        a.SetTunable("tail_quad", fresh)


def test_per_ray_skip_ids(plane):
    """Every bounce ray skips the triangle its primary hit (its own id: neighbours carry different ones), alone and as the first batch
    of a two-batch launch whose second batch has no ids."""
    v, f, a, rays1, bounce, shadow, off, fresh = plane
    n = bounce.shape[0]
    hit1 = off["primary"][1] == 1
    ids = np.where(hit1, off["primary"][0]["prim_id"], 0xFFFFFFFF).astype(np.uint32)[:n]
    again = rays1[:n]  # the primaries once more, each skipping what it hit: the id matters for every ray that hit
    try:
        a.SetTunable("tail_quad", 0)
        want = {k: a.TraverseBatch(again[:k], skip_prim_ids=ids[:k]) for k in SIZES + (n,)}
        hit = hit1[:n]
        assert hit.any() and (want[n][0]["prim_id"][hit] != off["primary"][0]["prim_id"][:n][hit]).all()
        two0 = a.TraverseBatches([again[:40], (shadow[:3], "occlusion")], skip_prim_ids=[ids[:40], None])
        assert_hits_identical(want[n][0][:40], want[n][1][:40], two0[0][0], two0[0][1])
        for tq in THRESHOLDS:
            a.SetTunable("tail_quad", tq)
            for k in SIZES + (n,):
                h, m = a.TraverseBatch(again[:k], skip_prim_ids=ids[:k])
                assert_hits_identical(want[k][0], want[k][1], h, m)
                assert "false, false, 4, 2>" in a.LastKernelName()
            two = a.TraverseBatches([again[:40], (shadow[:3], "occlusion")], skip_prim_ids=[ids[:40], None])
            assert_hits_identical(two0[0][0], two0[0][1], two[0][0], two[0][1])
            assert np.array_equal(two0[1][1], two[1][1])
    finally:
        a.SetTunable("tail_quad", fresh)


def test_rejecting_options(plane):
    """Back-face culling and a primitive-id range: the twin of the kernel that keeps the id tests."""
    v, f, a, rays1, bounce, shadow, off, fresh = plane
    o = default_trace_options()
    o["prim_ids_range"] = (1000, 15000)
    o["skip_prim_id"] = 5000
    o["cull_back_face"] = 1
    try:
        for rays in (rays1, bounce):
            a.SetTunable("tail_quad", 0)
            want_h, want_m = a.TraverseBatch(rays, o)
            assert "false, false, 4, 2>" in a.LastKernelName()
            for tq in THRESHOLDS:
                a.SetTunable("tail_quad", tq)
                for k in SIZES + (rays.shape[0],):
                    h, m = a.TraverseBatch(rays[:k], o)
                    assert_hits_identical(want_h[:k], want_m[:k], h, m)
    finally:
        a.SetTunable("tail_quad", fresh)


def test_wide_leaves(oracle, plane):
    """min_leaf_primitives = 20: leaves of more than sixteen records — several trips of a quad with a remainder, the owners' loop in
    the main walk.  Such a tree does not take leaf items: the kernel is the `…, 4, 0>` one."""
    v, f, a0, rays1, bounce, shadow, off, fresh = plane
    b = BVHAccel(np.float32)
    bo = default_build_options()
    bo["min_leaf_primitives"] = 20
    assert b.Build(f.shape[0], TriangleMesh(v, f), bo)
    bn, bi = b.GetTree()
    counts = bn["data"][bn["flag"] != 0, 0]
    assert int(counts.max()) > 16 and any(int(c) % 4 for c in counts) and any(int(c) % 16 for c in counts)
    for rays in (rays1[:3000], bounce[:3000]):
        b.SetTunable("tail_quad", 0)
        want_h, want_m = b.TraverseBatch(rays)
        assert b.LastKernelName().endswith(", 4, 0>"), b.LastKernelName()
        oh, om = oracle.traverse(bn, bi, v, f, rays[: max(SIZES)])
        assert_hits_identical(oh, om, want_h[: max(SIZES)], want_m[: max(SIZES)])
        for tq in THRESHOLDS:
            b.SetTunable("tail_quad", tq)
            for k in SIZES + (rays.shape[0],):
                h, m = b.TraverseBatch(rays[:k])
                assert_hits_identical(want_h[:k], want_m[:k], h, m)
                assert b.LastKernelName().endswith(", 4, 0>")


def test_deep_stack_crosses_the_lds_depth(oracle):
    """tests/test_gpu_tail_quad.py's pile (every box hit, every step pushes three entries; first_leaf_stack_bound beyond the twelve LDS
    entries), in batches of one to four rays: the tail makes the whole walk, so a ray's stack grows past the LDS depth into the
    spill arrays, comes back below it and passes it again.  A batch of 200 reaches the tail with its stacks already beyond."""
    v, f, dup, nt, rays = deep_stack_case()
    a = BVHAccel(np.float32)
    bo = default_build_options()
    bo["min_leaf_primitives"] = 1
    assert a.Build(f.shape[0], TriangleMesh(v, f), bo)
    nodes, idx = a.GetTree()
    assert (nodes["bmin"][:, :2].max(axis=0) < -0.3).all() and (nodes["bmax"][:, :2].min(axis=0) > 0.3).all()
    assert first_leaf_stack_bound(nodes) > 12
    a.SetTunable("tail_quad", 0)
    want_h, want_m = a.TraverseBatch(rays[:200])
    assert want_m.all()
    oh, om = oracle.traverse(nodes, idx, v, f, rays[:200])
    assert_hits_identical(oh, om, want_h, want_m)
    for tq in THRESHOLDS:
        a.SetTunable("tail_quad", tq)
        for k in FIRST_TRIP + (5, 17, 200):
            h, m = a.TraverseBatch(rays[:k])
            assert_hits_identical(want_h[:k], want_m[:k], h, m)


def test_ten_launches_back_to_back(plane):
    import torch

    v, f, a, rays1, bounce, shadow, off, fresh = plane
    want_h, want_m = off["bounce"]
    assert a.GetTunable("tail_quad") == DEFAULT
    d_rays = _dev(bounce)
    rsz = bounce.dtype.itemsize
    sizes = [bounce.shape[0], 1, 2, 4099, 3, 4, 1003, 5, 129, 17]
    outs = []
    for n in sizes:  # one stream, nothing waited for in between
        d_h = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        d_m = torch.zeros(n, dtype=torch.uint8, device="cuda")
        a.TraverseBatchDevice(d_rays[: n * rsz], d_h, d_m)
        outs.append((d_h, d_m))
    torch.cuda.synchronize()
    for n, (d_h, d_m) in zip(sizes, outs):
        assert_hits_identical(want_h[:n], want_m[:n], d_h.cpu().numpy().view(want_h.dtype), d_m.cpu().numpy())

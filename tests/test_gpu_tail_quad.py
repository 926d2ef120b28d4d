"""Tunable tail_quad (traverse.hip "four lanes to a ray"): a wave of the fp32 two-level triangle walk that is out of rays and holds at
most `tail_quad` live lanes moves live ray q to quad q (ds_bpermute; the stack stays in its owner's column) and finishes the rays with
lane j testing box j of a record / record i + j of a leaf, DPP quad permutes combining the results.  Same tests on the same operands,
accepted in the same sequence: every field of every record must be BIT-IDENTICAL to the walk with the switch off (tail_quad = 0) and,
where the oracle covers the case, to the restated reference's on the same node array."""
import numpy as np
import pytest

from helpers import assert_hits_identical, deep_stack_case, first_leaf_stack_bound
from nanort_amd import BVHAccel, TriangleMesh, scenes
from nanort_amd.wire import default_build_options, default_trace_options

pytestmark = pytest.mark.gpu

THRESHOLDS = (1, 4, 16)


def sweep(a, fn):
    """fn() with the switch off, then at every threshold: [(threshold, result), ...]; the switch is left off."""
    out = []
    for tq in (0,) + THRESHOLDS:
        a.SetTunable("tail_quad", tq)
        out.append((tq, fn()))
    a.SetTunable("tail_quad", 0)
    return out


def assert_sweep_identical(a, rays, opt=None):
    res = sweep(a, lambda: a.TraverseBatch(rays, opt))
    (_, (h0, m0)) = res[0]
    for tq, (h, m) in res[1:]:
        assert_hits_identical(h0, m0, h, m)
    return h0, m0


@pytest.fixture(scope="module")
def plane():
    v, f = scenes.plane(120, 80)
    a = BVHAccel(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    rays1 = scenes.camera_rays(160, 90)
    h, m = a.TraverseBatch(rays1)
    bounce = scenes.secondary_rays("bounce", v, f, rays1, h, m)
    shadow = scenes.secondary_rays("shadow", v, f, rays1, h, m)
    return v, f, a, rays1, bounce, shadow


def test_batch_sizes(oracle, c1_mesh):
    """A batch below one wave is tail from its first step; 63 / 64 / 65 straddle a wave, 300 a block; the 96 x 64 view fills a few."""
    v, f = c1_mesh
    a = BVHAccel(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    rays = scenes.camera_rays(96, 64)
    for n in (1, 5, 63, 64, 65, 300, rays.shape[0]):
        h0, m0 = assert_sweep_identical(a, rays[:n])
    assert a.LastKernelName().endswith(", 4, 2>")
    nodes, idx = a.GetTree()
    oh, om = oracle.traverse(nodes, idx, v, f, rays)
    a.SetTunable("tail_quad", 16)
    h, m = a.TraverseBatch(rays)
    assert_hits_identical(oh, om, h, m)


def test_deep_stack_spills_and_ties(oracle):
    """A pile of 8192 large triangles that all straddle the z axis (a quarter of them exact duplicates of others), rays along that
    axis: every box of the tree is hit, so every step pushes three entries and the stack passes its 12 LDS entries into the spill
    arrays — established from the built tree itself: every box is hit by the rays (slab test below) and first_leaf_stack_bound
    exceeds 12.  Exact-t ties (the duplicates) are decided by record order."""
    v, f, dup, nt, rays = deep_stack_case()
    a = BVHAccel(np.float32)
    bo = default_build_options()
    bo["min_leaf_primitives"] = 1
    assert a.Build(f.shape[0], TriangleMesh(v, f), bo)
    nodes, idx = a.GetTree()
    # every ray passes through every node's box (x, y inside, the ray spans all of z) ...
    assert (nodes["bmin"][:, :2].max(axis=0) < -0.3).all() and (nodes["bmax"][:, :2].min(axis=0) > 0.3).all()
    assert nodes["bmin"][:, 2].min() > -5.0 and nodes["bmax"][:, 2].max() < 5.0
    # ... so at its first leaf it holds more entries than the LDS stack has
    bound = first_leaf_stack_bound(nodes)
    print("first-leaf stack bound:", bound)
    assert bound > 12
    h0, m0 = assert_sweep_identical(a, rays)
    assert m0.all()
    # A batch of at most 16 rays is out of rays at its first refill with at most 16 live lanes: at thresholds >= its size the wave
    # switches before its first step, so the QUADS make the walk to the first leaf and push and pop the entries beyond the 12th
    # through the spill arrays themselves (the bound above); 1500 rays alone could switch after the deep part of their walks.
    for k in (1, 4, 16):
        hk, mk = assert_sweep_identical(a, rays[:k])
        assert_hits_identical(h0[:k], m0[:k], hk, mk)
    oh, om = oracle.traverse(nodes, idx, v, f, rays[:200])
    assert_hits_identical(oh, om, h0[:200], m0[:200])
    # every ray's nearest triangle exists twice: an exact-t tie, settled by the order of the records (the oracle's, above)
    twice = set(int(p) for p in dup) | set(range(nt, f.shape[0]))
    assert all(int(p) in twice for p in h0["prim_id"])


def test_leaf_sizes(oracle, plane):
    v, f, a, rays1, bounce, _ = plane
    nodes, idx = a.GetTree()
    counts = set(int(c) for c in nodes["data"][nodes["flag"] != 0, 0])
    assert counts <= {1, 2, 3, 4} and len(counts) > 1, counts
    for rays in (rays1, bounce):
        h, m = assert_sweep_identical(a, rays)
        oh, om = oracle.traverse(nodes, idx, v, f, rays[::7])
        assert_hits_identical(oh, om, h[::7], m[::7])
    # leaves above four records: the owners' loop path (ORDER 0), five and more records in two trips of a quad
    b = BVHAccel(np.float32)
    bo = default_build_options()
    bo["min_leaf_primitives"] = 11
    assert b.Build(f.shape[0], TriangleMesh(v, f), bo)
    bn, bi = b.GetTree()
    assert int(bn["data"][bn["flag"] != 0, 0].max()) > 4
    for rays in (rays1[:3000], bounce[:3000]):
        h, m = assert_sweep_identical(b, rays)
        assert b.LastKernelName().endswith(", 4, 0>")
        oh, om = oracle.traverse(bn, bi, v, f, rays[::7])
        assert_hits_identical(oh, om, h[::7], m[::7])


def test_hostile_rays_and_duplicates(oracle):
    from test_gpu_wide4 import hostile_rays

    v, f = scenes.sphere(48, 24)
    f3 = np.concatenate([f, f[::-1], f]).astype(np.uint32)
    a = BVHAccel(np.float32)
    assert a.Build(f3.shape[0], TriangleMesh(v, f3))
    rays = np.concatenate([scenes.camera_rays(100, 60), hostile_rays(v, 6000, 7)])
    h, m = assert_sweep_identical(a, rays)
    nodes, idx = a.GetTree()
    oh, om = oracle.traverse(nodes, idx, v, f3, rays)
    assert_hits_identical(oh, om, h, m)


def test_rejecting_options(plane):
    v, f, a, rays1, bounce, _ = plane
    o = default_trace_options()
    o["prim_ids_range"] = (1000, 15000)
    o["skip_prim_id"] = 5000
    o["cull_back_face"] = 1
    for rays in (rays1, bounce):
        assert_sweep_identical(a, rays, o)
        assert "false, false, 4, 2>" in a.LastKernelName()


def test_occlusion_and_mixed_batches(plane):
    import torch

    v, f, a, rays1, bounce, shadow = plane
    res = sweep(a, lambda: a.OccludedBatch(shadow))
    for tq, occ in res[1:]:
        assert np.array_equal(res[0][1], occ)
    hit_size = 16

    def launch():
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()  # noqa: E731
        parts = [(shadow[:1237], True), (bounce[:999], False), (shadow[1237:1300], True), (rays1[:65], False), (bounce[999:1004], False)]
        batches, outs = [], []
        for r, occ in parts:
            d_h = None if occ else torch.zeros(r.shape[0] * hit_size, dtype=torch.uint8, device="cuda")
            d_m = torch.zeros(r.shape[0], dtype=torch.uint8, device="cuda")
            batches.append((dev(r), d_h, d_m, r.shape[0], "occlusion") if occ else (dev(r), d_h, d_m, r.shape[0]))
            outs.append((d_h, d_m))
        a.TraverseBatchesDevice(batches)
        torch.cuda.synchronize()
        return [(None if h is None else h.cpu().numpy().tobytes(), m.cpu().numpy().tobytes()) for h, m in outs]

    res = sweep(a, launch)
    for tq, got in res[1:]:
        assert got == res[0][1], tq


def test_back_to_back_launches(plane):
    import torch

    v, f, a, rays1, bounce, _ = plane
    want_h, want_m = a.TraverseBatch(bounce)
    d_rays = torch.from_numpy(bounce.view(np.uint8).copy()).cuda()
    rsz = bounce.dtype.itemsize
    sizes = [bounce.shape[0], 1, 63, 4097, 65, 1001, 7, 12345, 129, 3]
    for tq in THRESHOLDS:
        a.SetTunable("tail_quad", tq)
        outs = []
        for n in sizes:  # ten launches on one stream, nothing waited for in between
            d_h = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
            d_m = torch.zeros(n, dtype=torch.uint8, device="cuda")
            a.TraverseBatchDevice(d_rays[: n * rsz], d_h, d_m)
            outs.append((d_h, d_m))
        torch.cuda.synchronize()
        for n, (d_h, d_m) in zip(sizes, outs):
            h = d_h.cpu().numpy().view(want_h.dtype)
            assert_hits_identical(want_h[:n], want_m[:n], h, d_m.cpu().numpy())
    a.SetTunable("tail_quad", 0)


def test_kernel_name_is_unchanged(plane):
    v, f, a, rays1, _, _ = plane
    names = [k for _, k in sweep(a, lambda: (a.TraverseBatch(rays1[:500]), a.LastKernelName())[1])]
    assert len(set(names)) == 1 and names[0].endswith("<float, 12, false, 0, true, false, 4, 2>"), names

"""The four-lanes-to-a-ray tail (tunable tail_quad) now stands BEHIND the outer loop of the fp32 two-level triangle walk: the place in
the loop where it stood only notes that the wave switches and leaves the loop (traverse.hip).  What that changes and
tests/test_gpu_tail_quad.py does not visit: the default threshold, thresholds between the ones that file sweeps, the two ways into the
tail (at the top of the loop on the first trip; through the inner-node loop's extra exit with finished, unwritten results in the idle
lanes), waves that leave the loop WITHOUT the tail, and the result write behind the loop reading the batch table of a multi-batch
launch.  Every comparison is bit for bit on every field, against the same accelerator with the switch off (tail_quad = 0) and, where
the oracle covers the case, against the restated reference on the same node array."""
import numpy as np
import pytest

from helpers import assert_hits_identical
from nanort_amd import BVHAccel, TriangleMesh, scenes

pytestmark = pytest.mark.gpu

DEFAULT = 4  # ctx.h: tail_quad's default (profiles/r07a_tail_quad.txt; the sweep with the tail behind the loop is outstanding: r07b)


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


def test_default(oracle, plane):
    v, f, a, rays1, bounce, shadow, off, fresh = plane
    assert fresh == DEFAULT
    assert BVHAccel(np.float32).GetTunable("tail_quad") == DEFAULT
    assert a.GetTunable("tail_quad") == DEFAULT
    for name, rays in (("primary", rays1), ("bounce", bounce), ("shadow", shadow)):
        h, m = a.TraverseBatch(rays)
        assert_hits_identical(off[name][0], off[name][1], h, m)
        assert a.LastKernelName().endswith(", 4, 2>"), a.LastKernelName()
    assert np.array_equal(off["occluded"], a.OccludedBatch(shadow))  # any-hit
    assert np.array_equal(off["occluded"], off["shadow"][1])
    nodes, idx = a.GetTree()
    h, m = a.TraverseBatch(bounce)
    oh, om = oracle.traverse(nodes, idx, v, f, bounce[::7])
    assert_hits_identical(oh, om, h[::7], m[::7])


def test_two_ways_into_the_tail(oracle, plane):
    """A batch of at most N rays is out of rays after its first refill with at most N live lanes: it switches at the top of the outer
    loop on its first trip, before any step.  A batch of more than N rays (N + 1, 17, 65: one wave and two) walks the main loop
    first and switches through the inner-node loop's extra exit once enough rays have finished — their results still held,
    unwritten, in lanes that the tail is about to reuse."""
    v, f, a, rays1, bounce, shadow, off, fresh = plane
    nodes, idx = a.GetTree()
    oh, om = oracle.traverse(nodes, idx, v, f, bounce[:65])
    want_h, want_m = off["bounce"]
    assert_hits_identical(oh, om, want_h[:65], want_m[:65])
    sizes = sorted(set(k for n in (2, 3, 8, 12, 15) for k in (n - 1, n, n + 1, 17, 65)))
    a.SetTunable("tail_quad", 0)
    ref = {k: a.TraverseBatch(bounce[:k]) for k in sizes}
    for k in sizes:  # (a batch's records do not depend on what else the launch holds)
        assert_hits_identical(want_h[:k], want_m[:k], ref[k][0], ref[k][1])
    try:
        for n in (2, 3, 8, 12, 15):
            a.SetTunable("tail_quad", n)
            for k in (n - 1, n, n + 1, 17, 65):
                h, m = a.TraverseBatch(bounce[:k])
                assert_hits_identical(ref[k][0], ref[k][1], h, m)
                assert_hits_identical(oh[:k], om[:k], h, m)
    finally:
        a.SetTunable("tail_quad", fresh)


def test_waves_that_never_switch(plane):
    """Rays that point away from the mesh finish at their first step: the wave's live count goes from all to none, the loop is left
    through its own exit and the tail must not be entered (it would move rays that do not exist)."""
    v, f, a, rays1, bounce, shadow, off, fresh = plane
    away = rays1[:70].copy()
    away["dir"] = -away["dir"]
    try:
        for k in (5, 70):
            a.SetTunable("tail_quad", 0)
            h0, m0 = a.TraverseBatch(away[:k])
            assert not m0.any()
            assert np.array_equal(h0["t"], away["max_t"][:k]) and (h0["prim_id"] == 0xFFFFFFFF).all()
            for tq in (DEFAULT, 2, 8, 16):
                a.SetTunable("tail_quad", tq)
                h, m = a.TraverseBatch(away[:k])
                assert_hits_identical(h0, m0, h, m)
                assert not m.any() and np.array_equal(h["t"], away["max_t"][:k])
    finally:
        a.SetTunable("tail_quad", fresh)


def test_one_launch_over_two_batches(plane):
    """The result write behind the loop finds a ray's batch in the table in LDS; the second batch is an any-hit query."""
    import torch

    v, f, a, rays1, bounce, shadow, off, fresh = plane

    def launch():
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()  # noqa: E731
        d_h = torch.zeros(40 * 16, dtype=torch.uint8, device="cuda")
        d_m0 = torch.zeros(40, dtype=torch.uint8, device="cuda")
        d_m1 = torch.zeros(30, dtype=torch.uint8, device="cuda")
        a.TraverseBatchesDevice([(dev(bounce[100:140]), d_h, d_m0, 40), (dev(shadow[200:230]), None, d_m1, 30, "occlusion")])
        torch.cuda.synchronize()
        return d_h.cpu().numpy().view(off["bounce"][0].dtype), d_m0.cpu().numpy(), d_m1.cpu().numpy()

    try:
        a.SetTunable("tail_quad", 0)
        h0, m0, occ0 = launch()
        assert_hits_identical(off["bounce"][0][100:140], off["bounce"][1][100:140], h0, m0)
        assert np.array_equal(occ0, off["occluded"][200:230])
        for tq in (DEFAULT, 8, 16):
            a.SetTunable("tail_quad", tq)
            h, m, occ = launch()
            assert_hits_identical(h0, m0, h, m)
            assert np.array_equal(occ0, occ)
    finally:
        a.SetTunable("tail_quad", fresh)


def test_ten_launches_back_to_back(plane):
    """The completion record is published after the tail: the next launch on the context must not start on a half-finished one."""
    import torch

    v, f, a, rays1, bounce, shadow, off, fresh = plane
    want_h, want_m = off["bounce"]
    assert a.GetTunable("tail_quad") == DEFAULT
    d_rays = torch.from_numpy(bounce.view(np.uint8).copy()).cuda()
    rsz = bounce.dtype.itemsize
    sizes = [bounce.shape[0], 2, 17, 4099, 65, 15, 1003, 16, 130, 5]
    try:
        for tq in (DEFAULT, 16):
            a.SetTunable("tail_quad", tq)
            outs = []
            for n in sizes:  # one stream, nothing waited for in between
                d_h = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
                d_m = torch.zeros(n, dtype=torch.uint8, device="cuda")
                a.TraverseBatchDevice(d_rays[: n * rsz], d_h, d_m)
                outs.append((d_h, d_m))
            torch.cuda.synchronize()
            for n, (d_h, d_m) in zip(sizes, outs):
                assert_hits_identical(want_h[:n], want_m[:n], d_h.cpu().numpy().view(want_h.dtype), d_m.cpu().numpy())
    finally:
        a.SetTunable("tail_quad", fresh)

"""A launch's own streams in the walks (traverse.hip: the refill's ray loads, NRT_WRITE_RESULT's hit and flag stores, NRT_RAY_SKIP's id
load): every stream is addressed as global memory, whether its pointer is a kernel argument or comes out of the multi-batch table
in LDS, and a ray is loaded in 16-byte pieces.  That changes no bit of any record.  What can go wrong is addressing: a 36-byte ray
record is only 4-byte aligned and its pieces must stay inside it, and the pointers of a multi-batch launch are pre-offset by the
virtual index.  Every comparison is bit for bit on every field."""
import numpy as np
import pytest

from helpers import assert_hits_identical
from nanort_amd import BVHAccel, TriangleMesh, scenes
from nanort_amd.wire import hit_dtype

pytestmark = pytest.mark.gpu

HIT = hit_dtype(np.float32)
SIZES = (1, 63, 64, 65, 129)
OFFSETS = (0, 4, 8, 12)  # bytes past a 16-byte boundary


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


def at_offset(arr, off, tail=0):
    """The bytes of `arr` on the device, `off` bytes past a 16-byte boundary: a view into a larger uint8 tensor (kept alive by it)."""
    import torch

    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    big = torch.zeros(raw.shape[0] + 64 + tail, dtype=torch.uint8, device="cuda")
    pad = (-big.data_ptr()) % 16 + off
    view = big[pad : pad + raw.shape[0]]
    view.copy_(torch.from_numpy(raw.copy()))
    assert view.data_ptr() % 16 == off % 16
    return view


def exact(arr):
    """... in an allocation of exactly their size: the last record ends it."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def outputs(n, hit_off=0, mask_off=0):
    import torch

    d_h = at_offset(np.zeros(n, dtype=HIT), hit_off) if hit_off else torch.zeros(n * HIT.itemsize, dtype=torch.uint8, device="cuda")
    d_m = at_offset(np.zeros(n, dtype=np.uint8), mask_off) if mask_off else torch.zeros(n, dtype=torch.uint8, device="cuda")
    return d_h, d_m


def fetch(d_h, d_m):
    import torch

    torch.cuda.synchronize()
    return d_h.cpu().numpy().view(HIT).copy(), d_m.cpu().numpy().copy()


def launch(a, d_rays, n, hit_off=0, mask_off=0, **kw):
    d_h, d_m = outputs(n, hit_off, mask_off)
    assert a.TraverseBatchDevice(d_rays, d_h, d_m, **kw) == n
    return fetch(d_h, d_m)


def test_ray_base_alignment(oracle, plane):
    """Ray buffers 0, 4, 8 and 12 bytes past a 16-byte boundary, batches below, at and above a wave and a block: the same records
    as from an aligned copy, and the oracle's on the same node array."""
    v, f, a, rays1, bounce, _ = plane
    nodes, idx = a.GetTree()
    for rays in (rays1[3000:], bounce):
        oh, om = oracle.traverse(nodes, idx, v, f, rays[:65])
        for n in SIZES:
            want_h, want_m = launch(a, exact(rays[:n]), n)
            assert_hits_identical(oh[: min(n, 65)], om[: min(n, 65)], want_h[:65], want_m[:65])
            for off in OFFSETS:
                h, m = launch(a, at_offset(rays[:n], off), n)
                assert_hits_identical(want_h, want_m, h, m)
    assert a.LastKernelName().endswith(", 4, 2>")  # the production instantiation


def test_last_record_ends_the_allocation(plane):
    """Rays in exactly n * 36 bytes, records in exactly n * 16, flags in n: the pieces of the last ray's load cover its 36 bytes and
    no more, and so do the stores.  (What a load past the end would do depends on the allocator; what is asserted here is the
    records — of the last ray too — and the caching allocator's neighbours staying intact: a canary behind every buffer.)"""
    import torch

    v, f, a, rays1, bounce, _ = plane
    for rays in (rays1, bounce):
        want_h, want_m = a.TraverseBatch(rays)
        for n in SIZES + (rays.shape[0],):
            d_r = exact(rays[:n])
            assert d_r.numel() == n * 36
            d_h = torch.full((n * 16,), 0xA5, dtype=torch.uint8, device="cuda")
            d_m = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
            canary = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")  # (a neighbour of the small buffers in the allocator's block)
            a.TraverseBatchDevice(d_r, d_h, d_m)
            h, m = fetch(d_h, d_m)
            assert_hits_identical(want_h[:n], want_m[:n], h, m)
            assert bool((canary == 0x5A).all())
            assert d_r.cpu().numpy().tobytes() == rays[:n].tobytes()


def test_two_batches_in_one_launch(plane):
    """One launch over a closest-hit batch and an occlusion batch, every buffer at another offset: the pointers come out of the
    table in LDS, pre-offset by the virtual index.  The records are those of the two single-batch launches."""
    import torch

    v, f, a, rays1, bounce, shadow = plane
    for n1, n2 in ((129, 65), (1, 63), (4000, 3001)):
        r1, r2 = bounce[:n1], shadow[:n2]
        want_h, want_m = launch(a, exact(r1), n1)
        d_occ = torch.zeros(n2, dtype=torch.uint8, device="cuda")
        a.OccludedBatchDevice(exact(r2), d_occ)
        torch.cuda.synchronize()
        want_occ = d_occ.cpu().numpy()
        d_h1, d_m1 = outputs(n1, hit_off=48, mask_off=3)
        d_m2 = at_offset(np.zeros(n2, dtype=np.uint8), 7)
        a.TraverseBatchesDevice([(at_offset(r1, 4), d_h1, d_m1, n1), (at_offset(r2, 12), None, d_m2, n2, "occlusion")])
        h, m = fetch(d_h1, d_m1)
        assert_hits_identical(want_h, want_m, h, m)
        assert np.array_equal(want_occ, d_m2.cpu().numpy())
    assert a.LastKernelName().endswith(", 4, 2>")


def test_per_ray_skip_ids(plane):
    """Per-ray skip ids (each ray skips the triangle it starts on — and so does the aligned call), rays and ids at offset bases; the
    same in a two-batch launch, whose second batch takes the launch's skip id."""
    v, f, a, rays1, bounce, shadow = plane
    h1, m1 = a.TraverseBatch(rays1)
    n = min(4001, bounce.shape[0])
    assert n > 129
    src = np.ascontiguousarray(h1["prim_id"][m1 != 0][:n], dtype=np.uint32)  # the triangles the bounce rays leave (one ray per hit, in order)
    r = bounce[:n]
    want_h, want_m = launch(a, exact(r), n, skip_prim_ids=exact(src))
    for off in OFFSETS:
        h, m = launch(a, at_offset(r, off), n, hit_off=16, mask_off=5, skip_prim_ids=at_offset(src, (off + 4) % 16))
        assert_hits_identical(want_h, want_m, h, m)
    assert "false, false, 4, 2>" in a.LastKernelName()  # (ids can reject: never the PLAIN instantiation)
    assert not (want_h["prim_id"][want_m != 0] == src[want_m != 0]).any()
    # two batches, ids on the first only
    n2 = 777
    want2_h, want2_m = launch(a, exact(shadow[:n2]), n2)
    d_h1, d_m1 = outputs(n, hit_off=32, mask_off=1)
    d_h2, d_m2 = outputs(n2, hit_off=16, mask_off=9)
    a.TraverseBatchesDevice([(at_offset(r, 8), d_h1, d_m1, n), (at_offset(shadow[:n2], 4), d_h2, d_m2, n2)], skip_prim_ids=[at_offset(src, 12), None])
    assert_hits_identical(want_h, want_m, *fetch(d_h1, d_m1))
    assert_hits_identical(want2_h, want2_m, *fetch(d_h2, d_m2))


def test_tail_thresholds(plane):
    """The tail behind the loop writes its results through the same macros: primaries and bounce rays at tail_quad 0, 4 and 16, ray
    buffers at an offset base, against the aligned launch at the default."""
    v, f, a, rays1, bounce, _ = plane
    default = a.GetTunable("tail_quad")
    try:
        for rays in (rays1, bounce):
            want_h, want_m = launch(a, exact(rays), rays.shape[0])
            for tq in (0, 4, 16):
                a.SetTunable("tail_quad", tq)
                for n in (65, rays.shape[0]):
                    h, m = launch(a, at_offset(rays[:n], 12), n, hit_off=16, mask_off=1)
                    assert_hits_identical(want_h[:n], want_m[:n], h, m)
            a.SetTunable("tail_quad", default)
    finally:
        a.SetTunable("tail_quad", default)
    assert a.LastKernelName().endswith(", 4, 2>")

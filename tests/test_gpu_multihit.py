"""Multi-hit traversal on the GPU (nanort_amd/csrc/own_walks.hip, include/nanort_hip.h nrtMultiHitTraverseBatch*): every byte of
the hit rows and counts equals the CPU model of the contract (tests/multihit_model.c) on the same node array; K = 1 is closest hit
up to exact-t ties; layers, shared edges, the device entry on several streams, the header's batch method, error paths, and
rebuilds that wait for multi-hit launches in flight."""
import numpy as np
import pytest

from helpers import trace_options
from multihit_fixture import check_k1_against_closest, header_check, hits_bytes, hostile_rays, model, random_window_rays, soup, tie_checker
from nanort_amd import BVHAccel, TriangleMesh, scenes
from nanort_amd.capi import NrtError
from nanort_amd.wire import hit_dtype, ray_dtype, widen_rays

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 8, 16, 64)


def gpu_on_tree(real, v, f, nodes, idx, stride=None):
    a = BVHAccel(real)
    a.SetMesh(TriangleMesh(v, f, stride))
    a.SetTree(nodes, idx)
    return a


def assert_model(a, nodes, idx, v, f, rays, K, opts=None, stride=None):
    h, c = a.MultiHitTraverseBatch(rays, K, opts)
    mh, mc = model(nodes, idx, v, f, rays, K, opts, stride)
    assert np.array_equal(c, mc), "counts differ from the model (K=%d)" % K
    assert hits_bytes(h) == hits_bytes(mh), "hit rows differ from the model (K=%d)" % K
    return h, c


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["f32", "f64"])
def c1_built(request, c1_mesh):
    """C1 built on the GPU, its camera rays and their bounce rays."""
    real = request.param
    v, f = c1_mesh
    v = v.astype(real)
    a = BVHAccel(real)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    nodes, idx = a.GetTree()
    cam = scenes.camera_rays(192, 108)
    a32 = BVHAccel(np.float32)
    a32.Build(f.shape[0], TriangleMesh(v.astype(np.float32), f))
    h32, m32 = a32.TraverseBatch(cam)
    bounce = scenes.secondary_rays("bounce", v.astype(np.float32), f, cam, h32, m32)
    a32.close()
    if real == np.float64:
        cam, bounce = widen_rays(cam), widen_rays(bounce)
    return real, v, f, nodes, idx, a, cam, bounce


@pytest.mark.parametrize("K", KS)
def test_c1_camera_bounce_and_random_windows_equal_the_model(c1_built, K):
    real, v, f, nodes, idx, a, cam, bounce = c1_built
    for rays in (cam, bounce, random_window_rays(cam, 5)):
        assert_model(a, nodes, idx, v, f, rays, K)


@pytest.mark.parametrize("K", (1, 3, 8, 64))
def test_every_trace_option(c1_built, K):
    real, v, f, nodes, idx, a, cam, bounce = c1_built
    n = f.shape[0]
    for o in (trace_options(range_=(n // 4, 3 * n // 4)), trace_options(skip=int(n // 2)), trace_options(cull=True),
              trace_options(range_=(10, n - 10), skip=int(n // 3), cull=True)):
        assert_model(a, nodes, idx, v, f, cam, K, o)
        assert_model(a, nodes, idx, v, f, bounce, K, o)


@pytest.mark.parametrize("real", [np.float32, np.float64])
def test_random_soup_and_hostile_rays(oracle, real):
    v, f, stride = soup(real)
    nodes, idx, _ = oracle.build(v, f, stride=stride)
    a = gpu_on_tree(real, v, f, nodes, idx, stride)
    rays = hostile_rays(real, 6000)
    for K in KS:
        assert_model(a, nodes, idx, v, f, rays, K, None, stride)
    assert_model(a, nodes, idx, v, f, rays, 4, trace_options(cull=True), stride)


def test_deep_reference_tree_spills_past_the_lds_stack(oracle):
    v, f = scenes.plane(300, 150)
    nodes, idx, st = oracle.build(v, f)
    assert st["max_tree_depth"] > 40
    a = gpu_on_tree(np.float32, v, f, nodes, idx)
    rays = scenes.camera_rays(320, 180)
    for K in (1, 4, 64):
        assert_model(a, nodes, idx, v, f, rays, K)


def test_c3_sample_k4():
    v, f = scenes.plane(1000, 500)
    a = BVHAccel(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    nodes, idx = a.GetTree()
    rays = np.ascontiguousarray(scenes.camera_rays(1920, 1080)[::32])
    h, c = assert_model(a, nodes, idx, v, f, rays, 4)
    assert c.sum() > 0


def test_k1_against_closest_hit(oracle, c1_built):
    real, v, f, nodes, idx, a, cam, bounce = c1_built
    for rays in (cam, bounce):
        h, c = a.MultiHitTraverseBatch(rays, 1)
        ch, cm = a.TraverseBatch(rays)
        check_k1_against_closest(h, c, ch, cm, tie_checker(v, f, rays))
    sv, sf, stride = soup(real)
    snodes, sidx, _ = oracle.build(sv, sf, stride=stride)
    s = gpu_on_tree(real, sv, sf, snodes, sidx, stride)
    rays = hostile_rays(real, 6000)
    h, c = s.MultiHitTraverseBatch(rays, 1)
    ch, cm = s.TraverseBatch(rays)
    check_k1_against_closest(h, c, ch, cm, tie_checker(sv, sf, rays, None, stride))


def layered_quads(N):
    """N parallel unit quads at z = 1 .. N (two triangles each: prims 2k, 2k + 1 form layer k)."""
    v, f = [], []
    for k in range(N):
        z = float(k + 1)
        b = len(v)
        v += [(-1, -1, z), (1, -1, z), (1, 1, z), (-1, 1, z)]
        f += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.uint32)


@pytest.mark.parametrize("N", [1, 5, 40, 100])
def test_layers_front_to_back(N):
    v, f = layered_quads(N)
    a = BVHAccel(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    rng = np.random.default_rng(N)
    n = 512
    rays = np.zeros((n,), dtype=ray_dtype(np.float32))
    rays["org"][:, :2] = rng.uniform(-0.9, 0.9, size=(n, 2))
    rays["org"][:, 2] = 0.0
    rays["dir"] = (0, 0, 1)
    rays["max_t"] = 1e30
    for K in (1, 3, 16, 64):
        h, c = a.MultiHitTraverseBatch(rays, K)
        assert (c == min(K, N)).all()
        layer = h["prim_id"][:, : min(K, N)] // 2
        assert (layer == np.arange(min(K, N))[None, :]).all()
        assert (np.diff(h["t"][:, : min(K, N)], axis=1) > 0).all()


def test_shared_edge_returns_both_triangles():
    v = np.array([(-1, -1, 2), (1, -1, 2), (1, 1, 2), (-1, 1, 2)], dtype=np.float32)
    f = np.array([(0, 1, 2), (0, 2, 3)], dtype=np.uint32)
    a = BVHAccel(np.float32)
    assert a.Build(2, TriangleMesh(v, f))
    s = np.linspace(-0.75, 0.75, 7, dtype=np.float32)
    rays = np.zeros((s.size,), dtype=ray_dtype(np.float32))
    rays["org"][:, 0] = s
    rays["org"][:, 1] = s  # on the diagonal x == y, the edge both triangles share
    rays["dir"] = (0, 0, 1)
    rays["max_t"] = 1e30
    for K in (2, 3, 8):
        h, c = a.MultiHitTraverseBatch(rays, K)
        assert (c == 2).all()
        assert (h["prim_id"][:, 0] == 0).all() and (h["prim_id"][:, 1] == 1).all()
        assert (h["t"][:, 0] == h["t"][:, 1]).all()
    h, c = a.MultiHitTraverseBatch(rays, 1)
    assert (c == 1).all() and (h["prim_id"][:, 0] == 0).all()


def test_device_entry_on_two_streams_equals_host_entry(c1_built):
    import torch

    real, v, f, nodes, idx, a, cam, bounce = c1_built
    hsz = hit_dtype(real).itemsize
    jobs = [(cam, 8), (bounce, 3)]
    want = [a.MultiHitTraverseBatch(r, K) for r, K in jobs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for (r, K), s in zip(jobs, streams):
        d_rays = torch.from_numpy(r.view(np.uint8).copy()).cuda()
        d_hits = torch.full((r.shape[0] * K * hsz,), 0xAB, dtype=torch.uint8, device="cuda")
        d_counts = torch.full((r.shape[0],), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        a.MultiHitTraverseBatchDevice(d_rays, K, d_hits, d_counts, stream=s.cuda_stream)
        outs.append((d_rays, d_hits, d_counts))
    torch.cuda.synchronize()
    for (r, K), (h, c), (_, d_hits, d_counts) in zip(jobs, want, outs):
        gh = d_hits.cpu().numpy().view(hit_dtype(real)).reshape(r.shape[0], K)
        assert hits_bytes(gh) == hits_bytes(h)
        assert np.array_equal(d_counts.cpu().numpy().view(np.uint32), c)
    # counts may be NULL
    r, K = jobs[0]
    d_rays = torch.from_numpy(r.view(np.uint8).copy()).cuda()
    d_hits = torch.zeros((r.shape[0] * K * hsz,), dtype=torch.uint8, device="cuda")
    a.MultiHitTraverseBatchDevice(d_rays, K, d_hits)
    torch.cuda.synchronize()
    assert hits_bytes(d_hits.cpu().numpy().view(hit_dtype(real)).reshape(r.shape[0], K)) == hits_bytes(want[0][0])


def status_of(fn):
    try:
        fn()
    except NrtError as e:
        return int(str(e).split("status ")[1].split(":")[0])
    return 0


def test_error_paths_leave_the_context_usable(c1_mesh):
    from nanort_amd import capi

    v, f = c1_mesh
    rays = scenes.camera_rays(64, 32)
    a = BVHAccel(np.float32)
    INVALID, PRECISION = capi.NRT_ERR_INVALID, capi.NRT_ERR_PRECISION
    assert status_of(lambda: a.MultiHitTraverseBatch(rays, 4)) == INVALID  # no tree
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    want = a.MultiHitTraverseBatch(rays, 4)
    assert status_of(lambda: a.MultiHitTraverseBatch(rays, 0)) == INVALID
    assert status_of(lambda: a.MultiHitTraverseBatch(rays, 65)) == INVALID
    L, h = a._L, a._h
    hits = np.zeros((rays.shape[0] * 4,), dtype=hit_dtype(np.float32))
    assert L.nrtMultiHitTraverseBatch_f32(h, None, rays.shape[0], 4, None, hits.ctypes.data, None) == INVALID
    assert L.nrtMultiHitTraverseBatch_f32(h, rays.ctypes.data, rays.shape[0], 4, None, None, None) == INVALID
    assert L.nrtMultiHitTraverseBatch_f32(h, rays.ctypes.data, 0, 4, None, None, None) == 0  # n == 0
    assert L.nrtMultiHitTraverseBatchDevice_f32(h, rays.ctypes.data, 1 << 31, 4, None, hits.ctypes.data, None, None) == INVALID
    r64 = widen_rays(rays)
    hits64 = np.zeros((rays.shape[0] * 4,), dtype=hit_dtype(np.float64))
    assert L.nrtMultiHitTraverseBatch_f64(h, r64.ctypes.data, r64.shape[0], 4, None, hits64.ctypes.data, None) == PRECISION
    got = a.MultiHitTraverseBatch(rays, 4)
    assert hits_bytes(got[0]) == hits_bytes(want[0]) and np.array_equal(got[1], want[1])
    # sphere and cylinder contexts
    from nanort_amd.accel import CylinderGeometry, SphereGeometry

    s = BVHAccel(np.float32)
    c, r = scenes.random_spheres(200)
    assert s.Build(200, SphereGeometry(c, r))
    assert status_of(lambda: s.MultiHitTraverseBatch(scenes.particle_camera_rays(32, 32), 4)) == INVALID
    s.TraverseBatch(scenes.particle_camera_rays(32, 32))  # still usable
    cy = BVHAccel(np.float32)
    e, cr = scenes.random_cylinders(100)
    assert cy.Build(100, CylinderGeometry(e, cr))
    assert status_of(lambda: cy.MultiHitTraverseBatch(rays, 4)) == INVALID
    cy.TraverseBatch(rays)


def test_rebuild_waits_for_a_device_multihit_launch(c1_mesh):
    """A rebuild issued right behind an asynchronous multi-hit launch must wait for it: its rows are those of the OLD tree."""
    import torch

    v, f = c1_mesh
    a = BVHAccel(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    rays = scenes.camera_rays(960, 540)
    K = 16
    want = a.MultiHitTraverseBatch(rays, K)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.zeros((rays.shape[0] * K * 16,), dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros((rays.shape[0],), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    a.MultiHitTraverseBatchDevice(d_rays, K, d_hits, d_counts, stream=s.cuda_stream)
    moved = v + np.float32(50.0)  # the new mesh lies elsewhere: no camera ray reaches it
    assert a.Build(f.shape[0], TriangleMesh(moved, f))
    torch.cuda.synchronize()
    gh = d_hits.cpu().numpy().view(hit_dtype(np.float32)).reshape(rays.shape[0], K)
    assert hits_bytes(gh) == hits_bytes(want[0])
    assert np.array_equal(d_counts.cpu().numpy().view(np.uint32), want[1])
    assert a.MultiHitTraverseBatch(rays, K)[1].sum() != want[1].sum()


def test_header_backend_batch_equals_its_per_ray_multihit_traverse(tmp_path, c1_mesh):
    """-DNANORT_USE_HIP_BACKEND: Build() runs on the GPU, MultiHitTraverseBatch equals the program's own per-ray MultiHitTraverse
    (the host walk over the read-back tree), which equals the model on that tree."""
    v, f = c1_mesh
    rays = np.concatenate([scenes.camera_rays(96, 54), random_window_rays(scenes.camera_rays(64, 36), 9)])
    for K in (1, 4, 16):
        counts, rows, nodes, idx, bcounts, brows = header_check(str(tmp_path), v, f, rays, K, backend=True)
        assert np.array_equal(bcounts, counts)
        assert hits_bytes(brows) == hits_bytes(rows)
        mh, mc = model(nodes, idx, v, f, rays, K)
        assert np.array_equal(counts, mc) and hits_bytes(rows) == hits_bytes(mh)

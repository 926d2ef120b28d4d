"""Per-ray skip ids (include/nanort_hip.h, "per-ray skip ids"; nrt*BatchSkip*): ray i of a batch is traced with
BVHTraceOptions::skip_prim_id = skip_prim_ids[i].

The mesh: two nested closed shells of the lumpy-sphere generator (2 x 1024 triangles, the outer one the inner one scaled by 1.25
about its centre), the eye inside the inner shell, 4 099 pseudo-random directions — every ray hits, neighbouring rays hit
different triangles, and a ray that skips its first hit finds the outer shell behind it.  The tree is GPU-built
(min_leaf_primitives 4).  Wave 1 is a plain TraverseBatch; wave 2 traces the same rays with skip_prim_ids = wave 1's prim_id
column (depth peeling).  The oracle is oracle.bindings traverse on the GPU tree's own node and index arrays, called once per
distinct id with that id in the options; records are compared with assert_hits_identical (every field, no tolerance), under
every walk a launch with an array can take and at ray counts 1, 65 (the whole launch in the refill and tail code) and 4 099
(not a multiple of a chunk)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import assert_hits_identical, assert_hits_match
from nanort_amd import BVHAccel, CurveGeometry, CylinderGeometry, SphereGeometry, TriangleMesh, capi, scenes
from nanort_amd.wire import default_build_options, default_trace_options, hit_dtype, ray_dtype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 65, 4099)
SENTINEL = 0xFFFFFFFF
EYE = (3.0, 6.0, 1.0)


def shells():
    v1, f1 = scenes.sphere(32, 17)
    c = np.array([0.0, 5.0, 0.0], dtype=np.float32)
    v = np.concatenate([v1, (c + np.float32(1.25) * (v1 - c)).astype(np.float32)])
    f = np.concatenate([f1, f1 + v1.shape[0]]).astype(np.uint32)
    return np.ascontiguousarray(v), np.ascontiguousarray(f)


def eye_rays(n, real):
    rng = np.random.default_rng(5)
    d = rng.normal(size=(4099, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros(4099, dtype=ray_dtype(real))
    r["org"] = EYE
    r["dir"] = d.astype(np.float32)  # (the same directions in both precisions)
    r["min_t"], r["max_t"] = 0.0, 1.0e30
    return r[:n].copy()


def oracle_per_ray_skip(orc, w, rays, ids):
    """Ray i traced alone with skip_prim_id = ids[i]: one oracle call per distinct id."""
    hits = np.zeros(rays.shape[0], dtype=hit_dtype(w.real))
    mask = np.zeros(rays.shape[0], dtype=np.uint8)
    for p in np.unique(ids):
        sel = np.nonzero(ids == p)[0]
        o = default_trace_options()
        o["skip_prim_id"] = p
        h, m = orc.traverse(w.nodes, w.idx, w.v, w.f, rays[sel], o)
        hits[sel], mask[sel] = h, m
    return hits, mask


class World:
    """One precision: the mesh, the GPU-built tree, and per ray count the rays, wave 1 and the oracle's wave 2 (computed once)."""

    def __init__(self, real, orc, **build_tunables):
        self.real = real
        v, f = shells()
        self.v, self.f = v.astype(real), f
        self.a = BVHAccel(real)
        for k, val in build_tunables.items():  # (tunables that shape the private tree layout: before Build)
            self.a.SetTunable(k, val)
        bo = default_build_options(real)
        bo["min_leaf_primitives"] = 4
        assert self.a.Build(f.shape[0], TriangleMesh(self.v, f), bo)
        self.nodes, self.idx = self.a.GetTree()
        self.defaults = {k: self.a.GetTunable(k) for k in ("wide", "wide_stack", "leaf_compact", "order4", "wide4_big", "tail_quad")}
        self.orc = orc
        self.waves = {}

    def wave(self, n):
        if n not in self.waves:
            rays = eye_rays(n, self.real)
            self.reset()
            h1, m1 = self.a.TraverseBatch(rays)
            oh, om = self.orc.traverse(self.nodes, self.idx, self.v, self.f, rays)
            assert_hits_identical(oh, om, h1, m1)
            ids = np.where(m1 == 1, h1["prim_id"], SENTINEL).astype(np.uint32)
            # not vacuous: nearly every ray carries an id, and neighbours carry different ones (a lane that used its neighbour's or
            # its predecessor's id would be seen)
            assert (ids != SENTINEL).mean() >= 0.9
            if n > 1:
                assert (ids[1:] != ids[:-1]).mean() >= 0.5
            want = oracle_per_ray_skip(self.orc, self, rays, ids)
            assert want[1].mean() >= 0.9  # (the outer shell is behind the skipped triangle)
            self.waves[n] = (rays, h1, m1, ids, want)
        return self.waves[n]

    def reset(self):
        for k, val in self.defaults.items():
            self.a.SetTunable(k, val)

    def configure(self, **tunables):
        self.reset()
        for k, val in tunables.items():
            self.a.SetTunable(k, val)
        return self.a


@pytest.fixture(scope="module")
def w32(oracle):
    return World(np.float32, oracle)


@pytest.fixture(scope="module")
def w64(oracle):
    return World(np.float64, oracle)


@pytest.fixture(scope="module")
def w32_one_level(oracle):
    """A tree built without the two-level records: one level per step at the default depth of 10 LDS entries."""
    return World(np.float32, oracle, wide4=0)


def check_peeled(w, n, kernel_tail, tie_aware=False, **tunables):
    rays, h1, m1, ids, (oh, om) = w.wave(n)
    a = w.configure(**tunables)
    h2, m2 = a.TraverseBatch(rays, skip_prim_ids=ids)
    k = a.LastKernelName()
    assert k.endswith(kernel_tail), k
    if tie_aware:  # order4 = 1: prim_id / u / v are free at exact-t ties
        for p in np.unique(ids):  # (every differing ray re-verified under its own options)
            sel = np.nonzero(ids == p)[0]
            o = default_trace_options()
            o["skip_prim_id"] = p
            assert_hits_match(oh[sel], om[sel], h2[sel], m2[sel], w.orc, w.nodes, w.idx, w.v, w.f, rays[sel], base_opts=o)
    else:
        assert_hits_identical(oh, om, h2, m2)
    hit1 = m1 == 1
    assert ((m2[hit1] == 0) | (h2["prim_id"][hit1] != h1["prim_id"][hit1])).all()  # the skipped triangle is never reported
    w.reset()


# (kernel-name tails: "<T, STACK, STATS, KIND, PLAIN, CLOCK, WIDTH, ORDER>" — PLAIN false everywhere: a launch with ids keeps the id tests)
F32_WALKS = [
    ("literal", "k_traverse<float>", dict(wide=0)),
    ("one_level_8", "<float, 8, false, 0, false, false, 2, 0>", dict(wide_stack=8)),
    ("one_level_12", "<float, 12, false, 0, false, false, 2, 0>", dict(wide_stack=12)),
    ("one_level_16", "<float, 16, false, 0, false, false, 2, 0>", dict(wide_stack=16)),
    ("two_level_items_tail", "false, false, 4, 2>", dict(leaf_compact=1, tail_quad=16)),
    ("two_level_items_notail", "false, false, 4, 2>", dict(leaf_compact=1, tail_quad=0)),
    ("two_level_tail", "false, false, 4, 0>", dict(leaf_compact=0, tail_quad=16)),
    ("two_level_notail", "false, false, 4, 0>", dict(leaf_compact=0, tail_quad=0)),
    ("offsets64_items", "false, false, 4, 6>", dict(wide4_big=2, leaf_compact=1)),
    ("offsets64", "false, false, 4, 4>", dict(wide4_big=2, leaf_compact=0)),
]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name,tail,tunables", F32_WALKS, ids=[x[0] for x in F32_WALKS])
def test_depth_peeling_equals_the_per_ray_oracle_f32(w32, name, tail, tunables, n):
    check_peeled(w32, n, tail, **tunables)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("leaf_compact,tail", [(1, "false, false, 4, 3>"), (0, "false, false, 4, 1>")])
def test_depth_peeling_distance_order_f32(w32, leaf_compact, tail, n):
    check_peeled(w32, n, tail, tie_aware=True, order4=1, leaf_compact=leaf_compact)


@pytest.mark.parametrize("n", COUNTS)
def test_depth_peeling_one_level_default_depth_f32(w32_one_level, n):
    check_peeled(w32_one_level, n, "<float, 10, false, 0, false, false, 2, 0>")


F64_WALKS = [
    ("literal", "k_traverse<double>", dict(wide=0)),
    ("one_level_8", "<double, 8, false, 0, false, false, 2, 0>", dict(wide_stack=8)),
    ("one_level_10", "<double, 10, false, 0, false, false, 2, 0>", dict()),
    ("one_level_12", "<double, 12, false, 0, false, false, 2, 0>", dict(wide_stack=12)),
    ("one_level_16", "<double, 16, false, 0, false, false, 2, 0>", dict(wide_stack=16)),
]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name,tail,tunables", F64_WALKS, ids=[x[0] for x in F64_WALKS])
def test_depth_peeling_equals_the_per_ray_oracle_f64(w64, name, tail, tunables, n):
    check_peeled(w64, n, tail, **tunables)


def mixed_ids(w, n=4099):
    """Wave 1's ids with the sentinel on every third ray, an id at or above num_faces on every fifth and, on every seventh, a
    triangle the ray does not hit (checked with the oracle restricted to that triangle)."""
    if "mixed" in w.waves:
        return w.waves["mixed"]
    rays, h1, m1, ids, _ = w.wave(n)
    nf = w.f.shape[0]
    ids = ids.copy()
    i = np.arange(n)
    ids[i % 3 == 2] = SENTINEL
    ids[i % 5 == 4] = (nf + i[i % 5 == 4]).astype(np.uint32)
    for k in i[i % 7 == 6]:
        c = (int(h1["prim_id"][k]) + nf // 2) % nf
        while True:
            o = default_trace_options()
            o["prim_ids_range"] = (c, c + 1)
            if w.orc.traverse(w.nodes, w.idx, w.v, w.f, rays[k:k + 1], o)[1][0] == 0:
                break
            c = (c + 1) % nf
        ids[k] = c
    w.waves["mixed"] = (rays, h1, m1, ids, (i % 3 == 2) | (i % 5 == 4) | (i % 7 == 6))
    return w.waves["mixed"]


@pytest.mark.parametrize("walk", ["two_level_items", "two_level", "one_level", "literal"])
def test_mixed_ids_f32(w32, walk):
    rays, h1, m1, ids, no_effect = mixed_ids(w32)
    a = w32.configure(**{"two_level_items": dict(), "two_level": dict(leaf_compact=0), "one_level": dict(wide_stack=12), "literal": dict(wide=0)}[walk])
    h, m = a.TraverseBatch(rays, skip_prim_ids=ids)
    oh, om = oracle_per_ray_skip(w32.orc, w32, rays, ids)
    assert_hits_identical(oh, om, h, m)
    # the sentinel, an id beyond the mesh and a triangle the ray does not hit skip nothing: the no-skip launch's record
    assert_hits_identical(h1[no_effect], m1[no_effect], h[no_effect], m[no_effect])
    assert (h["prim_id"][~no_effect] != h1["prim_id"][~no_effect]).all()
    w32.reset()


def test_mixed_ids_f64(w64):
    rays, h1, m1, ids, no_effect = mixed_ids(w64)
    w64.reset()
    h, m = w64.a.TraverseBatch(rays, skip_prim_ids=ids)
    oh, om = oracle_per_ray_skip(w64.orc, w64, rays, ids)
    assert_hits_identical(oh, om, h, m)
    assert_hits_identical(h1[no_effect], m1[no_effect], h[no_effect], m[no_effect])


def _vp(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_null_array_is_the_existing_call(w32, w64, prec):
    w = w32 if prec == "f32" else w64
    rays, h1, m1, _, _ = w.wave(4099)
    w.reset()
    a, L = w.a, capi.lib()
    opt = default_trace_options()
    opt["skip_prim_id"] = int(h1["prim_id"][0])  # (read, as by the existing call, when there is no array)
    for o in (None, opt):
        h0, m0 = a.TraverseBatch(rays, o)
        k0 = a.LastKernelName()
        h = np.full(rays.shape[0], 0, dtype=hit_dtype(w.real))
        m = np.full(rays.shape[0], 9, dtype=np.uint8)
        assert getattr(L, "nrtTraverseBatchSkip_" + prec)(a._h, _vp(rays), rays.shape[0], _vp(o), None, _vp(h), _vp(m)) == 0
        assert a.LastKernelName() == k0
        assert h.tobytes() == h0.tobytes() and m.tobytes() == m0.tobytes()
        assert (", true, false, " in k0) == (o is None), k0  # PLAIN exactly for the default options
        occ0 = a.OccludedBatch(rays, o)
        occ = np.full(rays.shape[0], 9, dtype=np.uint8)
        assert getattr(L, "nrtOccludedBatchSkip_" + prec)(a._h, _vp(rays), rays.shape[0], _vp(o), None, _vp(occ)) == 0
        assert occ.tobytes() == occ0.tobytes()
    assert not (h0["prim_id"] == int(h1["prim_id"][0])).any()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_occlusion_equals_the_closest_hit_flags(w32, w64, prec):
    import torch

    w = w32 if prec == "f32" else w64
    rays, h1, m1, ids, _ = mixed_ids(w)
    # (half of the rays end before the outer shell: flags of both kinds)
    rays = rays.copy()
    rays["max_t"][::2] = h1["t"][::2] * 1.1
    w.reset()
    a = w.a
    h, m = a.TraverseBatch(rays, skip_prim_ids=ids)
    assert 0.1 < m.mean() < 0.95
    assert np.array_equal(a.OccludedBatch(rays, skip_prim_ids=ids), m)
    d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    d_ids = torch.from_numpy(ids.view(np.uint8)).cuda()
    d_mask = torch.full((rays.shape[0],), 9, dtype=torch.uint8, device="cuda")
    d_hits = torch.zeros(rays.shape[0] * hit_dtype(w.real).itemsize, dtype=torch.uint8, device="cuda")
    d_mask2 = torch.full((rays.shape[0],), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    a.OccludedBatchDevice(d_rays, d_mask, stream=s, skip_prim_ids=d_ids)
    a.TraverseBatchDevice(d_rays, d_hits, d_mask2, stream=s, skip_prim_ids=d_ids)
    s.synchronize()
    assert np.array_equal(d_mask.cpu().numpy(), m)
    assert np.array_equal(d_mask2.cpu().numpy(), m)
    assert d_hits.cpu().numpy().view(hit_dtype(w.real)).tobytes() == h.tobytes()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_batches_equal_separate_calls(w32, w64, prec):
    """Three batches — closest-hit with ids, occlusion with ids, closest-hit with a NULL entry (the call's skip_prim_id) — through
    the device form and the host form: each equals the separate calls.  fp32: one launch; fp64: one after the other."""
    import torch

    w = w32 if prec == "f32" else w64
    rays, h1, m1, ids, _ = mixed_ids(w)
    w.reset()
    a = w.a
    HIT = hit_dtype(w.real)
    opt = default_trace_options()
    opt["skip_prim_id"] = int(h1["prim_id"][7])
    b0, b1, b2 = rays[:2000], rays[1000:4099], rays[:777]
    i0, i1 = ids[:2000], ids[1000:4099]
    want0 = a.TraverseBatch(b0, opt, skip_prim_ids=i0)
    want1 = a.OccludedBatch(b1, opt, skip_prim_ids=i1)
    want2 = a.TraverseBatch(b2, opt)
    assert want2[0]["prim_id"][7] != h1["prim_id"][7] and not np.array_equal(want0[0]["prim_id"][:777], want2[0]["prim_id"])
    got = a.TraverseBatches([b0, (b1, "occlusion"), b2], opt, skip_prim_ids=[i0, i1, None])
    if prec == "f32":
        assert a.LastKernelName().endswith("false, false, 4, 2>"), a.LastKernelName()
    assert_hits_identical(want0[0], want0[1], got[0][0], got[0][1])
    assert np.array_equal(got[1][1], want1)
    assert_hits_identical(want2[0], want2[1], got[2][0], got[2][1])
    # a NULL array of pointers is the call without ids
    plain = a.TraverseBatches([b0, (b1, "occlusion"), b2], opt)
    none = a.TraverseBatches([b0, (b1, "occlusion"), b2], opt, skip_prim_ids=[None, None, None])
    for k in (0, 2):
        assert_hits_identical(plain[k][0], plain[k][1], none[k][0], none[k][1])
    assert np.array_equal(plain[1][1], none[1][1])
    # the device form
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).cuda()
    d = [(dev(b0), torch.zeros(b0.shape[0] * HIT.itemsize, dtype=torch.uint8, device="cuda"), torch.zeros(b0.shape[0], dtype=torch.uint8, device="cuda")),
         (dev(b1), None, torch.zeros(b1.shape[0], dtype=torch.uint8, device="cuda"), None, "occlusion"),
         (dev(b2), torch.zeros(b2.shape[0] * HIT.itemsize, dtype=torch.uint8, device="cuda"), torch.zeros(b2.shape[0], dtype=torch.uint8, device="cuda"))]
    torch.cuda.synchronize()
    a.TraverseBatchesDevice(d, opt, skip_prim_ids=[dev(i0), dev(i1), None])
    torch.cuda.synchronize()
    assert_hits_identical(want0[0], want0[1], d[0][1].cpu().numpy().view(HIT), d[0][2].cpu().numpy())
    assert np.array_equal(d[1][2].cpu().numpy(), want1)
    assert_hits_identical(want2[0], want2[1], d[2][1].cpu().numpy().view(HIT), d[2][2].cpu().numpy())


def test_refusals_write_nothing(w32, w64):
    import torch

    L = capi.lib()
    n = 64
    rays = eye_rays(n, np.float32)
    ids = np.zeros(n, dtype=np.uint32)
    sc, sr = scenes.random_spheres(64)
    cv, cr = scenes.random_cylinders(64)
    cps, radii = scenes.synthetic_hair(64)
    others = []
    for geom in (SphereGeometry(sc, sr), CylinderGeometry(cv, cr), CurveGeometry(cps, radii)):
        a = BVHAccel(np.float32)
        assert a.Build(64, geom)
        others.append(a)

    def refused(a, status, call, *outs):
        before = [o.copy() for o in outs]
        assert call() == status
        msg = L.nrtLastError(a._h).decode()
        assert ("precision" if status == capi.NRT_ERR_PRECISION else "skip ids") in msg, msg
        for o, b in zip(outs, before):
            assert o.tobytes() == b.tobytes(), "a refusal wrote to an output"

    for a in others:  # sphere, cylinder and curve contexts: their intersectors have no skip id
        h = np.full(n * 16, 0xAB, dtype=np.uint8)
        m = np.full(n, 0xAB, dtype=np.uint8)
        refused(a, capi.NRT_ERR_INVALID, lambda: L.nrtTraverseBatchSkip_f32(a._h, _vp(rays), n, None, _vp(ids), _vp(h), _vp(m)), h, m)
        refused(a, capi.NRT_ERR_INVALID, lambda: L.nrtOccludedBatchSkip_f32(a._h, _vp(rays), n, None, _vp(ids), _vp(m)), m)
        rp = (ctypes.c_void_p * 1)(rays.ctypes.data)
        ip = (ctypes.c_void_p * 1)(ids.ctypes.data)
        hp = (ctypes.c_void_p * 1)(h.ctypes.data)
        mp = (ctypes.c_void_p * 1)(m.ctypes.data)
        cnt = (ctypes.c_uint64 * 1)(n)
        refused(a, capi.NRT_ERR_INVALID, lambda: L.nrtTraverseBatchesSkip_f32(a._h, 1, rp, cnt, None, ip, hp, mp, None), h, m)
    # the wrong precision
    h = np.full(n * 16, 0xAB, dtype=np.uint8)
    m = np.full(n, 0xAB, dtype=np.uint8)
    refused(w64.a, capi.NRT_ERR_PRECISION, lambda: L.nrtTraverseBatchSkip_f32(w64.a._h, _vp(rays), n, None, _vp(ids), _vp(h), _vp(m)), h, m)
    rays64 = eye_rays(n, np.float64)
    h64 = np.full(n * 32, 0xAB, dtype=np.uint8)
    refused(w32.a, capi.NRT_ERR_PRECISION, lambda: L.nrtTraverseBatchSkip_f64(w32.a._h, _vp(rays64), n, None, _vp(ids), _vp(h64), _vp(m)), h64, m)
    refused(w32.a, capi.NRT_ERR_PRECISION, lambda: L.nrtOccludedBatchSkip_f64(w32.a._h, _vp(rays64), n, None, _vp(ids), _vp(m)), m)
    # a device array that is not 4-byte aligned
    d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    d_ids = torch.zeros(4 * n + 4, dtype=torch.uint8, device="cuda")
    d_hits = torch.full((16 * n,), 0xAB, dtype=torch.uint8, device="cuda")
    d_mask = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a = w32.a
    for off in (1, 2):
        assert L.nrtTraverseBatchSkipDevice_f32(a._h, d_rays.data_ptr(), n, None, d_ids.data_ptr() + off, d_hits.data_ptr(), d_mask.data_ptr(), None) == capi.NRT_ERR_INVALID
        assert "aligned" in L.nrtLastError(a._h).decode()
        assert L.nrtOccludedBatchSkipDevice_f32(a._h, d_rays.data_ptr(), n, None, d_ids.data_ptr() + off, d_mask.data_ptr(), None) == capi.NRT_ERR_INVALID
    torch.cuda.synchronize()
    assert (d_hits.cpu().numpy() == 0xAB).all() and (d_mask.cpu().numpy() == 0xAB).all()
    # ... and the aligned call on the same buffers works
    assert L.nrtTraverseBatchSkipDevice_f32(a._h, d_rays.data_ptr(), n, None, d_ids.data_ptr() + 4, d_hits.data_ptr(), d_mask.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (d_mask.cpu().numpy() == 1).all()


def test_header_traverse_batch_with_ids(tmp_path):
    """include/nanort.h with NANORT_USE_HIP_BACKEND: BVHAccel::TraverseBatch / OccludedBatch with skip_prim_ids against the accel's own
    per-ray CPU Traverse() with per-ray options (tests/cpp/skip_ids_check.cc)."""
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "nanort_amd", "lib")
    exe = tmp_path / "skip_ids_check_hip"
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-DNANORT_USE_HIP_BACKEND", "-D__HIP_PLATFORM_AMD__", "-I", inc, "-isystem",
                        "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "skip_ids_check.cc"), "-o", str(exe), "-L", libdir, "-lnanort_hip",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    rr = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert rr.returncode == 0, rr.stdout
    assert "batch_vs_per_ray_mismatches 0" in rr.stdout and "occluded_vs_per_ray_mismatches 0" in rr.stdout and "null_array_same 1" in rr.stdout, rr.stdout

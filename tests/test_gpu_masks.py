"""Visibility masks on the GPU (nanort_amd/csrc/own_walks.hip; include/nanort_hip.h, "visibility masks"): one 32-bit word
per triangle, one per ray, and a triangle exists for a ray iff the two share a bit.

Parity is exact.  For the rays that share one mask word the expected records are oracle.traverse — the project's pinned restatement
of the reference — over the CONTEXT'S OWN node array and the faces with every invisible one collapsed to a point
(tests/masks_fixture.py says why that is "the intersector returns false", bit for bit); the masked walk is the literal binary loop,
so every byte of every record and flag must match (assert_hits_identical, no tolerance).  Neighbouring rays carry different words
(masks_fixture.assign_ray_masks), the `mod3` words are not invariant under the builder's permutation of the faces, and
tests/test_masks_model.py asserts that the masks change the records: a walk that dropped, mis-indexed or ignored a word fails here."""
import os
import subprocess

import numpy as np
import pytest

import masks_fixture as kf
import size_thresholds as sz
from helpers import assert_hits_identical, trace_options
from nanort_amd import BVHAccel, CurveGeometry, CylinderGeometry, SphereGeometry, TriangleMesh, scenes
from nanort_amd.capi import NRT_ERR_INVALID, NrtError
from nanort_amd.wire import widen_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REALS = [np.float32, np.float64]
PATTERNS = ["random", "zeros", "ones", "bit31", "mod3"]


def odd_count(rays):
    """The same rays, trimmed so that their count is no multiple of 64 (the last wave of the launch is a partial one)."""
    n = rays.shape[0]
    n -= 37 if n % 64 == 0 else 0
    assert n % 64 != 0 and n > 128  # (above one claim chunk: lanes are refilled)
    return np.ascontiguousarray(rays[:n])


def window_rays(rays, seed):
    """The same rays with random [min_t, max_t] windows around the mesh (the camera is 15 to 25 away from it): some windows end in
    front of the hit, some begin behind it, some hold it."""
    rng = np.random.default_rng(seed)
    r = rays.copy()
    a = rng.uniform(0, 22, size=r.shape[0])
    r["min_t"], r["max_t"] = a, a + rng.uniform(0, 12, size=r.shape[0])
    return r


class World:
    """One precision: C1's mesh and four ray sets with their per-ray words (computed once): the camera wave, its bounce, random
    [min_t, max_t] windows, and the camera turned to look through the box's closed walls (masks_fixture.through_rays)."""

    def __init__(self, real, c1_mesh):
        self.real = real
        v, f = c1_mesh
        self.v = np.ascontiguousarray(v.astype(real))
        self.f = np.ascontiguousarray(f, dtype=np.uint32)
        cam = scenes.camera_rays(96, 64)
        a32 = BVHAccel(np.float32)
        a32.Build(f.shape[0], TriangleMesh(v.astype(np.float32), f))
        h32, m32 = a32.TraverseBatch(cam)
        bounce = scenes.secondary_rays("bounce", v.astype(np.float32), f, cam, h32, m32)
        a32.close()
        through = kf.through_rays(cam)
        if real == np.float64:
            cam, bounce, through = widen_rays(cam), widen_rays(bounce), widen_rays(through)
        self.sets = [odd_count(cam), odd_count(bounce), odd_count(window_rays(cam, 3)), odd_count(through)]
        self.words = [kf.assign_ray_masks(r.shape[0], seed=3 + k) for k, r in enumerate(self.sets)]
        self.kernel = "nrt::k_traverse_masked<%s>" % ("float" if real == np.float32 else "double")

    def built(self, n_faces=None):
        f = self.f if n_faces is None else self.f[:n_faces]
        a = BVHAccel(self.real)
        assert a.Build(f.shape[0], TriangleMesh(self.v, f))
        return a, f


@pytest.fixture(scope="module", params=REALS, ids=["f32", "f64"])
def w(request, c1_mesh):
    return World(request.param, c1_mesh)


@pytest.fixture(scope="module")
def w32(c1_mesh):
    return World(np.float32, c1_mesh)


def check_queries(oracle, a, w, v, f, pm, opts=None, sets=None, min_hits=None):
    """Records, flags, occlusion flags and the kernel's name for the ray sets `sets` against the expectation over the accel's own tree."""
    nodes, idx = a.GetTree()
    total = 0
    for k in (range(len(w.sets)) if sets is None else sets):
        rays, words = w.sets[k], w.words[k]
        eh, em = kf.expected(oracle, nodes, idx, v, f, pm, rays, words, opts)
        total += int(em.sum())
        h, m = a.TraverseBatchMasked(rays, words, opts)
        assert a.LastKernelName() == w.kernel
        assert_hits_identical(eh, em, h, m)
        assert np.array_equal(a.OccludedBatchMasked(rays, words, opts), em)
        assert a.LastKernelName() == w.kernel
        if min_hits is not None:
            assert em.sum() > min_hits, (k, em.sum())
    return nodes, idx, total


def refused(call, status, names):
    with pytest.raises(NrtError) as e:
        call()
    assert e.value.status == status, e.value
    text = str(e.value).split(": ", 1)[1].strip()
    assert text, "empty nrtLastError"
    assert names in text, "the message does not name the call: %r" % text


# ---- 1. records and flags ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_faces", [1, 2, 5, 513, None])
def test_records_and_flags_for_every_pattern(oracle, w, n_faces):
    """Every prim pattern on one accel: the words change between the queries, the tree is built once."""
    a, f = w.built(n_faces)
    tree0 = a.GetTree()
    pats = kf.prim_patterns(f.shape[0])
    for name in PATTERNS:
        a.SetPrimMasks(pats[name])
        full = n_faces is None
        check_queries(oracle, a, w, w.v, f, pats[name], sets=None if full else (0, 3), min_hits=100 if (full and name == "random") else None)
    tree1 = a.GetTree()
    assert tree1[0].tobytes() == tree0[0].tobytes() and tree1[1].tobytes() == tree0[1].tobytes(), "setting masks changed the tree"
    a.close()


# ---- 2. order and lifetime -----------------------------------------------------------------------------------------------------
def test_masks_before_and_after_build_settree_and_refit(oracle, w):
    f = w.f
    pats = kf.prim_patterns(f.shape[0])
    # masks set BEFORE the build (they need the mesh only) survive it
    a = BVHAccel(w.real)
    a.SetMesh(TriangleMesh(w.v, f))
    a.SetPrimMasks(pats["mod3"])
    assert a.BuildCurrent()
    check_queries(oracle, a, w, w.v, f, pats["mod3"], sets=(0, 3))
    # ... and set after it, with no build between: the tree is the same bytes
    n0, i0 = a.GetTree()
    a.SetPrimMasks(pats["random"])
    n1, i1, _ = check_queries(oracle, a, w, w.v, f, pats["random"], sets=(0, 3))
    assert n1.tobytes() == n0.tobytes() and i1.tobytes() == i0.tobytes()
    # an adopted tree with another leaf order: the masks stay, their leaf-order copy follows the new order
    onodes, oidx, _ = oracle.build(w.v, f)
    assert oidx.tobytes() != i0.tobytes(), "fixture: the oracle's leaf order equals the builder's"
    a.SetTree(onodes, oidx)
    check_queries(oracle, a, w, w.v, f, pats["random"], sets=(0, 3))
    a.SetPrimMasks(pats["mod3"])  # (set after SetTree)
    check_queries(oracle, a, w, w.v, f, pats["mod3"], sets=(3,))
    # a refit to jittered vertices keeps the masks and the order
    rng = np.random.default_rng(5)
    v2 = np.ascontiguousarray((w.v + rng.normal(scale=1e-2, size=w.v.shape)).astype(w.real))
    a.Refit(v2)
    check_queries(oracle, a, w, v2, f, pats["mod3"], sets=(0, 3))
    a.SetPrimMasks(pats["random"])  # (set after Refit)
    check_queries(oracle, a, w, v2, f, pats["random"], sets=(3,))
    # a rebuild keeps them too
    assert a.BuildCurrent()
    check_queries(oracle, a, w, v2, f, pats["random"], sets=(1,))
    a.close()


def test_removed_masks_and_setmesh(oracle, w):
    f = w.f
    pats = kf.prim_patterns(f.shape[0])
    rays, words = w.sets[0], w.words[0]
    a, _ = w.built()
    plain0 = a.TraverseBatch(rays)
    plain_kernel = a.LastKernelName()
    # no masks yet: refused, naming the call
    refused(lambda: a.TraverseBatchMasked(rays, words), NRT_ERR_INVALID, "nrtTraverseBatchMasked")
    refused(lambda: a.OccludedBatchMasked(rays, words), NRT_ERR_INVALID, "nrtOccludedBatchMasked")
    a.SetPrimMasks(pats["random"])
    check_queries(oracle, a, w, w.v, f, pats["random"], sets=(0,))
    # a plain query on a context that holds masks ignores them: the same kernel, the same bits (fp64 records carry 4 padding bytes,
    # which nothing writes: assert_hits_identical compares the four fields bit for bit)
    plain1 = a.TraverseBatch(rays)
    assert a.LastKernelName() == plain_kernel
    assert_hits_identical(*plain0, *plain1)
    # removed: refused again, the plain query unchanged, the tree still there
    a.SetPrimMasks(None)
    assert a.IsValid()
    refused(lambda: a.TraverseBatchMasked(rays, words), NRT_ERR_INVALID, "nrtTraverseBatchMasked")
    assert_hits_identical(*plain0, *a.TraverseBatch(rays))
    # SetMesh drops the masks
    a.SetPrimMasks(pats["mod3"])
    a.SetMesh(TriangleMesh(w.v, f))
    assert a.BuildCurrent()
    refused(lambda: a.TraverseBatchMasked(rays, words), NRT_ERR_INVALID, "nrtTraverseBatchMasked")
    a.close()


# ---- 3. trace options ----------------------------------------------------------------------------------------------------------
OPTIONS = {
    "range": dict(range_=(100, 700)),
    "skip": dict(skip=412),
    "cull": dict(cull=True),
    "all": dict(range_=(50, 900), skip=412, cull=True),
}


@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_records_and_flags_under_trace_options(oracle, w, opt):
    a, f = w.built()
    pm = kf.prim_patterns(f.shape[0])["random"]
    a.SetPrimMasks(pm)
    _, _, total = check_queries(oracle, a, w, w.v, f, pm, opts=trace_options(**OPTIONS[opt]), sets=(0, 1, 3))
    assert total > 0  # (not vacuous; the id range keeps a part of the mesh, culling little of a box seen from inside)
    a.close()


# ---- 4. NULL ray masks, all-ones words -----------------------------------------------------------------------------------------
def test_null_ray_masks_are_all_ones_and_all_ones_is_the_plain_query(oracle, w):
    a, f = w.built()
    pats = kf.prim_patterns(f.shape[0])
    nodes, idx = a.GetTree()
    for k in (0, 3):
        rays = w.sets[k]
        ones = np.full(rays.shape[0], 0xFFFFFFFF, dtype=np.uint32)
        a.SetPrimMasks(pats["random"])
        eh, em = kf.expected(oracle, nodes, idx, w.v, f, pats["random"], rays, None)
        for words in (None, ones):
            assert_hits_identical(eh, em, *a.TraverseBatchMasked(rays, words))
            assert np.array_equal(a.OccludedBatchMasked(rays, words), em)
        # all-ones on both sides: the records of the plain query, bit for bit in every field
        a.SetPrimMasks(pats["ones"])
        ph, pmask = a.TraverseBatch(rays)
        for words in (None, ones):
            assert_hits_identical(ph, pmask, *a.TraverseBatchMasked(rays, words))
        assert pmask.sum() > 100
    a.close()


# ---- 5. device forms -----------------------------------------------------------------------------------------------------------
def test_device_forms_on_a_side_stream(oracle, w):
    import torch

    a, f = w.built()
    pm = kf.prim_patterns(f.shape[0])["mod3"]
    side = torch.cuda.Stream()
    d_pm = torch.from_numpy(pm.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    a.SetPrimMasksDevice(d_pm, stream=side)
    d_pm.zero_()  # (the accel owns its copy)
    nodes, idx = a.GetTree()
    rays, words = w.sets[3], w.words[3]
    n = rays.shape[0]
    eh, em = kf.expected(oracle, nodes, idx, w.v, f, pm, rays, words)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    # the words: a view one element into a larger tensor
    big = torch.full((n + 5,), -1, dtype=torch.int32, device="cuda")
    big[1:1 + n] = torch.from_numpy(words.view(np.int32).copy()).cuda()
    d_words = big[1:1 + n]
    assert d_words.data_ptr() == big.data_ptr() + 4
    d_hits = torch.zeros((n * eh.dtype.itemsize,), dtype=torch.uint8, device="cuda")
    d_mask = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    d_occ = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a.TraverseBatchMaskedDevice(d_rays, d_words, d_hits, d_mask, stream=side)
    assert a.LastKernelName() == w.kernel
    a.OccludedBatchMaskedDevice(d_rays, d_words, d_occ, stream=side)
    # nrtSetPrimMasks right behind the Device launches waits for them (the next masked query rewrites the array they read)
    a.SetPrimMasks(kf.prim_patterns(f.shape[0])["zeros"])
    side.synchronize()
    h = np.frombuffer(d_hits.cpu().numpy().tobytes(), dtype=eh.dtype)
    assert_hits_identical(eh, em, h, d_mask.cpu().numpy())
    assert np.array_equal(d_occ.cpu().numpy(), em)
    assert em.sum() > 100
    # the same records as the host forms
    a.SetPrimMasks(pm)
    assert_hits_identical(eh, em, *a.TraverseBatchMasked(rays, words))
    # a misaligned word array is refused before anything is enqueued
    raw = torch.zeros((4 * n + 8,), dtype=torch.uint8, device="cuda")
    odd = raw[1:1 + 4 * n]
    assert odd.data_ptr() % 4 != 0
    refused(lambda: a.TraverseBatchMaskedDevice(d_rays, odd, d_hits, d_mask, stream=side), NRT_ERR_INVALID, "nrtTraverseBatchMasked")
    refused(lambda: a.OccludedBatchMaskedDevice(d_rays, odd, d_occ, stream=side), NRT_ERR_INVALID, "nrtOccludedBatchMasked")
    refused(lambda: a._check(a._L.nrtSetPrimMasksDevice(a._h, raw.data_ptr() + 1, f.shape[0], None)), NRT_ERR_INVALID, "nrtSetPrimMasksDevice")
    assert_hits_identical(eh, em, *a.TraverseBatchMasked(rays, words))  # (the refused setter left the masks as they were)
    a.close()


# ---- 6. pieced host loop -------------------------------------------------------------------------------------------------------
def test_host_call_in_pieces_advances_the_ray_masks(oracle, w32):
    """kPiece + 4093 rays through the staged host path: two pieces; each ray's word is a function of its index (index mod 4093, and
    kPiece mod 4093 = 384), so a second piece staged with the first one's words, or with another offset, fails."""
    w = w32
    assert sz.source_cap("kPiece") == sz.PIECE
    a, f = w.built()
    pm = kf.prim_patterns(f.shape[0])["random"]
    a.SetPrimMasks(pm)
    nodes, idx = a.GetTree()
    base = sz.cut(np.concatenate([w.sets[0], w.sets[3]]))
    bw = kf.assign_ray_masks(sz.B, seed=21)
    eh, em = kf.expected(oracle, nodes, idx, w.v, f, pm, base, bw)
    n = sz.PIECE + sz.B
    assert sz.crossing_trips(n, sz.PIECE) == 2 and sz.PIECE % sz.B != 0
    rays, words = sz.tiled(base, n), sz.tiled(bw, n)
    h, m = a.TraverseBatchMasked(rays, words)
    assert_hits_identical(sz.tiled(eh, n), sz.tiled(em, n), h, m)
    assert np.array_equal(a.OccludedBatchMasked(rays, words), sz.tiled(em, n))
    assert em.sum() > 100
    a.close()


def test_pipelined_host_call_carries_each_pieces_ray_masks(oracle, w32):
    """2 * kPiece + 4093 rays from page-locked arrays: the three-stream pipeline of the host form, three pieces over two staging slots;
    the words travel with their piece's rays (a slot reused for the third piece must hold the third piece's words)."""
    import torch

    w = w32
    a, f = w.built()
    pm = kf.prim_patterns(f.shape[0])["mod3"]
    a.SetPrimMasks(pm)
    nodes, idx = a.GetTree()
    base = sz.cut(np.concatenate([w.sets[0], w.sets[3]]))
    bw = kf.assign_ray_masks(sz.B, seed=22)
    eh, em = kf.expected(oracle, nodes, idx, w.v, f, pm, base, bw)
    n = 2 * sz.PIECE + sz.B
    assert sz.crossing_trips(n, sz.PIECE) == 3
    p_r = torch.empty(n * base.dtype.itemsize, dtype=torch.uint8, pin_memory=True)
    p_w = torch.empty(n, dtype=torch.int32, pin_memory=True)
    p_h = torch.full((n * eh.dtype.itemsize,), 0xA5, dtype=torch.uint8).pin_memory()
    p_m = torch.full((n,), 0xA5, dtype=torch.uint8).pin_memory()
    assert p_r.is_pinned() and p_w.is_pinned() and p_h.is_pinned() and p_m.is_pinned()
    p_r.numpy().view(base.dtype)[:] = sz.tiled(base, n)
    p_w.numpy().view(np.uint32)[:] = sz.tiled(bw, n)
    st = a._L.nrtTraverseBatchMasked_f32(a._h, p_r.data_ptr(), p_w.data_ptr(), n, None, p_h.data_ptr(), p_m.data_ptr())
    assert st == 0, a._L.nrtLastError(a._h)
    assert a.LastKernelName() == w.kernel
    assert_hits_identical(sz.tiled(eh, n), sz.tiled(em, n), p_h.numpy().view(eh.dtype), p_m.numpy())
    assert em.sum() > 100
    a.close()


# ---- 7. entry errors -----------------------------------------------------------------------------------------------------------
def test_other_primitive_kinds_are_refused():
    rays = scenes.camera_rays(8, 8)
    words = np.ones(rays.shape[0], dtype=np.uint32)
    c, r = scenes.random_spheres(64)
    e, er = scenes.random_cylinders(64)
    cps, cr = scenes.synthetic_hair(64)
    for geom, kind in ((SphereGeometry(c, r), "sphere"), (CylinderGeometry(e, er), "cylinder"), (CurveGeometry(cps, cr), "curve")):
        a = BVHAccel(np.float32)
        assert a.Build(geom.num_faces, geom)
        refused(lambda: a.SetPrimMasks(np.ones(64, dtype=np.uint32)), NRT_ERR_INVALID, "nrtSetPrimMasks")
        with pytest.raises(NrtError) as err:
            a.SetPrimMasks(np.ones(64, dtype=np.uint32))
        assert kind in str(err.value), "the message does not name the kind: %s" % err.value
        refused(lambda: a.TraverseBatchMasked(rays, words), NRT_ERR_INVALID, "nrtTraverseBatchMasked")
        refused(lambda: a.OccludedBatchMasked(rays, words), NRT_ERR_INVALID, "nrtOccludedBatchMasked")
        assert a.IsValid()
        assert a.OccludedBatch(rays).shape[0] == rays.shape[0]
        a.close()


def test_wrong_count_and_no_mesh_are_refused(oracle, w):
    a = BVHAccel(w.real)
    refused(lambda: a.SetPrimMasks(np.ones(4, dtype=np.uint32)), NRT_ERR_INVALID, "nrtSetPrimMasks")  # no mesh
    a.SetMesh(TriangleMesh(w.v, w.f))
    nf = w.f.shape[0]
    for count in (nf - 1, nf + 1, 1):
        refused(lambda: a.SetPrimMasks(np.ones(count, dtype=np.uint32)), NRT_ERR_INVALID, "nrtSetPrimMasks")
    # a refused setter leaves the masks that were there
    assert a.BuildCurrent()
    pm = kf.prim_patterns(nf)["mod3"]
    a.SetPrimMasks(pm)
    refused(lambda: a.SetPrimMasks(np.ones(nf + 1, dtype=np.uint32)), NRT_ERR_INVALID, "nrtSetPrimMasks")
    check_queries(oracle, a, w, w.v, w.f, pm, sets=(3,))
    a.close()


# ---- 8. include/nanort.h with the backend ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header_check(tmp_path_factory):
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "nanort_amd", "lib")
    exe = str(tmp_path_factory.mktemp("masks_check") / "masks_check")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", inc, os.path.join(ROOT, "tests", "cpp", "masks_check.cc"),
                        "-o", exe, "-DNANORT_USE_HIP_BACKEND", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include", "-L", libdir, "-lnanort_hip",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


@pytest.mark.parametrize("opt", ["default", "all"])
def test_header_backend_equals_its_own_host_walk(header_check, tmp_path, w, opt):
    """GPU Build() over TriangleMesh, SetPrimMasks(); TraverseBatchMasked / OccludedBatchMasked against the header's per-ray
    Traverse() with a MaskedTriangleIntersector over the read-back tree, byte for byte, inside tests/cpp/masks_check.cc; the masks
    changed with no Build(); a copy keeps its own."""
    real = w.real
    rays, words = w.sets[3], w.words[3]
    pats = kf.prim_patterns(w.f.shape[0])
    mesh, rp = (os.path.join(str(tmp_path), x) for x in ("mesh.bin", "rays.bin"))
    with open(mesh, "wb") as fp:
        fp.write(np.array([w.v.shape[0], w.f.shape[0]], dtype=np.uint32).tobytes() + w.v.tobytes() + w.f.tobytes() + pats["random"].tobytes()
                 + pats["mod3"].tobytes())
    with open(rp, "wb") as fp:
        fp.write(np.array([rays.shape[0]], dtype=np.uint64).tobytes() + rays.tobytes() + words.tobytes())
    o = trace_options(**(OPTIONS["all"] if opt == "all" else {}))
    o = o[()] if o.shape == () else o[0]
    r = subprocess.run([header_check, "f32" if real == np.float32 else "f64", mesh, rp, str(int(o["prim_ids_range"][0])), str(int(o["prim_ids_range"][1])),
                        str(int(o["skip_prim_id"])), str(int(o["cull_back_face"]))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    word, hits, n = r.stdout.split()[-3:]
    assert word == "ok" and int(n) == rays.shape[0] and int(hits) > (500 if opt == "default" else 0)

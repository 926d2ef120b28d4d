"""Multi-hit with per-ray skip ids, visibility words and motion times on the GPU (include/nanort_hip.h, nrtMultiHitQueryBatch*;
DESIGN.md 3.16; nanort_amd/csrc/own_walks.hip).

  1. shells: every combination through the Device form, K = 2, all three at K = 1 and 4, and under two sets of trace options;
  2. pile: all three at K = 4 and 64, past the walk's 32 LDS stack entries;
  3. routing: a descriptor with no flag and no ids is nrtMultiHitTraverseBatch*; the new kernel with nothing to apply gives its bytes;
  4. K = 1 against QueryBatchDevice of the same library;
  5. the host form against the Device form: one piece, a piece crossing of the staged rows, no counts;
  6. every refusal: status, a message naming the entry point, outputs untouched;
  7. the prim masks changed between two masked multi-hit queries with no build;
  8. include/nanort.h with the backend against the header's own host form;
  9. nrtMultiHitTraverseBatchDevice still gives multihit_fixture.model's bytes.

1 and 2 are exact against the expectation of tests/multihit_query_fixture.py over the context's own node array: every field of
every record of every row and every count, no tolerance.  The fixture conditions hold for the model alone:
tests/test_multihit_query_model.py asserts them without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import masks_fixture as kf
import multihit_fixture as mhf
import multihit_query_fixture as mq
import own_walks_fixture as ow
import query_fixture as qf
import size_thresholds as sz
from helpers import trace_options
from nanort_amd import BVHAccel, MotionTriangleMesh, SphereGeometry, TriangleMesh, capi, scenes
from nanort_amd.capi import NRT_ERR_INVALID, NRT_ERR_PRECISION, NRT_OK, NRT_QUERY_MASKED, NRT_QUERY_MOTION, NRT_QUERY_OCCLUSION
from nanort_amd.wire import hit_dtype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REALS = [np.float32, np.float64]
IDS = ["f32", "f64"]
FILL = 0xA5  # every output byte before a call: no record and no count holds it


def _c(real):
    return "float" if np.dtype(real) == np.float32 else "double"


def kernel_name(real, motion, masked):
    return "nrt::k_multihit_query<%s, 32, %s, %s>" % (_c(real), str(bool(motion)).lower(), str(bool(masked)).lower())


def plain_name(real):
    return "nrt::k_traverse_multihit<%s>" % _c(real)


def accel_of(w, masks=True):
    a = BVHAccel(w.real)
    a.SetMesh(MotionTriangleMesh(w.v, w.v1, w.f))
    a.SetTree(w.nodes, w.idx)
    if masks:
        a.SetPrimMasks(w.pm)
    return a


class Dev:
    """A world's rays and per-ray arrays in HBM, tiled to n rays (n None: as they are)."""

    def __init__(self, w, n=None):
        import torch

        self.torch = torch
        self.hit_t = hit_dtype(w.real)
        pick = (lambda x: x) if n is None else (lambda x: sz.tiled(x, n))
        self.n = w.rays.shape[0] if n is None else n
        self.rays = torch.from_numpy(np.ascontiguousarray(pick(w.rays)).view(np.uint8).copy()).cuda()
        self.times = torch.from_numpy(np.ascontiguousarray(pick(w.times)).copy()).cuda()
        self.words = torch.from_numpy(np.ascontiguousarray(pick(w.words)).view(np.int32).copy()).cuda()
        self.ids = torch.from_numpy(np.ascontiguousarray(pick(w.ids)).view(np.int32).copy()).cuda()

    def outputs(self, K):
        t = self.torch
        return (t.full((self.n * K * self.hit_t.itemsize,), FILL, dtype=t.uint8, device="cuda"), t.full((self.n * 4,), FILL, dtype=t.uint8, device="cuda"))

    def rows(self, d_h, K):
        return np.frombuffer(d_h.cpu().numpy().tobytes(), dtype=self.hit_t).reshape(self.n, K)

    def counts(self, d_c):
        return np.frombuffer(d_c.cpu().numpy().tobytes(), dtype=np.uint32)

    def query(self, a, K, motion, masked, ids, opts=None, times="own", words="own", skip="own", counts=True):
        """The Device form; (rows[n, K], counts or the untouched fill) on the host.  times / words / skip: "own", a tensor, or None."""
        d_h, d_c = self.outputs(K)
        pick = lambda given, own: own if isinstance(given, str) else given  # noqa: E731
        a.MultiHitQueryBatchDevice(self.rays, K, d_h, d_c if counts else None, times=pick(times, self.times) if motion else None,
                                   ray_masks=pick(words, self.words) if masked else None, skip_prim_ids=pick(skip, self.ids) if ids else None,
                                   motion=motion, masked=masked, options=opts)
        self.torch.cuda.synchronize()
        return self.rows(d_h, K), self.counts(d_c)

    def plain(self, a, K, opts=None):
        """nrtMultiHitTraverseBatchDevice."""
        d_h, d_c = self.outputs(K)
        a.MultiHitTraverseBatchDevice(self.rays, K, d_h.view(self.torch.uint8), d_c.view(self.torch.int32), options=opts)
        self.torch.cuda.synchronize()
        return self.rows(d_h, K), self.counts(d_c)


def check_combo(oracle, a, d, name, real, K, combo, opts=None, min_held=100):
    motion, masked, ids = mq.COMBOS[combo]
    eh, ec = mq.expect(oracle, name, real, K, motion=motion, masked=masked, ids=ids, opts=opts)
    assert ec.sum() > min_held, (combo, ec.sum())
    h, c = d.query(a, K, motion, masked, ids, opts=opts)
    assert a.LastKernelName() == kernel_name(real, motion, masked), a.LastKernelName()
    mq.assert_rows_identical(eh, ec, h, c)


# ---- 1. shells ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo,K", [(k, 2) for k in sorted(mq.COMBOS)] + [("all", 1), ("all", 4)])
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_shells_every_combination(oracle, real, combo, K):
    w = mq.world(oracle, "shells", real)
    a, d = accel_of(w), Dev(w)
    check_combo(oracle, a, d, "shells", real, K, combo)
    a.close()


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_shells_all_three_under_trace_options(oracle, real):
    """An id range and back-face culling on top of the three per-ray things; the skip id stays per ray.  The first options leave next
    to nothing (a range inside the innermost shell, culled), exact all the same; the second keep most of the shells."""
    w = mq.world(oracle, "shells", real)
    a, d = accel_of(w), Dev(w)
    check_combo(oracle, a, d, "shells", real, 2, "all", opts=qf.shell_options(), min_held=0)
    check_combo(oracle, a, d, "shells", real, 2, "all", opts=trace_options(range_=(50, 3900), skip=412))
    a.close()


# ---- 2. pile ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 64])
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_pile_all_three_past_the_lds_stack(oracle, real, K):
    w = mq.world(oracle, "pile", real)
    assert w.stats["max_tree_depth"] > ow.PILE_MIN_STACK
    a, d = accel_of(w), Dev(w)
    check_combo(oracle, a, d, "pile", real, K, "all")
    a.close()


# ---- 3. routing ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_routing(oracle, real):
    w = mq.world(oracle, "shells", real)
    assert (w.pm != 0).all()  # (all-ones ray words see every face)
    a, d = accel_of(w), Dev(w)
    torch = d.torch
    K = 4
    ph, pc = d.plain(a, K)
    assert a.LastKernelName() == plain_name(real) and pc.sum() > 1000
    # no flag, no ids: the same kernel, the same bytes
    h, c = d.query(a, K, False, False, False)
    assert a.LastKernelName() == plain_name(real)
    mq.assert_rows_identical(ph, pc, h, c)
    hh, hc = a.MultiHitQueryBatch(w.rays, K)
    assert a.LastKernelName() == plain_name(real)
    mq.assert_rows_identical(ph, pc, hh, hc)
    # the new kernel with nothing to apply
    n = d.n
    ones = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    h, c = d.query(a, K, True, False, False, times=None)  # MOTION, NULL times: every ray at time 0
    assert a.LastKernelName() == kernel_name(real, True, False)
    mq.assert_rows_identical(ph, pc, h, c)
    h, c = d.query(a, K, False, True, False, words=None)  # MASKED, NULL words: every ray 0xFFFFFFFF
    assert a.LastKernelName() == kernel_name(real, False, True)
    mq.assert_rows_identical(ph, pc, h, c)
    h, c = d.query(a, K, False, False, True, skip=ones)  # ids, all 0xFFFFFFFF
    assert a.LastKernelName() == kernel_name(real, False, False)
    mq.assert_rows_identical(ph, pc, h, c)
    a.SetPrimMasks(np.full(w.f.shape[0], 0xFFFFFFFF, dtype=np.uint32))
    h, c = d.query(a, K, False, True, False, words=ones)  # MASKED, all-ones words on both sides (a ray word of 0 sees nothing whatever the masks)
    assert a.LastKernelName() == kernel_name(real, False, True)
    mq.assert_rows_identical(ph, pc, h, c)
    h, c = d.query(a, K, True, True, True, times=None, words=ones, skip=ones)  # all of the above together
    assert a.LastKernelName() == kernel_name(real, True, True)
    mq.assert_rows_identical(ph, pc, h, c)
    a.close()


# ---- 4. K = 1 against the combined closest-hit query ----------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_k1_against_query_batch_device(oracle, real):
    w = mq.world(oracle, "shells", real)
    a, d = accel_of(w), Dev(w)
    torch = d.torch
    h1, c1 = d.query(a, 1, True, True, True)
    d_h = torch.full((d.n * d.hit_t.itemsize,), FILL, dtype=torch.uint8, device="cuda")
    d_m = torch.full((d.n,), FILL, dtype=torch.uint8, device="cuda")
    a.QueryBatchDevice(d.rays, d_h, d_m, times=d.times, ray_masks=d.words, skip_prim_ids=d.ids)
    torch.cuda.synchronize()
    ch, cm = np.frombuffer(d_h.cpu().numpy().tobytes(), dtype=d.hit_t), d_m.cpu().numpy()
    assert np.array_equal(c1, cm.astype(np.uint32)) and cm.sum() > 1000
    t1, tc = h1[:, 0]["t"], ch["t"]
    assert np.array_equal(t1, tc)
    nz = t1 != 0
    assert np.ascontiguousarray(t1[nz]).tobytes() == np.ascontiguousarray(tc[nz]).tobytes()
    a.close()


# ---- 5. the host form ---------------------------------------------------------------------------------------------------------------
def host_query(a, K, rays, times, words, ids, counts=True):
    """nrtMultiHitQueryBatch with all three over the caller's arrays, outputs pre-filled: (rows[n, K], counts or the fill)."""
    n, H = rays.shape[0], hit_dtype(a.real)
    hits, cnt = np.full(n * K * H.itemsize, FILL, dtype=np.uint8), np.full(n * 4, FILL, dtype=np.uint8)
    q = capi.MultiHitQuery(ctypes.sizeof(capi.MultiHitQuery), NRT_QUERY_MOTION | NRT_QUERY_MASKED, rays.ctypes.data, n, None, ids.ctypes.data,
                           times.ctypes.data, words.ctypes.data, hits.ctypes.data, cnt.ctypes.data if counts else None, K, 0)
    a._check(getattr(a._L, "nrtMultiHitQueryBatch_" + a._s)(a._h, ctypes.addressof(q)))
    return hits.view(H).reshape(n, K), cnt.view(np.uint32)


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_host_form_equals_the_device_form(oracle, real):
    w = mq.world(oracle, "shells", real)
    a, d = accel_of(w), Dev(w)
    K = 4
    wh, wc = d.query(a, K, True, True, True)
    assert wc.sum() > 1000
    h, c = host_query(a, K, w.rays, w.times, w.words, w.ids)
    assert a.LastKernelName() == kernel_name(real, True, True)
    mq.assert_rows_identical(wh, wc, h, c)
    # counts_out == NULL on both forms: the rows all the same, the counts untouched
    h, c = host_query(a, K, w.rays, w.times, w.words, w.ids, counts=False)
    mq.assert_rows_identical(wh, wc, h, wc)
    assert (c.view(np.uint8) == FILL).all()
    h, c = d.query(a, K, True, True, True, counts=False)
    mq.assert_rows_identical(wh, wc, h, wc)
    assert (c.view(np.uint8) == FILL).all()
    a.close()


def test_host_form_across_a_piece_of_the_staged_rows(oracle):
    """fp64, K = 64: the staged rows of one launch hold cap / (64 * 32) rays; 4099 more make a second piece.  Every per-ray array is the
    shells' tiled: 4099 is prime, so a piece staged with another piece's slice of the times, the words or the ids fails."""
    real, K = np.float64, 64
    w = mq.world(oracle, "shells", real)
    per_piece = mq.staged_rows_cap() // (K * hit_dtype(real).itemsize)
    n = per_piece + qf.SHELL_RAYS
    assert sz.crossing_trips(n, per_piece) == 2 and per_piece % qf.SHELL_RAYS != 0
    a, d = accel_of(w), Dev(w, n)
    wh, wc = d.query(a, K, True, True, True)
    rays, times, words, ids = (np.ascontiguousarray(sz.tiled(x, n)) for x in (w.rays, w.times, w.words, w.ids))
    h, c = host_query(a, K, rays, times, words, ids)
    assert np.array_equal(wc, c) and wc[:qf.SHELL_RAYS].sum() > 1000
    for k in h.dtype.names:
        assert np.array_equal(np.ascontiguousarray(wh[k]).view(np.uint8), np.ascontiguousarray(h[k]).view(np.uint8)), k
    a.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_every_refusal_writes_nothing_and_says_why(oracle, real):
    import torch

    w = mq.world(oracle, "shells", real)
    s, other = ("f32", "f64") if np.dtype(real) == np.float32 else ("f64", "f32")
    L = capi.lib()
    n, K = 64, 4
    H = hit_dtype(real)
    rays, times, words, ids = (np.ascontiguousarray(x[:n]) for x in (w.rays, w.times, w.words, w.ids))
    d = Dev(w)
    size = ctypes.sizeof(capi.MultiHitQuery)
    both = NRT_QUERY_MOTION | NRT_QUERY_MASKED
    names = [k for k, _ in capi.MultiHitQuery._fields_]

    def says_why(a, kw):
        msg = L.nrtLastError(a._h)
        assert msg and b"nrtMultiHitQueryBatch" in msg, (kw, msg)

    def host_case(a, status, fn=None, **kw):
        """One refused host call: the descriptor of an all-three query over n rays with `kw` replacing fields."""
        hits, cnt = np.full(n * 64 * H.itemsize, FILL, dtype=np.uint8), np.full(n * 4, FILL, dtype=np.uint8)
        f = dict(struct_size=size, flags=both, rays=rays.ctypes.data, num_rays=n, options=None, skip_prim_ids=ids.ctypes.data, times=times.ctypes.data,
                 ray_masks=words.ctypes.data, hits_out=hits.ctypes.data, counts_out=cnt.ctypes.data, max_hits=K, reserved=0)
        f.update(kw)
        q = capi.MultiHitQuery(*[f[k] for k in names])
        st = getattr(L, fn or ("nrtMultiHitQueryBatch_" + s))(a._h if a is not None else None, ctypes.addressof(q))
        assert st == status, (kw, st)
        assert (hits == FILL).all() and (cnt == FILL).all(), kw
        if a is not None:
            says_why(a, kw)

    def device_case(a, status, **kw):
        d_h = torch.full((n * 64 * H.itemsize,), FILL, dtype=torch.uint8, device="cuda")
        d_c = torch.full((n * 4,), FILL, dtype=torch.uint8, device="cuda")
        f = dict(struct_size=size, flags=both, rays=d.rays.data_ptr(), num_rays=n, options=None, skip_prim_ids=d.ids.data_ptr(), times=d.times.data_ptr(),
                 ray_masks=d.words.data_ptr(), hits_out=d_h.data_ptr(), counts_out=d_c.data_ptr(), max_hits=K, reserved=0)
        f.update(kw)
        q = capi.MultiHitQuery(*[f[k] for k in names])
        st = getattr(L, "nrtMultiHitQueryBatchDevice_" + s)(a._h, ctypes.addressof(q), None)
        torch.cuda.synchronize()
        assert st == status, (kw, st)
        assert bool((d_h == FILL).all()) and bool((d_c == FILL).all()), kw
        says_why(a, kw)

    a = accel_of(w)
    for case in (host_case, device_case):
        case(a, NRT_ERR_INVALID, struct_size=size - 8)
        case(a, NRT_ERR_INVALID, struct_size=size + 8)
        case(a, NRT_ERR_INVALID, struct_size=ctypes.sizeof(capi.RayQuery))
        case(a, NRT_ERR_INVALID, struct_size=0)
        case(a, NRT_ERR_INVALID, flags=both | 8)
        case(a, NRT_ERR_INVALID, flags=0x80000000)
        case(a, NRT_ERR_INVALID, flags=both | NRT_QUERY_OCCLUSION)
        case(a, NRT_ERR_INVALID, flags=NRT_QUERY_OCCLUSION)
        case(a, NRT_ERR_INVALID, reserved=1)
        case(a, NRT_ERR_INVALID, max_hits=0)
        case(a, NRT_ERR_INVALID, max_hits=65)
        case(a, NRT_ERR_INVALID, rays=None)
        case(a, NRT_ERR_INVALID, hits_out=None)
        case(a, NRT_ERR_INVALID, num_rays=1 << 31)
    # a NULL context and a NULL descriptor
    host_case(None, NRT_ERR_INVALID)
    assert getattr(L, "nrtMultiHitQueryBatch_" + s)(a._h, None) == NRT_ERR_INVALID
    says_why(a, "NULL descriptor")
    assert getattr(L, "nrtMultiHitQueryBatchDevice_" + s)(a._h, None, None) == NRT_ERR_INVALID
    says_why(a, "NULL descriptor, Device")
    assert getattr(L, "nrtMultiHitQueryBatchDevice_" + s)(None, None, None) == NRT_ERR_INVALID
    # the other precision (the context is looked at before any array is read)
    host_case(a, NRT_ERR_PRECISION, fn="nrtMultiHitQueryBatch_" + other)
    # a Device array that is not aligned to its element
    raw = torch.zeros((8 * n + 16,), dtype=torch.uint8, device="cuda")
    odd = raw.data_ptr() + 1
    assert odd % 4 != 0
    device_case(a, NRT_ERR_INVALID, times=odd)
    device_case(a, NRT_ERR_INVALID, ray_masks=odd)
    device_case(a, NRT_ERR_INVALID, skip_prim_ids=odd)
    device_case(a, NRT_ERR_INVALID, counts_out=odd)
    if np.dtype(real) == np.float64:  # (a double at a multiple of 4 that is no multiple of 8)
        assert raw.data_ptr() % 8 == 0
        device_case(a, NRT_ERR_INVALID, times=raw.data_ptr() + 4)
    # num_rays == 0 is fine, whatever else is NULL
    q = capi.MultiHitQuery(size, both, None, 0, None, None, None, None, None, None, K, 0)
    assert getattr(L, "nrtMultiHitQueryBatch_" + s)(a._h, ctypes.addressof(q)) == NRT_OK
    assert getattr(L, "nrtMultiHitQueryBatchDevice_" + s)(a._h, ctypes.addressof(q), None) == NRT_OK
    # ... and the context still answers
    h, c = a.MultiHitQueryBatch(rays, K, times=times, ray_masks=words, skip_prim_ids=ids)
    assert c.sum() > 0
    a.close()
    # MASKED without masks
    a = accel_of(w, masks=False)
    for case in (host_case, device_case):
        case(a, NRT_ERR_INVALID)
        case(a, NRT_ERR_INVALID, flags=NRT_QUERY_MASKED)
    a.close()
    # no tree; MOTION without a keyframe
    a = BVHAccel(real)
    a.SetMesh(TriangleMesh(w.v, w.f))
    a.SetPrimMasks(w.pm)
    for case in (host_case, device_case):  # no tree, whatever the descriptor asks for
        case(a, NRT_ERR_INVALID, flags=NRT_QUERY_MASKED)
        case(a, NRT_ERR_INVALID, flags=0, skip_prim_ids=None)
    a.SetTree(w.nodes, w.idx)
    for case in (host_case, device_case):
        case(a, NRT_ERR_INVALID)
        case(a, NRT_ERR_INVALID, flags=NRT_QUERY_MOTION)
    a.close()
    # a context of another primitive kind: refused whatever the descriptor asks for
    if np.dtype(real) == np.float32:
        c, r = scenes.random_spheres(64)
        a = BVHAccel(np.float32)
        geom = SphereGeometry(c, r)
        assert a.Build(geom.num_faces, geom)
        for case in (host_case, device_case):
            case(a, NRT_ERR_INVALID, flags=0)
            case(a, NRT_ERR_INVALID, flags=0, skip_prim_ids=None)
        assert a.OccludedBatch(scenes.camera_rays(8, 8)).shape[0] == 64
        a.close()


# ---- 7. the masks change between two queries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_set_prim_masks_between_two_masked_queries_with_no_build(oracle, real):
    w = mq.world(oracle, "shells", real)
    a, d = accel_of(w), Dev(w)
    K = 2
    fh, fc = d.query(a, K, True, True, True)
    mq.assert_rows_identical(*mq.expect(oracle, "shells", real, K), fh, fc)
    other = kf.prim_patterns(w.f.shape[0])["mod3"]
    a.SetPrimMasks(other)
    assert a.IsValid()
    eh, ec = mq.expect(oracle, "shells", real, K, prim_masks=other)
    h, c = d.query(a, K, True, True, True)
    mq.assert_rows_identical(eh, ec, h, c)
    assert ec.sum() > 100 and mq.rows_differ(eh, ec, fh, fc).mean() > 0.05  # (the new words matter)
    a.close()


# ---- 8. include/nanort.h with the backend ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header_check(tmp_path_factory):
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "nanort_amd", "lib")
    exe = str(tmp_path_factory.mktemp("multihit_query_check") / "multihit_query_check_hip")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", inc,
                        os.path.join(ROOT, "tests", "cpp", "multihit_query_check.cc"), "-o", exe, "-DNANORT_USE_HIP_BACKEND", "-D__HIP_PLATFORM_AMD__",
                        "-isystem", "/opt/rocm/include", "-L", libdir, "-lnanort_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                        "-lamdhip64"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_header_backend_equals_its_own_host_form(oracle, header_check, tmp_path, real):
    """GPU Build() over MotionTriangleMesh, SetPrimMasks(); BVHAccel::MultiHitTraverseBatchQuery(q) for the eight combinations of
    MOTION, MASKED and per-ray ids at K = 4 against the header's host form over the read-back tree, byte for byte, inside
    tests/cpp/multihit_query_check.cc."""
    w = mq.world(oracle, "shells", real)
    mesh, rp = (os.path.join(str(tmp_path), x) for x in ("mesh.bin", "rays.bin"))
    with open(mesh, "wb") as fp:
        fp.write(np.array([w.v.shape[0], w.f.shape[0]], dtype=np.uint32).tobytes() + w.v.tobytes() + w.v1.tobytes() + w.f.tobytes() + w.pm.tobytes())
    with open(rp, "wb") as fp:
        fp.write(np.array([w.rays.shape[0]], dtype=np.uint64).tobytes() + w.rays.tobytes() + w.times.tobytes() + w.words.tobytes() + w.ids.tobytes())
    r = subprocess.run([header_check, "f32" if real == np.float32 else "f64", mesh, "-", rp, "-", "4", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    word, held, n = r.stdout.split()[-3:]
    assert word == "ok" and int(n) == w.rays.shape[0] and int(held) > 8000


# ---- 9. the plain kernel after the K-buffer was factored ------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_plain_multihit_still_gives_the_model(oracle, real):
    w = mq.world(oracle, "shells", real)
    a, d = accel_of(w), Dev(w)
    h, c = d.plain(a, 4)
    assert a.LastKernelName() == plain_name(real)
    eh, ec = mhf.model(w.nodes, w.idx, w.v, w.f, w.rays, 4)
    mq.assert_rows_identical(eh, ec, h, c)
    assert ec.sum() > 1000
    a.close()

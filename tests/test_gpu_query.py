"""The combined ray query on the GPU (include/nanort_hip.h, "one descriptor for every triangle ray query"; DESIGN.md 3.13;
nanort_amd/csrc/own_walks.hip): per-ray skip ids, visibility words and motion times on the same ray.

  1. shells: the four composite combinations through the Device form, closest hit and occlusion, one arm with trace options;
  2. pile: all three past the walk's 32 LDS stack entries;
  3. routing: a descriptor an existing call can express is that call — its kernel, its bytes;
  4. the host form against the Device form: staged in one piece, staged in two, pipelined from page-locked arrays in three;
  5. every refusal: status, a message, outputs untouched;
  6. the prim masks changed between two composite queries with no build;
  7. include/nanort.h with the backend: BVHAccel::TraverseBatchQuery(q) against the header's own host form.

1 and 2 are exact against the expectation of tests/query_fixture.py over the context's own node array: every field of every record,
no tolerance.  3 to 7 compare with calls that 1 and 2 (and the older files) tie to the oracle.  The fixture conditions — every
feature matters on the same ray, the pile's walk is deeper than the LDS stack — hold for the reference alone;
tests/test_query_model.py asserts them without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import masks_fixture as kf
import motion_fixture as mf
import own_walks_fixture as ow
import query_fixture as qf
import size_thresholds as sz
from helpers import assert_hits_identical, trace_options
from nanort_amd import BVHAccel, MotionTriangleMesh, SphereGeometry, TriangleMesh, capi, scenes
from nanort_amd.capi import NRT_ERR_INVALID, NRT_ERR_PRECISION, NRT_OK, NRT_QUERY_MASKED, NRT_QUERY_MOTION, NRT_QUERY_OCCLUSION
from nanort_amd.wire import hit_dtype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REALS = [np.float32, np.float64]
IDS = ["f32", "f64"]
FILL = 0xA5  # every output byte before a call: no record and no flag holds it
COMBOS = {"motion+ids": (True, False, True), "masked+ids": (False, True, True), "motion+masked": (True, True, False), "all": (True, True, True)}


def _c(real):
    return "float" if np.dtype(real) == np.float32 else "double"


@pytest.fixture(scope="module")
def worlds(oracle):
    """{(name, precision): World}, each built on first use and kept for the file."""
    cache = {}

    def get(name, real):
        key = (name, np.dtype(real).name)
        if key not in cache:
            cache[key] = (qf.shells if name == "shells" else qf.pile)(oracle, real)
        return cache[key]

    return get


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

    def outputs(self):
        t = self.torch
        return (t.full((self.n * self.hit_t.itemsize,), FILL, dtype=t.uint8, device="cuda"), t.full((self.n,), FILL, dtype=t.uint8, device="cuda"))

    def query(self, a, motion, masked, ids, occlusion=False, opts=None, times=None, words=None, skip=None):
        """The Device form; (records or None, flags) on the host."""
        d_h, d_m = self.outputs()
        a.QueryBatchDevice(self.rays, None if occlusion else d_h, d_m, times=(self.times if times is None else times) if motion else None,
                           ray_masks=(self.words if words is None else words) if masked else None,
                           skip_prim_ids=(self.ids if skip is None else skip) if ids else None, motion=motion, masked=masked, occlusion=occlusion,
                           options=opts)
        self.torch.cuda.synchronize()
        if occlusion:
            assert bytes(d_h.cpu().numpy()) == bytes([FILL]) * d_h.numel(), "an occlusion query wrote records"
        return (None if occlusion else self.records(d_h)), d_m.cpu().numpy()

    def records(self, d_h):
        return np.frombuffer(d_h.cpu().numpy().tobytes(), dtype=self.hit_t)


def check_combo(oracle, a, w, d, combo, opts=None, min_hits=100):
    motion, masked, ids = COMBOS[combo]
    eh, em = w.expected(oracle, motion=motion, masked=masked, ids=ids, opts=opts)
    assert em.sum() > min_hits, (combo, em.sum())
    h, m = d.query(a, motion, masked, ids, opts=opts)
    assert a.LastKernelName().startswith("nrt::k_traverse_query<%s, " % _c(w.real)), a.LastKernelName()
    assert_hits_identical(eh, em, h, m)
    _, occ = d.query(a, motion, masked, ids, occlusion=True, opts=opts)
    assert a.LastKernelName().startswith("nrt::k_traverse_query<%s, " % _c(w.real)), a.LastKernelName()
    assert np.array_equal(occ, em)
    return a.LastKernelName()


# ---- 1. shells ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", sorted(COMBOS))
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_shells_every_composite_combination(oracle, worlds, real, combo):
    w = worlds("shells", real)
    a, d = accel_of(w), Dev(w)
    name = check_combo(oracle, a, w, d, combo)
    motion, masked, _ = COMBOS[combo]
    assert name == "nrt::k_traverse_query<%s, 32, %s, %s>" % (_c(real), str(motion).lower(), str(masked).lower())
    a.close()


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_shells_all_three_under_trace_options(oracle, worlds, real):
    """An id range and back-face culling on top of the three per-ray things; the skip id stays per ray.  The first options are the
    ones asked for: a range inside the innermost shell, culled — next to nothing is left (tests/test_query_model.py), exact all the
    same; the second keep most of the shells."""
    w = worlds("shells", real)
    a, d = accel_of(w), Dev(w)
    check_combo(oracle, a, w, d, "all", opts=qf.shell_options(), min_hits=0)
    check_combo(oracle, a, w, d, "all", opts=trace_options(range_=(50, 3900), skip=412))
    a.close()


# ---- 2. pile ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_pile_all_three_past_the_lds_stack(oracle, worlds, real):
    """The reference's tree over the pile is 138 deep and the walk holds 137 entries: 105 past the LDS entries, in the slot's spill array."""
    w = worlds("pile", real)
    assert w.stats["max_tree_depth"] > ow.PILE_MIN_STACK
    a, d = accel_of(w), Dev(w)
    check_combo(oracle, a, w, d, "all")
    a.close()


# ---- 3. routing ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_a_descriptor_an_existing_call_can_express_is_that_call(worlds, real):
    w = worlds("shells", real)
    a, d = accel_of(w), Dev(w)
    torch = d.torch

    def old(call, occlusion):
        d_h, d_m = d.outputs()
        call(d_h, d_m)
        torch.cuda.synchronize()
        return (None if occlusion else d.records(d_h)), d_m.cpu().numpy(), a.LastKernelName()

    def same(want, motion, masked, ids, occlusion, kernel=None):
        wh, wm, wk = want
        h, m = d.query(a, motion, masked, ids, occlusion=occlusion)
        assert a.LastKernelName() == wk and (kernel is None or wk == kernel), (a.LastKernelName(), wk, kernel)
        assert m.tobytes() == wm.tobytes() and wm.any()
        if not occlusion:
            assert_hits_identical(wh, wm, h, m)

    c = _c(real)
    same(old(lambda h, m: a.TraverseBatchDevice(d.rays, h, m), False), False, False, False, False)
    same(old(lambda h, m: a.OccludedBatchDevice(d.rays, m), True), False, False, False, True)
    same(old(lambda h, m: a.TraverseBatchDevice(d.rays, h, m, skip_prim_ids=d.ids), False), False, False, True, False)
    same(old(lambda h, m: a.OccludedBatchDevice(d.rays, m, skip_prim_ids=d.ids), True), False, False, True, True)
    same(old(lambda h, m: a.TraverseBatchMotionDevice(d.rays, d.times, h, m), False), True, False, False, False, "nrt::k_traverse_motion<%s>" % c)
    same(old(lambda h, m: a.OccludedBatchMotionDevice(d.rays, d.times, m), True), True, False, False, True, "nrt::k_traverse_motion<%s>" % c)
    same(old(lambda h, m: a.TraverseBatchMaskedDevice(d.rays, d.words, h, m), False), False, True, False, False, "nrt::k_traverse_masked<%s>" % c)
    same(old(lambda h, m: a.OccludedBatchMaskedDevice(d.rays, d.words, m), True), False, True, False, True, "nrt::k_traverse_masked<%s>" % c)
    # the host forms route the same way
    for call, kw in ((lambda: a.TraverseBatch(w.rays), dict()), (lambda: a.TraverseBatch(w.rays, skip_prim_ids=w.ids), dict(skip_prim_ids=w.ids)),
                     (lambda: a.TraverseBatchMotion(w.rays, w.times), dict(times=w.times)),
                     (lambda: a.TraverseBatchMasked(w.rays, w.words), dict(ray_masks=w.words))):
        want = call()
        kernel = a.LastKernelName()
        h, m = a.QueryBatch(w.rays, **kw)
        assert a.LastKernelName() == kernel
        assert_hits_identical(want[0], want[1], h, m)
    # the composite kernel with nothing to apply: all-ones words on both sides, time 0 everywhere, no id -> the plain records over keyframe 0
    plain = old(lambda h, m: a.TraverseBatchDevice(d.rays, h, m), False)
    a.SetPrimMasks(np.full(w.f.shape[0], 0xFFFFFFFF, dtype=np.uint32))
    n = d.n
    zeros = torch.zeros((n,), dtype=d.times.dtype, device="cuda")
    ones = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    h, m = d.query(a, True, True, True, times=zeros, words=ones, skip=ones)
    assert a.LastKernelName() == "nrt::k_traverse_query<%s, 32, true, true>" % c
    assert_hits_identical(plain[0], plain[1], h, m)
    assert m.sum() > 100
    a.close()


# ---- 4. the host form ---------------------------------------------------------------------------------------------------------------
class HostAlloc:
    """Page-locked host arrays from nrtHostAlloc, as numpy views; freed by close()."""

    def __init__(self):
        self.L, self.ptrs = capi.lib(), []

    def array(self, src):
        src = np.ascontiguousarray(src)
        p = ctypes.c_void_p()
        assert self.L.nrtHostAlloc(max(1, src.nbytes), ctypes.byref(p)) == NRT_OK and p.value
        self.ptrs.append(p)
        out = np.frombuffer((ctypes.c_char * src.nbytes).from_address(p.value), dtype=src.dtype)
        out[:] = src
        return out

    def close(self):
        for p in self.ptrs:
            self.L.nrtHostFree(p)
        self.ptrs = []


@pytest.mark.parametrize("pieces", [1, 2, 3])
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_host_form_equals_the_device_form(worlds, real, pieces):
    """4099 rays (one staged piece), kPiece + 4099 from pageable arrays (two staged pieces), 2 kPiece + 4099 from nrtHostAlloc'd
    arrays (the three-stream pipeline: three pieces over two staging slots).  Every per-ray array is the shells' tiled: 4099 is
    prime and kPiece mod 4099 = 3715, so a piece staged with another piece's slice of the times, the words or the ids fails."""
    w = worlds("shells", real)
    assert sz.source_cap("kPiece") == sz.PIECE and sz.PIECE % qf.SHELL_RAYS != 0
    n = (pieces - 1) * sz.PIECE + qf.SHELL_RAYS
    assert sz.crossing_trips(n, sz.PIECE) == pieces
    a, d = accel_of(w), Dev(w, n)
    wh, wm = d.query(a, True, True, True)
    _, wocc = d.query(a, True, True, True, occlusion=True)
    assert wm[:qf.SHELL_RAYS].sum() > 100 and np.array_equal(wocc, wm)
    rays, times, words, ids = (sz.tiled(x, n) for x in (w.rays, w.times, w.words, w.ids))
    H = hit_dtype(real)
    pool = HostAlloc()
    try:
        if pieces == 3:
            rays, times, words, ids = (pool.array(x) for x in (rays, times, words, ids))
            hits, mask = pool.array(np.full(n * H.itemsize, FILL, dtype=np.uint8)), pool.array(np.full(n, FILL, dtype=np.uint8))
        else:
            rays, times, words, ids = (np.ascontiguousarray(x) for x in (rays, times, words, ids))
            hits, mask = np.full(n * H.itemsize, FILL, dtype=np.uint8), np.full(n, FILL, dtype=np.uint8)
        q = capi.RayQuery(ctypes.sizeof(capi.RayQuery), NRT_QUERY_MOTION | NRT_QUERY_MASKED, rays.ctypes.data, n, None, ids.ctypes.data,
                          times.ctypes.data, words.ctypes.data, hits.ctypes.data, mask.ctypes.data)
        a._check(getattr(a._L, "nrtQueryBatch_" + a._s)(a._h, ctypes.addressof(q)))
        assert a.LastKernelName() == "nrt::k_traverse_query<%s, 32, true, true>" % _c(real)
        assert_hits_identical(wh, wm, hits.view(H), mask)
        if pieces < 3:  # (the occlusion form has the staged path alone)
            assert np.array_equal(a.QueryBatch(rays, times=times, ray_masks=words, skip_prim_ids=ids, occlusion=True), wm)
    finally:
        a.close()
        pool.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_every_refusal_writes_nothing_and_says_why(worlds, real):
    import torch

    w = worlds("shells", real)
    s, other = ("f32", "f64") if np.dtype(real) == np.float32 else ("f64", "f32")
    L = capi.lib()
    n = 64
    H = hit_dtype(real)
    rays, times, words, ids = (np.ascontiguousarray(x[:n]) for x in (w.rays, w.times, w.words, w.ids))
    d = Dev(w)
    size = ctypes.sizeof(capi.RayQuery)
    both = NRT_QUERY_MOTION | NRT_QUERY_MASKED

    def host_case(a, status, fn=None, **kw):
        """One refused host call: the descriptor of an all-three query over n rays with `kw` replacing fields."""
        hits, mask = np.full(n * H.itemsize, FILL, dtype=np.uint8), np.full(n, FILL, dtype=np.uint8)
        f = dict(struct_size=size, flags=both, rays=rays.ctypes.data, num_rays=n, options=None, skip_prim_ids=ids.ctypes.data,
                 times=times.ctypes.data, ray_masks=words.ctypes.data, hits_out=hits.ctypes.data, mask_out=mask.ctypes.data)
        f.update(kw)
        q = capi.RayQuery(*[f[k] for k, _ in capi.RayQuery._fields_])
        st = getattr(L, fn or ("nrtQueryBatch_" + s))(a._h if a is not None else None, ctypes.addressof(q))
        assert st == status, (kw, st)
        assert (hits == FILL).all() and (mask == FILL).all(), kw
        if a is not None:
            assert L.nrtLastError(a._h), kw

    def device_case(a, status, **kw):
        d_h, d_m = d.outputs()
        f = dict(struct_size=size, flags=both, rays=d.rays.data_ptr(), num_rays=n, options=None, skip_prim_ids=d.ids.data_ptr(),
                 times=d.times.data_ptr(), ray_masks=d.words.data_ptr(), hits_out=d_h.data_ptr(), mask_out=d_m.data_ptr())
        f.update(kw)
        q = capi.RayQuery(*[f[k] for k, _ in capi.RayQuery._fields_])
        st = getattr(L, "nrtQueryBatchDevice_" + s)(a._h, ctypes.addressof(q), None)
        torch.cuda.synchronize()
        assert st == status, (kw, st)
        assert bool((d_h == FILL).all()) and bool((d_m == FILL).all()), kw
        assert L.nrtLastError(a._h), kw

    a = accel_of(w)
    for case in (host_case, device_case):
        case(a, NRT_ERR_INVALID, struct_size=size - 8)
        case(a, NRT_ERR_INVALID, struct_size=size + 8)
        case(a, NRT_ERR_INVALID, struct_size=0)
        case(a, NRT_ERR_INVALID, flags=both | 8)
        case(a, NRT_ERR_INVALID, flags=0x80000000)
        case(a, NRT_ERR_INVALID, rays=None)
        case(a, NRT_ERR_INVALID, hits_out=None)
        case(a, NRT_ERR_INVALID, flags=both | NRT_QUERY_OCCLUSION, mask_out=None)
        case(a, NRT_ERR_INVALID, num_rays=1 << 31)
    # a NULL context and a NULL descriptor
    host_case(None, NRT_ERR_INVALID)
    assert getattr(L, "nrtQueryBatch_" + s)(a._h, None) == NRT_ERR_INVALID and L.nrtLastError(a._h)
    assert getattr(L, "nrtQueryBatchDevice_" + s)(a._h, None, None) == NRT_ERR_INVALID and L.nrtLastError(a._h)
    assert getattr(L, "nrtQueryBatchDevice_" + s)(None, None, None) == NRT_ERR_INVALID
    # the other precision (arrays of twice the rays: the wider entry point stages twice the bytes before the context is looked at)
    rays2, times2 = np.ascontiguousarray(w.rays[:2 * n]), np.ascontiguousarray(w.times[:2 * n])
    host_case(a, NRT_ERR_PRECISION, fn="nrtQueryBatch_" + other, rays=rays2.ctypes.data, times=times2.ctypes.data)
    # a Device array that is not aligned to its element size
    raw = torch.zeros((8 * n + 16,), dtype=torch.uint8, device="cuda")
    odd = raw.data_ptr() + 1
    assert odd % 4 != 0
    device_case(a, NRT_ERR_INVALID, times=odd)
    device_case(a, NRT_ERR_INVALID, ray_masks=odd)
    device_case(a, NRT_ERR_INVALID, skip_prim_ids=odd)
    if np.dtype(real) == np.float64:  # (a double at a multiple of 4 that is no multiple of 8)
        assert raw.data_ptr() % 8 == 0
        device_case(a, NRT_ERR_INVALID, times=raw.data_ptr() + 4)
    # num_rays == 0 is fine, whatever else is NULL
    hits, mask = np.full(n * H.itemsize, FILL, dtype=np.uint8), np.full(n, FILL, dtype=np.uint8)
    q = capi.RayQuery(size, both, None, 0, None, None, None, None, None, None)
    assert getattr(L, "nrtQueryBatch_" + s)(a._h, ctypes.addressof(q)) == NRT_OK
    assert getattr(L, "nrtQueryBatchDevice_" + s)(a._h, ctypes.addressof(q), None) == NRT_OK
    # ... and the context still answers
    h, m = a.QueryBatch(rays, times=times, ray_masks=words, skip_prim_ids=ids)
    assert m.sum() > 0
    a.close()
    # MASKED without masks
    a = accel_of(w, masks=False)
    for case in (host_case, device_case):
        case(a, NRT_ERR_INVALID)
        case(a, NRT_ERR_INVALID, flags=NRT_QUERY_MASKED)
    a.close()
    # MOTION without a keyframe
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
            case(a, NRT_ERR_INVALID)
            case(a, NRT_ERR_INVALID, flags=0, skip_prim_ids=None)
            case(a, NRT_ERR_INVALID, flags=NRT_QUERY_OCCLUSION, skip_prim_ids=None)
        assert a.OccludedBatch(scenes.camera_rays(8, 8)).shape[0] == 64
        a.close()


# ---- 6. the masks change under a motion context ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_set_prim_masks_between_two_composite_queries_with_no_build(oracle, worlds, real):
    w = worlds("shells", real)
    a, d = accel_of(w), Dev(w)
    first = d.query(a, True, True, True)
    assert_hits_identical(*w.expected(oracle), *first)
    other = kf.prim_patterns(w.f.shape[0])["mod3"]
    a.SetPrimMasks(other)
    assert a.IsValid()
    eh, em = qf.expected(oracle, w.nodes, w.idx, w.v, w.v1, w.f, other, w.rays, w.times, w.words, w.ids, motion=True, masked=True)
    h, m = d.query(a, True, True, True)
    assert_hits_identical(eh, em, h, m)
    assert em.sum() > 100 and mf.differs(eh, em, *first).mean() > 0.05  # (the new words matter)
    a.close()


# ---- 7. include/nanort.h with the backend ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header_check(tmp_path_factory):
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "nanort_amd", "lib")
    exe = str(tmp_path_factory.mktemp("query_backend_check") / "query_backend_check")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", inc,
                        os.path.join(ROOT, "tests", "cpp", "query_backend_check.cc"), "-o", exe, "-DNANORT_USE_HIP_BACKEND", "-D__HIP_PLATFORM_AMD__",
                        "-isystem", "/opt/rocm/include", "-L", libdir, "-lnanort_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
                        "-lamdhip64"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


@pytest.mark.parametrize("opt", ["default", "options"])
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_header_backend_equals_its_own_host_form(header_check, tmp_path, worlds, real, opt):
    """GPU Build() over MotionTriangleMesh, SetPrimMasks(); BVHAccel::TraverseBatchQuery(q) for the eight combinations of MOTION,
    MASKED and per-ray ids, closest hit and occlusion, against the header's host form over the read-back tree, byte for byte, inside
    tests/cpp/query_backend_check.cc."""
    w = worlds("shells", real)
    mesh, rp = (os.path.join(str(tmp_path), x) for x in ("mesh.bin", "rays.bin"))
    with open(mesh, "wb") as fp:
        fp.write(np.array([w.v.shape[0], w.f.shape[0]], dtype=np.uint32).tobytes() + w.v.tobytes() + w.v1.tobytes() + w.f.tobytes() + w.pm.tobytes())
    with open(rp, "wb") as fp:
        fp.write(np.array([w.rays.shape[0]], dtype=np.uint64).tobytes() + w.rays.tobytes() + w.times.tobytes() + w.words.tobytes() + w.ids.tobytes())
    # (no culling here: from a point between the shells it leaves next to nothing — the culled arm is test 1's)
    o = trace_options(range_=(50, 3900), skip=412) if opt == "options" else trace_options()
    o = o[()] if o.shape == () else o[0]
    r = subprocess.run([header_check, "f32" if real == np.float32 else "f64", mesh, rp, str(int(o["prim_ids_range"][0])), str(int(o["prim_ids_range"][1])),
                        str(int(o["skip_prim_id"])), str(int(o["cull_back_face"]))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    word, hits, n = r.stdout.split()[-3:]
    assert word == "ok" and int(n) == w.rays.shape[0] and int(hits) > 1000

"""How a ray query enters the library (nanort_amd/csrc/api_query.hip: query_host, query_device): every ray-query entry point of the C
ABI, called through capi.lib() directly, makes the same first refusals in the same order with the same words, and its valid call
returns the bytes the BVHAccel method for that query returns.  Nothing here launches a kernel that can be refused: the refusals are
all made on the host before anything is enqueued.  Also: every Device method of BVHAccel takes None, a raw handle or a
torch.cuda.Stream as its stream."""
import ctypes

import numpy as np
import pytest

from nanort_amd import BVHAccel, capi
from nanort_amd.accel import CurveGeometry, CylinderGeometry, MotionTriangleMesh, SphereGeometry
from nanort_amd.wire import CURVE_HIT_F32, CYL_HIT_F32, hit_dtype, ray_dtype, suffix

pytestmark = pytest.mark.gpu

N = 8  # rays: the even ones come down on the two primitives (at x = 0 and x = 5), the odd ones pass between and beside them
K = 2  # max_hits of the multi-hit entry points
SKIP_IDS = np.array([0, 0xFFFFFFFF] * (N // 2), dtype=np.uint32)  # (rays 0 and 4 come down on primitive 0 and skip it)

# One row per entry point pair (host form, Device form = name + "Device"):
#   name, precisions, context, what lies between the rays and the outputs, the outputs, and the message the required output's
#   absence draws from the host form and from the Device form — written down from the sources before the entry points shared
#   query_host / query_device.  The skip and motion host forms speak as the entry point they extend, and both multi-hit forms
#   as nrtMultiHitTraverseBatch.
ENTRIES = [
    ("nrtTraverseBatch", ("f32", "f64"), "triangles", "", "hits+mask", "nrtTraverseBatch: NULL rays/hits", "nrtTraverseBatchDevice: NULL hits"),
    ("nrtTraverseBatchSkip", ("f32", "f64"), "triangles", "ids", "hits+mask", "nrtTraverseBatch: NULL rays/hits", "nrtTraverseBatchSkipDevice: NULL hits"),
    ("nrtOccludedBatch", ("f32", "f64"), "triangles", "", "mask", "nrtOccludedBatch: NULL rays/mask", "nrtOccludedBatchDevice: NULL mask"),
    ("nrtOccludedBatchSkip", ("f32", "f64"), "triangles", "ids", "mask", "nrtOccludedBatch: NULL rays/mask", "nrtOccludedBatchSkipDevice: NULL mask"),
    ("nrtOccludedBatchPrims", ("f32",), "spheres", "", "mask", "nrtOccludedBatchPrims: NULL rays/mask", "nrtOccludedBatchPrimsDevice: NULL mask"),
    ("nrtTraverseBatchCylinders", ("f32",), "cylinders", "", "hits+mask", "nrtTraverseBatchCylinders: NULL rays/hits", "nrtTraverseBatchCylindersDevice: NULL hits"),
    ("nrtTraverseBatchCurves", ("f32",), "curves", "", "hits+mask", "nrtTraverseBatchCurves: NULL rays/hits", "nrtTraverseBatchCurvesDevice: NULL hits"),
    ("nrtMultiHitTraverseBatch", ("f32", "f64"), "triangles", "k", "hits+counts", "nrtMultiHitTraverseBatch: NULL rays/hits", "nrtMultiHitTraverseBatch: NULL rays/hits"),
    ("nrtTraverseBatchMotion", ("f32", "f64"), "triangles", "times", "hits+mask", "nrtTraverseBatch: NULL rays/hits", "nrtTraverseBatchMotionDevice: NULL hits"),
    ("nrtOccludedBatchMotion", ("f32", "f64"), "triangles", "times", "mask", "nrtOccludedBatch: NULL rays/mask", "nrtOccludedBatchMotionDevice: NULL mask"),
]
CASES = [pytest.param(e, s, dev, id="%s%s_%s" % (e[0], "Device" if dev else "", s)) for e in ENTRIES for s in e[1] for dev in (False, True)]


def make_rays(real):
    rays = np.zeros(N, dtype=ray_dtype(real))
    x = np.array([0.0, 2.5, 5.0, 7.5, 0.125, 2.25, 5.125, -3.0])
    rays["org"] = np.stack([x, np.full(N, 0.0625), np.full(N, 5.0)], axis=1)
    rays["dir"] = (0.0, 0.0, -1.0)
    rays["max_t"] = 100.0
    return rays


class Contexts:
    """The four contexts of the module (and the fp64 twin of the triangle one), built once and only read afterwards."""

    def __init__(self):
        v0 = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0], [4, -1, 0], [6, -1, 0], [5, 1, 0]], dtype=np.float64)
        faces = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.uint32)
        self.accel = {}
        for real in (np.float32, np.float64):
            a = BVHAccel(real)
            assert a.Build(2, MotionTriangleMesh(v0.astype(real), (v0 + (0.25, 0, 0.5)).astype(real), faces))
            self.accel["triangles", suffix(real)] = a
        two = np.array([[0, 0, 0], [5, 0, 0]], dtype=np.float32)
        ends = np.stack([two - (0, 1, 0), two + (0, 1, 0)], axis=1).astype(np.float32)
        cps = np.stack([two + (0, y, 0) for y in (-1.0, -0.25, 0.25, 1.0)], axis=1).astype(np.float32)
        for kind, geom in (("spheres", SphereGeometry(two, np.full(2, 0.5, np.float32))), ("cylinders", CylinderGeometry(ends, np.full((2, 2), 0.5, np.float32))),
                           ("curves", CurveGeometry(cps, np.full((2, 4), 0.5, np.float32)))):
            a = BVHAccel(np.float32)
            assert a.Build(2, geom)
            self.accel[kind, "f32"] = a
        self.times = {s: np.linspace(0.0, 1.0, N).astype(np.float32 if s == "f32" else np.float64) for s in ("f32", "f64")}


@pytest.fixture(scope="module")
def ctxs():
    return Contexts()


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Call:
    """One entry point with one set of arrays: host arrays, or their device copies and torch's current stream."""

    def __init__(self, entry, sfx, dev, ctxs):
        import torch

        self.torch = torch
        self.name, _, self.kind, self.between, self.outputs, msg_host, msg_dev = entry
        self.sfx, self.dev, self.message = sfx, dev, (msg_dev if dev else msg_host)
        self.accel = ctxs.accel[self.kind, sfx]
        self.other = ctxs.accel["triangles", "f64" if sfx == "f32" else "f32"]  # a built context of the other precision
        self.fn = getattr(capi.lib(), self.name + ("Device" if dev else "") + "_" + sfx)
        real = np.float32 if sfx == "f32" else np.float64
        rec = CYL_HIT_F32 if self.kind == "cylinders" else CURVE_HIT_F32 if self.kind == "curves" else hit_dtype(real)
        self.rays, self.times = make_rays(real), ctxs.times[sfx]
        self.records = np.zeros(N * (K if self.between == "k" else 1), dtype=rec) if self.outputs != "mask" else None
        self.flags = np.zeros(N, dtype=np.uint32 if self.outputs == "hits+counts" else np.uint8)
        self.required = "flags" if self.outputs == "mask" else "records"
        if dev:
            self.d = {k: None if a is None else torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
                      for k, a in (("rays", self.rays), ("times", self.times), ("ids", SKIP_IDS), ("records", self.records), ("flags", self.flags))}

    def ptr(self, what):
        if self.dev:
            return None if self.d[what] is None else self.d[what].data_ptr()
        return _vp({"rays": self.rays, "times": self.times, "ids": SKIP_IDS, "records": self.records, "flags": self.flags}[what])

    def __call__(self, handle, n, null=()):
        p = lambda what: None if what in null else self.ptr(what)  # noqa: E731
        args = [handle, p("rays")] + ([p("times")] if self.between == "times" else []) + [n] + ([K] if self.between == "k" else []) + [None]
        args += ([p("ids")] if self.between == "ids" else []) + ([p("records")] if self.outputs != "mask" else []) + [p("flags")]
        if self.dev:
            args.append(self.torch.cuda.current_stream().cuda_stream)
        return self.fn(*args)

    def results(self):
        """(record bytes or None, flag bytes) the last valid call left."""
        if self.dev:
            self.torch.cuda.synchronize()
            return (None if self.records is None else self.d["records"].cpu().numpy().tobytes()), self.d["flags"].cpu().numpy().tobytes()
        return (None if self.records is None else self.records.tobytes()), self.flags.tobytes()

    def through_accel(self):
        """The same query through the BVHAccel method for it: (record bytes or None, flag bytes)."""
        a, torch = self.accel, self.torch
        ids = SKIP_IDS if self.between == "ids" else None
        if not self.dev:
            if self.name.startswith("nrtOccludedBatchMotion"):
                return None, a.OccludedBatchMotion(self.rays, self.times).tobytes()
            if self.name.startswith("nrtOccludedBatch"):
                return None, a.OccludedBatch(self.rays, None, ids).tobytes()
            h, m = (a.TraverseBatchMotion(self.rays, self.times) if self.between == "times" else
                    a.MultiHitTraverseBatch(self.rays, K) if self.between == "k" else a.TraverseBatch(self.rays, None, ids))
            return h.tobytes(), m.tobytes()
        d_rec = None if self.records is None else torch.zeros_like(self.d["records"])
        d_flags = torch.zeros_like(self.d["flags"])
        d_ids = self.d["ids"] if ids is not None else None
        if self.name.startswith("nrtOccludedBatchMotion"):
            a.OccludedBatchMotionDevice(self.d["rays"], self.d["times"], d_flags)
        elif self.name.startswith("nrtOccludedBatch"):
            a.OccludedBatchDevice(self.d["rays"], d_flags, skip_prim_ids=d_ids)
        elif self.between == "times":
            a.TraverseBatchMotionDevice(self.d["rays"], self.d["times"], d_rec, d_flags)
        elif self.between == "k":
            a.MultiHitTraverseBatchDevice(self.d["rays"], K, d_rec, d_flags)
        else:
            a.TraverseBatchDevice(self.d["rays"], d_rec, d_flags, skip_prim_ids=d_ids)
        torch.cuda.synchronize()
        return (None if d_rec is None else d_rec.cpu().numpy().tobytes()), d_flags.cpu().numpy().tobytes()


@pytest.mark.parametrize("entry,sfx,dev", CASES)
def test_entry_checks_and_result(ctxs, entry, sfx, dev):
    L = capi.lib()
    call = Call(entry, sfx, dev, ctxs)
    h = call.accel._h
    # (a) no context
    assert call(None, N) == capi.NRT_ERR_INVALID
    # (c) rays, but not the output the query is for: refused on the host, in the parent's words, nothing written
    assert call(h, N, null=(call.required,)) == capi.NRT_ERR_INVALID
    assert L.nrtLastError(h).decode() == call.message
    # (b) no rays: fine without any array, and no word about it
    assert call(h, 0, null=("rays", "times", "ids", "records", "flags")) == capi.NRT_OK
    assert L.nrtLastError(h).decode() == call.message
    # (d) a context of the other precision
    assert call(call.other._h, N) == capi.NRT_ERR_PRECISION
    assert "precision mismatch" in L.nrtLastError(call.other._h).decode()
    got_before = call.results()
    assert got_before[1] == bytes(len(got_before[1])) and (got_before[0] is None or got_before[0] == bytes(len(got_before[0])))  # (nothing written so far)
    # (e) the valid call: the bytes of the BVHAccel method
    assert call(h, N) == capi.NRT_OK
    got, want = call.results(), call.through_accel()
    assert got[1] == want[1]
    if call.records is not None:  # (field by field: nrt_hit_f64 ends in four bytes of padding, which no walk writes)
        g, w = (np.frombuffer(b, dtype=call.records.dtype) for b in (got[0], want[0]))
        assert all(g[f].tobytes() == w[f].tobytes() for f in call.records.dtype.names)
    flags = np.frombuffer(want[1], dtype=call.flags.dtype)
    hit = (flags != 0).reshape(N)
    if "Skip" in call.name:  # (rays 0 and 4 skip the triangle they come down on)
        assert hit.tolist() == [False, False, True, False, False, False, True, False]
    else:
        assert hit.tolist() == [True, False] * (N // 2)


def test_device_methods_take_none_a_raw_handle_or_a_torch_stream(ctxs):
    import torch

    a = ctxs.accel["triangles", "f32"]
    rays = make_rays(np.float32)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    hsz = hit_dtype(np.float32).itemsize
    methods = {
        "TraverseBatchDevice": (lambda out, fl, s: a.TraverseBatchDevice(d_rays, out, fl, stream=s), N * hsz, N),
        "OccludedBatchDevice": (lambda out, fl, s: a.OccludedBatchDevice(d_rays, fl, stream=s), 0, N),
        "MultiHitTraverseBatchDevice": (lambda out, fl, s: a.MultiHitTraverseBatchDevice(d_rays, K, out, fl, stream=s), N * K * hsz, 4 * N),
    }
    for name, (run, out_bytes, flag_bytes) in methods.items():
        seen = []
        for stream in (None, side.cuda_stream, side):
            out = torch.zeros(max(out_bytes, 1), dtype=torch.uint8, device="cuda")
            fl = torch.zeros(flag_bytes, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert run(out, fl, stream) == N
            torch.cuda.synchronize()
            seen.append((out.cpu().numpy().tobytes(), fl.cpu().numpy().tobytes()))
        assert seen[0] == seen[1] == seen[2], name
        assert any(seen[0][1]), name  # (rays hit: the flags, or counts, are not all zero)

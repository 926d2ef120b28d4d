"""Sphere and curve refit on the GPU (nanort_amd/csrc/refit.hip, include/nanort_hip.h nrtRefitPrims_f32 / nrtRefitPrimsDevice_f32):
the refit tree keeps every topology byte and the index array, its boxes equal the numpy model (tests/refit_prims_model.py) on the
moved primitives, and the closest-hit records on it are those of the CPU restatement of the kind's walk over the refit node array
and the new arrays; occlusion flags equal the closest-hit flags.  Also: a refit with the arrays of the build, a build after a
refit, an adopted tree with an empty leaf and an unreachable record, the Device form on side streams, the refusals, and
BVHAccel::RefitGeometry of include/nanort.h (tests/cpp/refit_prims_check.cc)."""
import os
import subprocess

import numpy as np
import pytest

import curves_fixture as cf
import sphere_fixture
from nanort_amd import BVHAccel, CurveGeometry, CylinderGeometry, SphereGeometry, TriangleMesh, scenes
from nanort_amd.capi import NRT_ERR_INVALID, NRT_ERR_PRECISION, NrtError
from nanort_amd.wire import CURVE_HIT_F32, HIT_F32, NODE_F32, RAY_F32
from oracle import bindings as ob
from refit_prims_model import assert_boxes_equal, refit as model_refit, topology_bytes

pytestmark = pytest.mark.gpu

BIG = np.finfo(np.float32).max
SPHERE_SIZES = ["1", "3", "5", "257", "fixture"]  # 1: the root is a leaf; 5: the leaf-size boundary; 257: subtree phase / top phase
CURVE_SCENES = ["1", "2", "5", "64", "fur"]
FAR = np.array([250.0, -130.0, 75.0], np.float32)


# ---- the two kinds behind one face --------------------------------------------------------------------------------------------
class Spheres:
    kind = "spheres"
    hit_bytes = HIT_F32.itemsize

    @staticmethod
    def scene(name):
        return sphere_fixture.scene() if name == "fixture" else scenes.random_spheres(int(name))

    @staticmethod
    def rays(name):
        r = sphere_fixture.rays()  # 31 760 rays: the camera's and the hostile extras
        return r if name == "fixture" else np.ascontiguousarray(r[::7])

    @staticmethod
    def geometry(pos, rad):
        return SphereGeometry(pos, rad)

    @staticmethod
    def restatement(nodes, idx, pos, rad, rays):
        return ob.SphereOracle().traverse(nodes, idx, pos, rad, rays)

    @staticmethod
    def same(h, m, oh, om, what=""):
        """Every field of every record and the flags, bit for bit (u and v included: all inputs here are finite)."""
        assert np.array_equal(m, om), "%s: hit flags differ at %s" % (what, np.nonzero(m != om)[0][:8])
        for f in ("t", "prim_id", "u", "v"):
            bad = np.nonzero(h[f].view(np.uint32) != oh[f].view(np.uint32))[0]
            assert bad.size == 0, "%s: %s differs in %d records, largest difference %g" % (what, f, bad.size, np.max(np.abs(h[f][bad] - oh[f][bad])))
        assert h.tobytes() == oh.tobytes(), what


class Curves:
    kind = "curves"
    hit_bytes = CURVE_HIT_F32.itemsize

    @staticmethod
    def scene(name):
        return cf.scene(name)

    @staticmethod
    def rays(name):
        return cf.all_rays()  # 4096 camera rays and the hostile ones

    @staticmethod
    def geometry(pos, rad):
        return CurveGeometry(pos, rad)

    @staticmethod
    def restatement(nodes, idx, pos, rad, rays):
        return cf.model_traverse(nodes, idx, pos, rad, rays, 4)

    @staticmethod
    def same(h, m, oh, om, what=""):
        assert np.array_equal(m, om), "%s: hit flags differ at %s" % (what, np.nonzero(m != om)[0][:8])
        assert h.dtype == CURVE_HIT_F32 and h.tobytes() == oh.tobytes(), "%s: records differ at %s" % (what, np.nonzero(h != oh)[0][:8])


KINDS = {"spheres": Spheres, "curves": Curves}
CASES = [("spheres", s) for s in SPHERE_SIZES] + [("curves", s) for s in CURVE_SCENES]
CASE_IDS = ["%s_%s" % c for c in CASES]


def deformations(pos, rad):
    """name -> (positions, radii or None, offset of the rays' origins): a jitter, a translation far outside the old bounds (the
    rays follow it), a non-uniform scale about the centroid with the radii halved, and the radii doubled or halved at unchanged
    positions.  radii None: the accel keeps the radii it holds.  Everything is finite."""
    rng = np.random.default_rng(11)
    pts = pos.reshape(-1, 3)
    c = pts.mean(axis=0)
    ext = float(np.abs(pts - c).max()) + 1.0
    zero = np.zeros(3, np.float32)
    out = []
    out.append(("jitter", (pos + rng.normal(scale=0.02 * ext, size=pos.shape)).astype(np.float32), None, zero))
    out.append(("translate", (pos + FAR).astype(np.float32), None, FAR))
    out.append(("scale", ((pts - c) * np.array([3.0, 0.25, -1.5]) + c).astype(np.float32).reshape(pos.shape), (rad * np.float32(0.5)).astype(np.float32), zero))
    out.append(("radii", pos.copy(), (rad * np.where(rng.random(rad.shape) < 0.5, 2.0, 0.5)).astype(np.float32), zero))
    return out


def built(K, pos, rad, wide4=1):
    a = BVHAccel(np.float32)
    a.SetTunable("wide4", wide4)
    assert a.Build(rad.shape[0], K.geometry(pos, rad))
    return a


def check_traces(K, a, nodes, idx, pos, rad, rays, what):
    oh, om = K.restatement(nodes, idx, pos, rad, rays)
    h, m = a.TraverseBatch(rays)
    K.same(h, m, oh, om, what)
    assert np.array_equal(a.OccludedBatch(rays), m), "%s: occlusion flags differ from the closest-hit flags" % what
    return h, m


# ---- 1. boxes, topology and traces --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide4", [1, 0], ids=["two_level", "one_level"])
@pytest.mark.parametrize("kind,size", CASES, ids=CASE_IDS)
def test_refit_boxes_topology_and_traces(kind, size, wide4):
    K = KINDS[kind]
    pos, rad = K.scene(size)
    rays = K.rays(size)
    a = built(K, pos, rad, wide4)
    n0, i0 = a.GetTree()
    held = rad  # the radii the accel holds
    hits = 0
    for name, p1, r1, shift in deformations(pos, rad):
        what = "%s %s %s" % (kind, size, name)
        a.RefitPrims(p1, r1)
        held = held if r1 is None else r1
        n1, i1 = a.GetTree()
        assert topology_bytes(n1) == topology_bytes(n0), "%s: refit changed flag / axis / data" % what
        assert i1.tobytes() == i0.tobytes(), "%s: refit changed the index array" % what
        assert_boxes_equal(n1, model_refit(kind, n0, i0, p1, held), "boxes (%s)" % what)
        moved = rays.copy()
        moved["org"] += shift
        _, m = check_traces(K, a, n1, i1, p1, held, moved, what)
        hits += int(m.sum())
    assert hits > 0  # (one curve or sphere may lie off the camera's grid after one deformation, never after all four)
    a.close()


# ---- 2. unchanged arrays ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,size", CASES, ids=CASE_IDS)
def test_refit_with_the_arrays_of_the_build_returns_the_built_boxes(kind, size):
    K = KINDS[kind]
    pos, rad = K.scene(size)
    rays = K.rays(size)
    a = built(K, pos, rad)
    n0, i0 = a.GetTree()
    h0, m0 = a.TraverseBatch(rays)
    for radii in (rad, None):  # (the second call reuses the plan)
        a.RefitPrims(pos, radii)
        n1, i1 = a.GetTree()
        assert topology_bytes(n1) == topology_bytes(n0) and i1.tobytes() == i0.tobytes()
        assert_boxes_equal(n1, n0)
        h1, m1 = a.TraverseBatch(rays)
        assert np.array_equal(m1, m0) and h1.tobytes() == h0.tobytes()
    a.close()


# ---- 3. build after refit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,size", [("spheres", "257"), ("spheres", "fixture"), ("curves", "64"), ("curves", "fur")])
def test_build_after_refit_equals_a_fresh_build(kind, size):
    """nrtBuild straight after a refit (no setter in between) builds over the refit positions and radii."""
    K = KINDS[kind]
    pos, rad = K.scene(size)
    _, p1, r1, _ = deformations(pos, rad)[2]
    a = built(K, pos, rad)
    a.RefitPrims(p1, r1)
    assert a.BuildCurrent()
    nb, ib = a.GetTree()
    b = built(K, p1, r1)
    nf, if_ = b.GetTree()
    assert nb.tobytes() == nf.tobytes() and ib.tobytes() == if_.tobytes()
    a.close()
    b.close()


# ---- 4. adopted trees ---------------------------------------------------------------------------------------------------------
def test_refit_of_an_adopted_tree_with_empty_and_unreachable_records():
    """A sphere context that adopts (nrtSetTree) a hand-extended tree: root' -> (the built root, an empty leaf), and two records
    nothing points to."""
    K = Spheres
    pos, rad = scenes.random_spheres(60)
    src = built(K, pos, rad)
    on, oi = src.GetTree()
    src.close()
    n = on.shape[0]
    nodes = np.concatenate([np.zeros(1, NODE_F32), on, np.zeros(3, NODE_F32)])
    br = nodes["flag"][1:n + 1] == 0
    nodes["data"][1:n + 1][br] += 1  # the built tree's child ids, shifted by one
    nodes[0]["flag"], nodes[0]["axis"], nodes[0]["data"] = 0, 0, (1, n + 1)
    nodes[0]["bmin"], nodes[0]["bmax"] = on[0]["bmin"], on[0]["bmax"]
    nodes[n + 1]["flag"], nodes[n + 1]["data"] = 1, (0, 0)  # empty leaf
    nodes[n + 1]["bmin"], nodes[n + 1]["bmax"] = (1, 2, 3), (4, 5, 6)  # (a refit has to replace this)
    nodes[n + 2]["flag"], nodes[n + 2]["data"] = 1, (3, 0)  # unreachable leaf
    nodes[n + 2]["bmin"], nodes[n + 2]["bmax"] = (9, 9, 9), (10, 10, 10)
    nodes[n + 3]["flag"], nodes[n + 3]["data"] = 0, (1, 2)  # unreachable branch
    nodes[n + 3]["bmin"], nodes[n + 3]["bmax"] = (-7, -7, -7), (7, 7, 7)
    a = BVHAccel(np.float32)
    a.SetMesh(SphereGeometry(pos, rad))
    a.SetTree(nodes, oi)
    p1 = (pos * np.array([2.0, 0.5, 1.0]) + 0.3).astype(np.float32)
    a.RefitPrims(p1)
    n1, i1 = a.GetTree()
    assert topology_bytes(n1) == topology_bytes(nodes) and i1.tobytes() == oi.tobytes()
    assert_boxes_equal(n1, model_refit("spheres", nodes, oi, p1, rad))
    assert np.array_equal(n1[n + 1]["bmin"], [BIG] * 3) and np.array_equal(n1[n + 1]["bmax"], [-BIG] * 3)
    assert n1[n + 2].tobytes() == nodes[n + 2].tobytes() and n1[n + 3].tobytes() == nodes[n + 3].tobytes()
    _, m = check_traces(K, a, n1, i1, p1, rad, K.rays("60"), "adopted")
    assert m.any()
    a.close()


# ---- 5. the Device form -------------------------------------------------------------------------------------------------------
def read_hits(d_hits, dtype):
    return np.frombuffer(d_hits.cpu().numpy().tobytes(), dtype=dtype)


def test_refit_device_spheres_ten_frames_on_side_streams():
    """A torch kernel advects the centres on a side stream, RefitPrimsDevice runs behind it on that stream, TraverseBatchDevice on
    another stream with no host sync in between: the records of a frame in the middle and of the last are the restatement's on
    that frame's centres and read-back tree."""
    import torch

    K = Spheres
    pos, rad = K.scene("fixture")
    rays = np.ascontiguousarray(K.rays("fixture")[::2])
    a = built(K, pos, rad)
    n0, i0 = a.GetTree()
    s_refit, s_trace = torch.cuda.Stream(), torch.cuda.Stream()
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
    d_c = torch.from_numpy(pos.copy()).cuda()
    d_vel = torch.from_numpy(np.random.default_rng(2).normal(scale=0.01, size=pos.shape).astype(np.float32)).cuda()
    d_hits = torch.zeros((rays.shape[0] * K.hit_bytes,), dtype=torch.uint8, device="cuda")
    d_mask = torch.zeros((rays.shape[0],), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    checked = 0
    for frame in range(10):
        with torch.cuda.stream(s_refit):
            d_c.add_(d_vel)
            a.RefitPrimsDevice(d_c, stream=s_refit)
        a.TraverseBatchDevice(d_rays, d_hits, d_mask, stream=s_trace.cuda_stream)
        if frame in (4, 9):
            s_trace.synchronize()
            s_refit.synchronize()
            c1 = d_c.cpu().numpy()
            n1, i1 = a.GetTree()
            assert topology_bytes(n1) == topology_bytes(n0) and i1.tobytes() == i0.tobytes()
            assert_boxes_equal(n1, model_refit("spheres", n0, i0, c1, rad), "boxes (frame %d)" % frame)
            oh, om = K.restatement(n1, i1, c1, rad, rays)
            K.same(read_hits(d_hits, HIT_F32), d_mask.cpu().numpy(), oh, om, "frame %d" % frame)
            assert om.any()
            checked += 1
    assert checked == 2
    torch.cuda.synchronize()
    a.close()


def test_refit_device_curves_moved_control_points():
    import torch

    K = Curves
    pos, rad = K.scene("fur")
    rays = K.rays("fur")
    a = built(K, pos, rad)
    n0, i0 = a.GetTree()
    _, p1, r1, _ = deformations(pos, rad)[2]
    s_refit, s_trace = torch.cuda.Stream(), torch.cuda.Stream()
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
    d_hits = torch.zeros((rays.shape[0] * K.hit_bytes,), dtype=torch.uint8, device="cuda")
    d_mask = torch.zeros((rays.shape[0],), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s_refit):
        d_p, d_r = torch.from_numpy(p1).cuda(), torch.from_numpy(r1).cuda()
        a.RefitPrimsDevice(d_p, d_r, stream=s_refit)
    a.TraverseBatchDevice(d_rays, d_hits, d_mask, stream=s_trace.cuda_stream)
    s_trace.synchronize()
    n1, i1 = a.GetTree()
    assert topology_bytes(n1) == topology_bytes(n0) and i1.tobytes() == i0.tobytes()
    assert_boxes_equal(n1, model_refit("curves", n0, i0, p1, r1))
    oh, om = K.restatement(n1, i1, p1, r1, rays)
    K.same(read_hits(d_hits, CURVE_HIT_F32), d_mask.cpu().numpy(), oh, om, "device curves")
    assert om.any()
    with pytest.raises(ValueError):  # shapes are checked against the kind and count before the library is called
        a.RefitPrimsDevice(d_p[:-1].contiguous(), d_r)
    with pytest.raises(ValueError):
        a.RefitPrimsDevice(d_p, d_r[:, :2].contiguous())
    with pytest.raises(ValueError):
        a.RefitPrimsDevice(d_p[:, :, :2], d_r)  # not contiguous
    with pytest.raises(TypeError):
        a.RefitPrimsDevice(d_p.double(), d_r)
    torch.cuda.synchronize()
    a.close()


# ---- 6. refusals write nothing ------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    import torch

    K = Spheres
    pos, rad = scenes.random_spheres(257)
    rays = K.rays("257")
    p1 = (pos + np.float32(0.25)).astype(np.float32)
    a = BVHAccel(np.float32)
    L = a._L
    ptr = lambda x: x.ctypes.data  # noqa: E731

    def refused(st, want, word, ctx=a):
        msg = L.nrtLastError(ctx._h).decode()
        assert st == want and word in msg, (st, msg)

    refused(L.nrtRefitPrims_f32(a._h, ptr(p1), ptr(rad), 257), NRT_ERR_INVALID, "no tree")  # a fresh context
    a.SetMesh(SphereGeometry(pos, rad))
    with pytest.raises(NrtError) as e:  # primitives, but no tree
        a.RefitPrims(p1)
    assert e.value.status == NRT_ERR_INVALID and "no tree" in str(e.value)
    assert a.BuildCurrent()
    n0, i0 = a.GetTree()
    h0, m0 = a.TraverseBatch(rays)
    d_p, d_r = torch.from_numpy(p1).cuda(), torch.from_numpy(rad).cuda()
    assert L.nrtRefitPrims_f32(None, ptr(p1), ptr(rad), 257) == NRT_ERR_INVALID  # NULL context
    assert L.nrtRefitPrimsDevice_f32(None, d_p.data_ptr(), d_r.data_ptr(), 257, None) == NRT_ERR_INVALID
    refused(L.nrtRefitPrims_f32(a._h, None, ptr(rad), 257), NRT_ERR_INVALID, "NULL")
    refused(L.nrtRefitPrimsDevice_f32(a._h, None, d_r.data_ptr(), 257, None), NRT_ERR_INVALID, "NULL")
    refused(L.nrtRefitPrims_f32(a._h, ptr(p1), ptr(rad), 256), NRT_ERR_INVALID, "num_prims")
    refused(L.nrtRefitPrims_f32(a._h, ptr(p1), None, 258), NRT_ERR_INVALID, "num_prims")
    refused(L.nrtRefitPrimsDevice_f32(a._h, d_p.data_ptr(), d_r.data_ptr(), 0, None), NRT_ERR_INVALID, "num_prims")
    refused(L.nrtRefitPrimsDevice_f32(a._h, d_p.data_ptr() + 2, d_r.data_ptr(), 257, None), NRT_ERR_INVALID, "aligned")
    refused(L.nrtRefitPrimsDevice_f32(a._h, d_p.data_ptr(), d_r.data_ptr() + 1, 257, None), NRT_ERR_INVALID, "aligned")
    for bad in (p1[:-1], np.zeros((257, 4), np.float32)):  # the Python layer: shapes against the kind and count
        with pytest.raises(ValueError):
            a.RefitPrims(bad)
    with pytest.raises(ValueError):
        a.RefitPrims(p1, rad[:-1])
    torch.cuda.synchronize()
    n1, i1 = a.GetTree()
    assert n1.tobytes() == n0.tobytes() and i1.tobytes() == i0.tobytes()
    h1, m1 = a.TraverseBatch(rays)
    assert np.array_equal(m1, m0) and h1.tobytes() == h0.tobytes() and m0.any()
    a.close()

    # a triangle context: the message points to nrtRefit; a cylinder context: the message says why; an fp64 context: precision
    v, f = scenes.load_c1_mesh()
    cam = scenes.camera_rays(48, 32)
    t = BVHAccel(np.float32)
    assert t.Build(f.shape[0], TriangleMesh(v, f))
    tn, ti = t.GetTree()
    th, tm = t.TraverseBatch(cam)
    refused(L.nrtRefitPrims_f32(t._h, ptr(v), None, f.shape[0]), NRT_ERR_INVALID, "nrtRefit /", t)
    with pytest.raises(NrtError) as e:
        t.RefitPrims(v)
    assert e.value.status == NRT_ERR_INVALID and "triangles" in str(e.value)
    tn1, ti1 = t.GetTree()
    th1, tm1 = t.TraverseBatch(cam)
    assert tn1.tobytes() == tn.tobytes() and ti1.tobytes() == ti.tobytes() and th1.tobytes() == th.tobytes() and np.array_equal(tm1, tm)
    t.close()
    ends, er = scenes.random_cylinders(50)
    c = BVHAccel(np.float32)
    assert c.Build(50, CylinderGeometry(ends, er))
    cn, ci = c.GetTree()
    ch, cm = c.TraverseBatch(rays)
    refused(L.nrtRefitPrims_f32(c._h, ptr(ends), ptr(er), 50), NRT_ERR_INVALID, "segments", c)
    with pytest.raises(NrtError) as e:
        c.RefitPrims(ends, er)
    assert e.value.status == NRT_ERR_INVALID and "cylinders" in str(e.value)
    cn1, ci1 = c.GetTree()
    ch1, cm1 = c.TraverseBatch(rays)
    assert cn1.tobytes() == cn.tobytes() and ci1.tobytes() == ci.tobytes() and ch1.tobytes() == ch.tobytes() and np.array_equal(cm1, cm)
    c.close()
    d = BVHAccel(np.float64)
    assert d.Build(f.shape[0], TriangleMesh(v.astype(np.float64), f))
    dn, _ = d.GetTree()
    refused(L.nrtRefitPrims_f32(d._h, ptr(v), None, f.shape[0]), NRT_ERR_PRECISION, "f64", d)
    refused(L.nrtRefitPrimsDevice_f32(d._h, d_p.data_ptr(), None, f.shape[0], None), NRT_ERR_PRECISION, "f64", d)
    assert d.GetTree()[0].tobytes() == dn.tobytes()
    d.close()


# ---- 7. the header ------------------------------------------------------------------------------------------------------------
def _prims_file(path, pos, rad):
    with open(path, "wb") as fp:
        fp.write(np.array([rad.shape[0]], dtype=np.uint32).tobytes() + np.ascontiguousarray(pos, np.float32).tobytes()
                 + np.ascontiguousarray(rad, np.float32).tobytes())


def _rays_file(path, rays):
    with open(path, "wb") as fp:
        fp.write(np.array([rays.shape[0]], dtype=np.uint64).tobytes() + np.ascontiguousarray(rays, RAY_F32).tobytes())


def _trees(path):
    raw = open(path, "rb").read()
    nn, ni = (int(x) for x in np.frombuffer(raw, np.uint64, 2))
    before = np.frombuffer(raw, NODE_F32, nn, 16)
    idx = np.frombuffer(raw, np.uint32, ni, 16 + 40 * nn)
    return before, idx, np.frombuffer(raw, NODE_F32, nn, 16 + 40 * nn + 4 * ni)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    from test_refit_prims_abi import compile_driver

    return compile_driver(tmp_path_factory.mktemp("refit_prims_check") / "refit_prims_check")


@pytest.mark.parametrize("devices", [None, "0,0"], ids=["one", "replicas"])
def test_header_refit_geometry(driver, tmp_path, devices):
    exe = driver
    sets = {}
    for K, size, stem, rays_name in ((Spheres, "257", "spheres", "srays.bin"), (Curves, "fur", "curves", "crays.bin")):
        pos, rad = K.scene(size)
        _, p1, r1, _ = deformations(pos, rad)[2]
        _prims_file(str(tmp_path / (stem + "0.bin")), pos, rad)
        _prims_file(str(tmp_path / (stem + "1.bin")), p1, r1)
        _rays_file(str(tmp_path / rays_name), K.rays(size)[::3])
        sets[stem] = (K.kind, p1, r1)
    env = dict(os.environ)
    env.pop("NANORT_HIP_DEVICES", None)
    if devices:
        env["NANORT_HIP_DEVICES"] = devices
    r = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stdout[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("devices ")][-1].split()
    assert int(line[1]) == (2 if devices else 1), r.stdout
    assert int(line[3]) > 40 and int(line[5]) == 0, r.stdout
    for stem, (kind, p1, r1) in sets.items():  # GetNodes() after the refit returns the refit boxes
        before, idx, after = _trees(str(tmp_path / (stem + "_out.bin")))
        assert topology_bytes(after) == topology_bytes(before)
        assert_boxes_equal(after, model_refit(kind, before, idx, p1, r1), "GetNodes() after RefitGeometry (%s)" % stem)

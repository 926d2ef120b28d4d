"""Closest-point test fixture (nrtClosestPointBatch*, include/nanort_closest.h): the CPU model (tests/closest_model.cc: brute force
over the faces and a plain walk of a given tree), the header's host form (tests/cpp/closest_host_shim.cc over include/nanort.h,
without the backend), and the point sets the CPU and the GPU tests share.

The point sets lie over the C1 mesh; each has more than 128 points and a count that is no multiple of 64:
  a  hit points of scenes.camera_rays(96, 64), pushed off the surface by random offsets up to a tenth of the mesh's diagonal
  b  uniform points in 1.5 x the bounding box
  c  every vertex, some edge midpoints and some centroids: dist2 is exactly 0 for the faces at a vertex, near 0 across an edge, so
     the smallest-prim_id rule decides
  d  points on a quarter-integer grid
  e  a handful with NaN or inf coordinates, and points 1e6 away
max_dist per point cycles through +inf, a finite value, 0, a finite value, NaN, a finite value, -1, a finite value — the finite ones
drawn around the set's median distance — so consecutive points always differ in it."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from nanort_amd import scenes
from nanort_amd.wire import closest_dtype, node_dtype, point_dtype, suffix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODEL = None
_SHIM = None
_SETS = {}
_BRUTE = {}
DEFAULT_OPTS = (0, 0x7FFFFFFF, 0xFFFFFFFF)  # prim_ids_range, skip_prim_id: BVHTraceOptions' defaults
SET_NAMES = ("a", "b", "c", "d", "e")


def _compile(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def model_lib():
    """g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC tests/closest_model.cc, once per process."""
    global _MODEL
    if _MODEL is None:
        so = os.path.join(tempfile.mkdtemp(prefix="nrt_closest_model_"), "libclosest_model.so")
        _compile(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-shared", "-fPIC", "-I",
                  os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tests", "closest_model.cc")])
        L = ctypes.CDLL(so)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        for s in ("f32", "f64"):
            getattr(L, "clm_brute_" + s).argtypes = [vp, vp, u32, vp, u64, vp, vp, vp, vp]
            getattr(L, "clm_brute_" + s).restype = None
            getattr(L, "clm_walk_" + s).argtypes = [vp, vp, vp, vp, vp, u64, vp, vp, vp, vp]
            getattr(L, "clm_walk_" + s).restype = None
            getattr(L, "clm_bound_search_" + s).argtypes = [vp, u64, vp]
            getattr(L, "clm_bound_search_" + s).restype = None
        _MODEL = L
    return _MODEL


def shim_lib():
    """tests/cpp/closest_host_shim.cc over include/nanort.h, compiled WITHOUT the backend, once per process."""
    global _SHIM
    if _SHIM is None:
        so = os.path.join(tempfile.mkdtemp(prefix="nrt_closest_shim_"), "libclosest_shim.so")
        _compile(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-shared", "-fPIC", "-I",
                  os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tests", "cpp", "closest_host_shim.cc")])
        L = ctypes.CDLL(so)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        for s in ("f32", "f64"):
            getattr(L, "chs_create_" + s).argtypes = [vp, u32, vp, u32]
            getattr(L, "chs_create_" + s).restype = vp
            getattr(L, "chs_sizes_" + s).argtypes = [vp, vp]
            getattr(L, "chs_sizes_" + s).restype = None
            getattr(L, "chs_tree_" + s).argtypes = [vp, vp, vp]
            getattr(L, "chs_tree_" + s).restype = None
            getattr(L, "chs_closest_" + s).argtypes = [vp, vp, u64, vp, vp, vp]
            getattr(L, "chs_closest_" + s).restype = ctypes.c_int
            getattr(L, "chs_destroy_" + s).argtypes = [vp]
            getattr(L, "chs_destroy_" + s).restype = None
        _SHIM = L
    return _SHIM


def _opt3(opts):
    return np.asarray(DEFAULT_OPTS if opts is None else opts, dtype=np.uint32)


def trace_options(opts):
    """(range0, range1, skip) as the library's trace options record (None: None, the defaults)."""
    from nanort_amd.wire import default_trace_options

    if opts is None:
        return None
    o = default_trace_options()
    o["prim_ids_range"] = (opts[0], opts[1])
    o["skip_prim_id"] = opts[2]
    return o


def make_points(real, xyz, max_dist):
    pts = np.zeros((np.asarray(xyz).reshape(-1, 3).shape[0],), dtype=point_dtype(real))
    pts["p"] = np.asarray(xyz, dtype=real).reshape(-1, 3)
    pts["max_dist"] = np.asarray(max_dist, dtype=real)
    return pts


def brute(verts, faces, pts, opts=None, ties=False):
    """The model's brute-force loop over the faces: (records, found[, faces attaining the minimum per point])."""
    real = verts.dtype
    verts = np.ascontiguousarray(verts)
    faces = np.ascontiguousarray(faces, dtype=np.uint32)
    pts = np.ascontiguousarray(pts, dtype=point_dtype(real))
    n = pts.shape[0]
    out = np.zeros((n,), dtype=closest_dtype(real))
    found = np.zeros((n,), dtype=np.uint8)
    t = np.zeros((n,), dtype=np.uint32) if ties else None
    getattr(model_lib(), "clm_brute_" + suffix(real))(_p(verts), _p(faces), faces.shape[0], _p(pts), n, _p(_opt3(opts)), _p(out), _p(found), _p(t))
    return (out, found, t) if ties else (out, found)


def walk(nodes, indices, verts, faces, pts, opts=None, count=False):
    """The model's walk over the given tree: (records, found[, nodes opened, most stack entries waiting at once])."""
    real = verts.dtype
    nodes = np.ascontiguousarray(nodes, dtype=node_dtype(real))
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    verts = np.ascontiguousarray(verts)
    faces = np.ascontiguousarray(faces, dtype=np.uint32)
    pts = np.ascontiguousarray(pts, dtype=point_dtype(real))
    n = pts.shape[0]
    out = np.zeros((n,), dtype=closest_dtype(real))
    found = np.zeros((n,), dtype=np.uint8)
    opened = np.zeros((2,), dtype=np.uint64)
    getattr(model_lib(), "clm_walk_" + suffix(real))(_p(nodes), _p(indices), _p(verts), _p(faces), _p(pts), n, _p(_opt3(opts)), _p(out), _p(found),
                                                     _p(opened))
    return (out, found, int(opened[0]), int(opened[1])) if count else (out, found)


class HostAccel:
    """include/nanort.h's BVHAccel<T> over (TriangleMesh, TriangleSAHPred), built on the host without the backend."""

    def __init__(self, verts, faces):
        self.real = verts.dtype
        self.s = suffix(self.real)
        self.L = shim_lib()
        verts = np.ascontiguousarray(verts)
        faces = np.ascontiguousarray(faces, dtype=np.uint32)
        self.h = getattr(self.L, "chs_create_" + self.s)(_p(verts), verts.shape[0], _p(faces), faces.shape[0])
        assert self.h, "the header's host Build failed"

    def __del__(self):
        if getattr(self, "h", None):
            getattr(self.L, "chs_destroy_" + self.s)(self.h)
            self.h = None

    def tree(self):
        sz = np.zeros((2,), dtype=np.uint64)
        getattr(self.L, "chs_sizes_" + self.s)(self.h, _p(sz))
        nodes = np.zeros((int(sz[0]),), dtype=node_dtype(self.real))
        indices = np.zeros((int(sz[1]),), dtype=np.uint32)
        getattr(self.L, "chs_tree_" + self.s)(self.h, _p(nodes), _p(indices))
        return nodes, indices

    def closest(self, pts, opts=None):
        pts = np.ascontiguousarray(pts, dtype=point_dtype(self.real))
        n = pts.shape[0]
        out = np.zeros((n,), dtype=closest_dtype(self.real))
        found = np.zeros((n,), dtype=np.uint8)
        assert getattr(self.L, "chs_closest_" + self.s)(self.h, _p(pts), n, _p(_opt3(opts)), _p(out), _p(found)) == 0
        return out, found


def _odd_count(xyz):
    """More than 128 points, and no multiple of 64 of them."""
    if xyz.shape[0] % 64 == 0:
        xyz = xyz[:-1]
    assert xyz.shape[0] > 128 and xyz.shape[0] % 64 != 0
    return xyz


def _radii(rng, real, verts, faces, xyz, diag):
    """One max_dist per point: +inf, finite, 0, finite, NaN, finite, -1, finite, ... — the finite ones around the median distance."""
    n = xyz.shape[0]
    free, _ = brute(verts, faces, make_points(real, xyz, np.inf))
    dist = np.sqrt(free["dist2"][free["prim_id"] != 0xFFFFFFFF].astype(np.float64))
    med = float(np.median(dist)) if dist.size else 0.0
    if not med > 0.0:
        med = 1e-3 * diag
    md = med * np.exp(rng.uniform(-1.0, 1.0, size=n))
    kind = np.arange(n) % 8
    md[kind == 0] = np.inf
    md[kind == 2] = 0.0
    md[kind == 4] = np.nan
    md[kind == 6] = -1.0
    md = md.astype(real)
    same = md[1:] == md[:-1]  # (two finite neighbours never meet; a finite value that rounds to its neighbour's special one cannot either)
    assert not same.any()
    return md


def point_sets(real):
    """{name: points} of the accel's precision over the C1 mesh (the same coordinates in both precisions, rounded to fp32 first)."""
    real = np.dtype(real)
    if real in _SETS:
        return _SETS[real]
    from oracle.bindings import Oracle

    v32, f = scenes.load_c1_mesh()
    verts = v32.astype(real)
    bmin, bmax = v32.min(0).astype(np.float64), v32.max(0).astype(np.float64)
    diag = float(np.linalg.norm(bmax - bmin))
    rng = np.random.default_rng(20261021)
    xyz = {}
    # a: off the surface
    orc = Oracle()
    nodes, idx, _ = orc.build(v32, f)
    rays = scenes.camera_rays(96, 64)
    hits, mask = orc.traverse(nodes, idx, v32, f, rays)
    m = mask != 0
    hp = rays["org"][m].astype(np.float64) + rays["dir"][m].astype(np.float64) * hits["t"][m].astype(np.float64)[:, None]
    d = rng.normal(size=hp.shape)
    d /= np.linalg.norm(d, axis=1)[:, None]
    xyz["a"] = _odd_count((hp + d * rng.uniform(0.0, 0.1 * diag, size=(hp.shape[0], 1)))[::3])
    # b: uniform in 1.5 x the box
    c, h = 0.5 * (bmin + bmax), 0.75 * (bmax - bmin)
    xyz["b"] = _odd_count(rng.uniform(c - h, c + h, size=(1003, 3)))
    # c: vertices, edge midpoints, centroids
    fe = f[rng.choice(f.shape[0], size=300, replace=False)]
    mid = 0.5 * (v32[fe[:, 0]].astype(np.float64) + v32[fe[:, 1]].astype(np.float64))
    fc = f[rng.choice(f.shape[0], size=200, replace=False)]
    cen = (v32[fc[:, 0]].astype(np.float64) + v32[fc[:, 1]] + v32[fc[:, 2]]) / 3.0
    xyz["c"] = _odd_count(np.concatenate([v32.astype(np.float64), mid, cen]))
    # d: the quarter-integer grid
    lo, hi = np.floor(bmin * 4) / 4, np.ceil(bmax * 4) / 4
    g = np.stack([rng.integers(int(lo[k] * 4), int(hi[k] * 4) + 1, size=777) / 4.0 for k in range(3)], axis=1)
    xyz["d"] = _odd_count(g)
    # e: non-finite coordinates, and far away
    far = rng.normal(size=(130, 3))
    far = far / np.linalg.norm(far, axis=1)[:, None] * 1e6
    bad = np.tile(c, (9, 1))
    bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
    bad[3] = np.nan
    bad[4] = np.inf
    bad[5, 0], bad[5, 1] = np.inf, np.nan
    bad[6, 2] = np.nan
    bad[7, 0] = -np.inf
    bad[8, 1] = np.nan
    e = np.concatenate([far[:60], bad, far[60:]])
    xyz["e"] = _odd_count(e)
    sets = {}
    for name in SET_NAMES:
        p = xyz[name].astype(np.float32).astype(real)  # (the same points in both precisions)
        with np.errstate(invalid="ignore"):
            sets[name] = make_points(real, p, _radii(rng, real, verts, f, p, diag))
    _check_sets(real, verts, f, sets)
    _SETS[real] = sets
    return sets


def mesh(real):
    v32, f = scenes.load_c1_mesh()
    return np.ascontiguousarray(v32.astype(real)), np.ascontiguousarray(f, dtype=np.uint32)


def middle_third(nf):
    return (nf // 3, 2 * nf // 3, 0xFFFFFFFF)


def busiest_face(real):
    """The face that is the answer of the most points of sets a and b: what the skip_prim_id cases skip."""
    ids = np.concatenate([expected(real, k)[0]["prim_id"] for k in ("a", "b")])
    ids = ids[ids != 0xFFFFFFFF]
    return int(np.bincount(ids).argmax())


def option_cases(real):
    """{name: (range0, range1, skip)}: range, skip and both."""
    nf = mesh(real)[1].shape[0]
    r0, r1, _ = middle_third(nf)
    skip = busiest_face(real)
    mid = expected(real, "b", (r0, r1, 0xFFFFFFFF))[0]["prim_id"]
    mid = mid[mid != 0xFFFFFFFF]
    return {"range": (r0, r1, 0xFFFFFFFF), "skip": (0, 0x7FFFFFFF, skip), "both": (r0, r1, int(np.bincount(mid).argmax()))}


def expected(real, name, opts=None):
    """The model's brute force over set `name` (computed once per precision, set and options; do not write to it)."""
    key = (np.dtype(real), name, tuple(DEFAULT_OPTS if opts is None else opts))
    if key not in _BRUTE:
        v, f = mesh(real)
        out, found = brute(v, f, point_sets(real)[name], opts)
        out.setflags(write=False)
        found.setflags(write=False)
        _BRUTE[key] = (out, found)
    return _BRUTE[key]


def _check_sets(real, verts, faces, sets):
    """What the sets must exercise, by brute force alone."""
    nf = faces.shape[0]
    for name in ("a", "b"):
        pts = sets[name]
        out, found = brute(verts, faces, pts)
        fin = np.isfinite(pts["max_dist"]) & (pts["max_dist"] > 0)
        assert fin.sum() >= pts.shape[0] // 4
        assert found[fin].sum() >= fin.sum() / 10.0, "set %s: too few finite-radius points are found" % name
        assert (found[fin] == 0).sum() >= fin.sum() / 10.0, "set %s: too few finite-radius points are not found" % name
    tied = 0
    for name in ("c", "d"):
        _, found, ties = brute(verts, faces, sets[name], ties=True)
        tied += int((ties >= 2).sum())
    assert tied >= 100, "sets c and d: only %d points have their minimum attained by two or more faces" % tied
    # The options must matter: skipping the busiest face, or admitting the middle third of the faces only, changes at least a tenth
    # of the ANSWERS of sets a and b — of the points that have one.  (A point that finds nothing under the default options finds
    # nothing under narrower ones: its record cannot change, and with the radii above that is the larger half of every set.  Of all
    # 1804 points of a and b the skipped face changes 101 and the range 714.)
    ab = np.concatenate([sets["a"], sets["b"]])
    base, base_found = brute(verts, faces, ab)
    have = np.nonzero(base_found)[0]
    skip = int(np.bincount(base["prim_id"][have]).argmax())
    for what, opts in (("skip_prim_id", (0, 0x7FFFFFFF, skip)), ("prim_ids_range", middle_third(nf))):
        out, _ = brute(verts, faces, ab, opts)
        changed = sum(out[i].tobytes() != base[i].tobytes() for i in have)
        assert changed >= have.shape[0] / 10.0, "%s changes only %d of %d answers" % (what, changed, have.shape[0])


def assert_same(out, found, ref_out, ref_found, what=""):
    """Byte-identical records and found bytes."""
    assert np.array_equal(np.asarray(found), np.asarray(ref_found)), "%s: found bytes differ at %s" % (what, np.nonzero(np.asarray(found) != np.asarray(ref_found))[0][:8])
    if out.tobytes() != ref_out.tobytes():
        bad = [i for i in range(out.shape[0]) if out[i].tobytes() != ref_out[i].tobytes()]
        raise AssertionError("%s: %d of %d records differ, first %s:\n%s\n%s" % (what, len(bad), out.shape[0], bad[:4], out[bad[:4]], ref_out[bad[:4]]))

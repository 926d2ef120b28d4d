"""Nearest-faces test fixture (nrtNearestFacesBatch*, the K-nearest rule of include/nanort_closest.h): the CPU model
(tests/nearest_model.cc: brute force over the faces with the K-buffer, and a plain walk of a given tree), the header's host form
(tests/cpp/nearest_host_shim.cc over include/nanort.h, without the backend), the point sets and conditions the CPU and the GPU tests
share, and an independent statement of the answer in numpy (independent_rows), because the model shares the header's insertion
rule with the code under test and cannot vouch for it.

The point sets are closest_fixture's a–e over the C1 mesh (980 faces), in two copies: one with every max_dist = +inf (radii=False),
and one per K with radii of its own (radii=True) — +inf, finite, 0, finite, NaN, finite, -1, finite, ... as closest_fixture cycles
them, the finite ones drawn around the set's median distance to the ceil(K / 2)-th nearest face, so that about half of a row is
found.  _check_sets asserts, from the model's brute force alone, what the sets must exercise for every K of KS."""
import ctypes
import os
import tempfile

import numpy as np

import closest_fixture as cf
from nanort_amd.wire import closest_dtype, node_dtype, point_dtype, suffix

ROOT = cf.ROOT
KS = (1, 2, 4, 7, 64)
SET_NAMES = cf.SET_NAMES
_MODEL = None
_SHIM = None
_SETS = {}
_BRUTE = {}
_CHECKED = set()
_FACE_DIST2 = {}
_p = cf._p
_opt3 = cf._opt3


def model_lib():
    """g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC tests/nearest_model.cc, once per process."""
    global _MODEL
    if _MODEL is None:
        so = os.path.join(tempfile.mkdtemp(prefix="nrt_nearest_model_"), "libnearest_model.so")
        cf._compile(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-shared", "-fPIC", "-I",
                     os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tests", "nearest_model.cc")])
        L = ctypes.CDLL(so)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        for s in ("f32", "f64"):
            getattr(L, "nrm_brute_" + s).argtypes = [vp, vp, u32, vp, u64, u32, vp, vp, vp, ctypes.c_int]
            getattr(L, "nrm_brute_" + s).restype = None
            getattr(L, "nrm_walk_" + s).argtypes = [vp, vp, vp, vp, vp, u64, u32, vp, vp, vp, vp]
            getattr(L, "nrm_walk_" + s).restype = None
        _MODEL = L
    return _MODEL


def shim_lib():
    """tests/cpp/nearest_host_shim.cc over include/nanort.h, compiled WITHOUT the backend, once per process."""
    global _SHIM
    if _SHIM is None:
        so = os.path.join(tempfile.mkdtemp(prefix="nrt_nearest_shim_"), "libnearest_shim.so")
        cf._compile(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-shared", "-fPIC", "-I",
                     os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tests", "cpp", "nearest_host_shim.cc")])
        L = ctypes.CDLL(so)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        for s in ("f32", "f64"):
            getattr(L, "nhs_create_" + s).argtypes = [vp, u32, vp, u32]
            getattr(L, "nhs_create_" + s).restype = vp
            getattr(L, "nhs_nearest_" + s).argtypes = [vp, vp, u64, u32, vp, vp, vp]
            getattr(L, "nhs_nearest_" + s).restype = ctypes.c_int
            getattr(L, "nhs_destroy_" + s).argtypes = [vp]
            getattr(L, "nhs_destroy_" + s).restype = None
        _SHIM = L
    return _SHIM


def brute(verts, faces, pts, k, opts=None, reversed_order=False):
    """The model's brute-force loop over the faces (in descending id order if `reversed_order`): (records[n, k], counts)."""
    real = verts.dtype
    verts = np.ascontiguousarray(verts)
    faces = np.ascontiguousarray(faces, dtype=np.uint32)
    pts = np.ascontiguousarray(pts, dtype=point_dtype(real))
    n = pts.shape[0]
    out = np.zeros((n, k), dtype=closest_dtype(real))
    counts = np.zeros((n,), dtype=np.uint32)
    getattr(model_lib(), "nrm_brute_" + suffix(real))(_p(verts), _p(faces), faces.shape[0], _p(pts), n, k, _p(_opt3(opts)), _p(out), _p(counts),
                                                      1 if reversed_order else 0)
    return out, counts


def walk(nodes, indices, verts, faces, pts, k, opts=None, count=False):
    """The model's walk over the given tree: (records[n, k], counts[, nodes opened, most stack entries waiting at once])."""
    real = verts.dtype
    nodes = np.ascontiguousarray(nodes, dtype=node_dtype(real))
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    verts = np.ascontiguousarray(verts)
    faces = np.ascontiguousarray(faces, dtype=np.uint32)
    pts = np.ascontiguousarray(pts, dtype=point_dtype(real))
    n = pts.shape[0]
    out = np.zeros((n, k), dtype=closest_dtype(real))
    counts = np.zeros((n,), dtype=np.uint32)
    opened = np.zeros((2,), dtype=np.uint64)
    getattr(model_lib(), "nrm_walk_" + suffix(real))(_p(nodes), _p(indices), _p(verts), _p(faces), _p(pts), n, k, _p(_opt3(opts)), _p(out),
                                                     _p(counts), _p(opened))
    return (out, counts, int(opened[0]), int(opened[1])) if count else (out, counts)


class HostAccel:
    """include/nanort.h's BVHAccel<T> over (TriangleMesh, TriangleSAHPred), built on the host without the backend."""

    def __init__(self, verts, faces):
        self.real = verts.dtype
        self.s = suffix(self.real)
        self.L = shim_lib()
        verts = np.ascontiguousarray(verts)
        faces = np.ascontiguousarray(faces, dtype=np.uint32)
        self.h = getattr(self.L, "nhs_create_" + self.s)(_p(verts), verts.shape[0], _p(faces), faces.shape[0])
        assert self.h, "the header's host Build failed"

    def __del__(self):
        if getattr(self, "h", None):
            getattr(self.L, "nhs_destroy_" + self.s)(self.h)
            self.h = None

    def nearest(self, pts, k, opts=None):
        pts = np.ascontiguousarray(pts, dtype=point_dtype(self.real))
        n = pts.shape[0]
        out = np.zeros((n, k), dtype=closest_dtype(self.real))
        counts = np.zeros((n,), dtype=np.uint32)
        assert getattr(self.L, "nhs_nearest_" + self.s)(self.h, _p(pts), n, k, _p(_opt3(opts)), _p(out), _p(counts)) == 0
        return out, counts


def searchable(pts):
    with np.errstate(invalid="ignore"):
        return np.isfinite(pts["p"]).all(axis=1) & (pts["max_dist"] >= 0)


def _own_radii(real, name, xyz, k):
    """One max_dist per point, cycling as closest_fixture._radii does; the finite ones around the median distance from the set's
    points to their ceil(k / 2)-th nearest face (by the model's brute force with +inf)."""
    v, f = cf.mesh(real)
    half = -(-k // 2)
    rows, counts = brute(v, f, cf.make_points(real, xyz, np.inf), half)
    dist = np.sqrt(rows[counts == half, half - 1]["dist2"].astype(np.float64))
    dist = dist[dist > 0]
    diag = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0).astype(np.float64)))
    med = float(np.median(dist)) if dist.size else 1e-3 * diag
    n = xyz.shape[0]
    rng = np.random.default_rng(20261021 + 1000 * k + SET_NAMES.index(name))
    md = med * np.exp(rng.uniform(-1.0, 1.0, size=n))
    kind = np.arange(n) % 8
    md[kind == 0] = np.inf
    md[kind == 2] = 0.0
    md[kind == 4] = np.nan
    md[kind == 6] = -1.0
    return md.astype(real)


def point_sets(real, k=None):
    """{name: points} over the C1 mesh: closest_fixture's coordinates with every max_dist = +inf (k None), or with the radii drawn
    for K = k.  Computed once; do not write."""
    real = np.dtype(real)
    key = (real, k)
    if key not in _SETS:
        base = cf.point_sets(real)
        sets = {}
        for name in SET_NAMES:
            xyz = base[name]["p"]
            with np.errstate(invalid="ignore"):
                sets[name] = cf.make_points(real, xyz, np.inf if k is None else _own_radii(real, name, xyz, k))
            sets[name].setflags(write=False)
        _SETS[key] = sets
    return _SETS[key]


def expected(real, name, k, radii, opts=None):
    """The model's brute force over set `name` (its +inf copy, or the copy with K's own radii), K = k: (records[n, k], counts).
    Computed once per precision, set, K, copy and options; do not write to it."""
    check_sets(real)
    return _expected(real, name, k, radii, opts)


def _expected(real, name, k, radii, opts=None):
    key = (np.dtype(real), name, k, bool(radii), tuple(cf.DEFAULT_OPTS if opts is None else opts))
    if key not in _BRUTE:
        v, f = cf.mesh(real)
        out, counts = brute(v, f, point_sets(real, k if radii else None)[name], k, opts)
        out.setflags(write=False)
        counts.setflags(write=False)
        _BRUTE[key] = (out, counts)
    return _BRUTE[key]


def restrictions(real):
    """{name: (range0, range1, skip)}: closest_fixture's busiest_face and middle_third cases."""
    nf = cf.mesh(real)[1].shape[0]
    return {"busiest_face": (0, 0x7FFFFFFF, cf.busiest_face(real)), "middle_third": cf.middle_third(nf)}


def check_sets(real):
    """What the sets must exercise, from the model's brute force alone, for every K of KS (once per precision).

    * With K's own radii, of the finite-radius points of all five sets at least a tenth have count == K and — for K >= 2 — at least
      a tenth have 0 < count < K.  (K = 1 has no count strictly between 0 and K: there at least a tenth have count == 0, the
      condition closest_fixture sets for its radii.)
    * With +inf every Searchable point has count == min(K, admitted faces), and every other point 0.
    * On set c at least 100 points have their K-th and (K+1)-th keys equal in dist2, for K = 2 and for K = 4: prim_id decides
      the eviction.
    * Each of the two restrictions of the options changes at least a tenth of the rows of sets a and b, on the +inf copy."""
    real = np.dtype(real)
    if real in _CHECKED:
        return
    v, f = cf.mesh(real)
    nf = f.shape[0]
    for k in KS:
        full = part = none = fin_total = 0
        for name in SET_NAMES:
            pts = point_sets(real, k)[name]
            _, counts = _expected(real, name, k, True)
            with np.errstate(invalid="ignore"):
                fin = np.isfinite(pts["max_dist"]) & (pts["max_dist"] > 0) & np.isfinite(pts["p"]).all(axis=1)
            fin_total += int(fin.sum())
            full += int((counts[fin] == k).sum())
            part += int(((counts[fin] > 0) & (counts[fin] < k)).sum())
            none += int((counts[fin] == 0).sum())
            assert (counts[~searchable(pts)] == 0).all()
        assert full >= fin_total / 10.0, "K = %d: only %d of %d finite-radius points have count == K" % (k, full, fin_total)
        if k >= 2:
            assert part >= fin_total / 10.0, "K = %d: only %d of %d finite-radius points have 0 < count < K" % (k, part, fin_total)
        else:
            assert none >= fin_total / 10.0, "K = 1: only %d of %d finite-radius points have count == 0" % (none, fin_total)
        for name in SET_NAMES:
            pts = point_sets(real)[name]
            _, counts = _expected(real, name, k, False)
            ok = searchable(pts)
            assert (counts[ok] == min(k, nf)).all() and (counts[~ok] == 0).all(), "K = %d, set %s with +inf" % (k, name)
    for k in (2, 4):
        rows, counts = brute(v, f, point_sets(real)["c"], k + 1)
        tied = int(((counts == k + 1) & (rows[:, k - 1]["dist2"] == rows[:, k]["dist2"])).sum())
        assert tied >= 100, "set c: only %d points have equal dist2 in their keys %d and %d" % (tied, k, k + 1)
    for k in KS:
        for oname, opts in restrictions(real).items():
            changed = total = 0
            for name in ("a", "b"):
                base, _ = _expected(real, name, k, False)
                out, counts = _expected(real, name, k, False, opts)
                assert (counts[searchable(point_sets(real)[name])] == min(k, int(cf.admitted(nf, opts).sum()))).all()
                changed += sum(out[i].tobytes() != base[i].tobytes() for i in range(out.shape[0]))
                total += out.shape[0]
            assert changed >= total / 10.0, "K = %d: %s changes only %d of %d rows of a and b" % (k, oname, changed, total)
    _CHECKED.add(real)


def face_dist2(real, name):
    """[points, faces] dist2 of set `name`'s coordinates, by the EXISTING closest-point brute force (closest_fixture.brute) run once
    per face with prim_ids_range = [f, f + 1) and max_dist = +inf; NaN where that finds nothing (a non-finite coordinate, a NaN
    dist2).  Shares nothing with the K-nearest rule.  All five sets are computed in one pass, once per precision."""
    real = np.dtype(real)
    if real not in _FACE_DIST2:
        v, f = cf.mesh(real)
        names = list(SET_NAMES)
        xyz = np.concatenate([point_sets(real)[k]["p"] for k in names])
        pts = cf.make_points(real, xyz, np.inf)
        d = np.full((xyz.shape[0], f.shape[0]), np.nan, dtype=real)
        for face in range(f.shape[0]):
            out, found = cf.brute(v, f, pts, (face, face + 1, 0xFFFFFFFF))
            hit = found != 0
            assert (out["prim_id"][hit] == face).all()
            d[hit, face] = out["dist2"][hit]
        d.setflags(write=False)
        off = np.cumsum([0] + [point_sets(real)[k].shape[0] for k in names])
        _FACE_DIST2[real] = {k: d[off[i]:off[i + 1]] for i, k in enumerate(names)}
    return _FACE_DIST2[real][name]


def independent_rows(real, name, pts, k, opts=None):
    """(prim ids [n, k] (0xFFFFFFFF past the count), dist2 [n, k] (r2 past the count), counts) of `pts` — set `name`'s coordinates
    under any radii — from face_dist2 and numpy alone: np.lexsort by (dist2, prim_id), cut at r2 and at k, NaN dropped."""
    real = np.dtype(real)
    d = face_dist2(real, name)
    n, nf = d.shape
    assert pts.shape[0] == n and np.array_equal(pts["p"], point_sets(real)[name]["p"], equal_nan=True)
    with np.errstate(invalid="ignore"):
        r2 = pts["max_dist"] * pts["max_dist"]  # (rounded in `real`)
        cand = (d <= r2[:, None]) & (pts["max_dist"] >= 0)[:, None] & cf.admitted(nf, opts)[None, :]
    ids = np.full((n, k), 0xFFFFFFFF, dtype=np.uint32)
    d2 = np.repeat(r2[:, None], k, axis=1).astype(real)
    counts = np.zeros((n,), dtype=np.uint32)
    prim = np.arange(nf, dtype=np.uint32)
    for i in range(n):
        c = np.nonzero(cand[i])[0]
        order = c[np.lexsort((prim[c], d[i, c]))][:k]
        counts[i] = order.shape[0]
        ids[i, :order.shape[0]] = order
        d2[i, :order.shape[0]] = d[i, order]
    return ids, d2, counts


def tiled(real, k, n):
    """n points — the five sets with K's own radii, repeated — and their expected rows and counts."""
    base = np.concatenate([point_sets(real, k)[s] for s in SET_NAMES])
    ref_out = np.concatenate([expected(real, s, k, True)[0] for s in SET_NAMES])
    ref_counts = np.concatenate([expected(real, s, k, True)[1] for s in SET_NAMES])
    reps = -(-n // base.shape[0])
    return np.tile(base, reps)[:n], np.tile(ref_out, (reps, 1))[:n], np.tile(ref_counts, reps)[:n]


def assert_same(out, counts, ref_out, ref_counts, what=""):
    """Byte-identical rows and counts."""
    counts, ref_counts = np.asarray(counts), np.asarray(ref_counts)
    assert counts.dtype == np.uint32 and np.array_equal(counts, ref_counts), "%s: counts differ at %s" % (what, np.nonzero(counts != ref_counts)[0][:8])
    assert out.shape == ref_out.shape, "%s: %s rows against %s" % (what, out.shape, ref_out.shape)
    if out.tobytes() != ref_out.tobytes():
        bad = [i for i in range(out.shape[0]) if out[i].tobytes() != ref_out[i].tobytes()]
        raise AssertionError("%s: %d of %d rows differ, first %s:\n%s\n%s" % (what, len(bad), out.shape[0], bad[:2], out[bad[:2]], ref_out[bad[:2]]))

"""Signed distance test fixture (nrtSignedDistanceBatch*, include/nanort_sdf.h): the CPU model (tests/sdf_model.cc: the header's
normals, brute force over the faces and a plain walk, for GIVEN normals), the header's host form (tests/cpp/sdf_host_shim.cc), the
meshes and points the CPU and the GPU tests share, and an independent reference that shares nothing with the rule: the winding
number (van Oosterom and Strackee) and the pseudonormals, both in numpy longdouble.

Closed classes (outside is the side from which a face runs counter-clockwise): cube (12 faces, sides 12 x 8 x 6), wedge (a thin
tetrahedron, sharpest dihedral under 20 degrees), torus (12 x 8, jittered parameters), torus_fine (40 x 20), cube_grid (the cube
with points on the quarter-integer lattice: they tie between faces and lie exactly in neighbouring planes).  About 4000 points each,
part uniform in twice the box and part in the box; the same coordinates in both precisions (rounded to fp32 first).

Hostile classes, for byte parity only: the closest fixture's `mixed`, a fan of 2000 faces round one vertex, a mesh with an
unreferenced vertex, faces with a repeated index, zero-area faces, an edge shared by three faces, an open sheet."""
import ctypes
import os
import tempfile

import numpy as np

import closest_fixture as cf
from nanort_amd.wire import node_dtype, point_dtype, signed_dtype, suffix

ROOT = cf.ROOT
LD = np.longdouble
CLOSED_NAMES = ("cube", "wedge", "torus", "torus_fine", "cube_grid")
HOSTILE_NAMES = ("mixed", "fan", "unreferenced", "repeated_index", "zero_area", "three_face_edge", "open_sheet")
INSIDE = 0x80000000
_MODEL = None
_SHIM = None
_CLOSED = {}
_HOSTILE = {}
_REF = {}
_p = cf._p


def model_lib():
    """g++ -O2 -ffp-contract=off -fno-fast-math -shared -fPIC tests/sdf_model.cc, once per process."""
    global _MODEL
    if _MODEL is None:
        so = os.path.join(tempfile.mkdtemp(prefix="nrt_sdf_model_"), "libsdf_model.so")
        cf._compile(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-shared", "-fPIC", "-I",
                     os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tests", "sdf_model.cc")])
        L = ctypes.CDLL(so)
        vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        for s in ("f32", "f64"):
            for name, args in (("sdm_normals_", [vp, vp, u32, u32, vp, vp]), ("sdm_brute_", [vp, vp, u32, vp, vp, i32, vp, u64, vp, vp, vp]),
                               ("sdm_walk_", [vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp]), ("sdm_feature_cases_", [vp, u64, vp, vp])):
                getattr(L, name + s).argtypes = args
                getattr(L, name + s).restype = None
        _MODEL = L
    return _MODEL


def shim_lib():
    """tests/cpp/sdf_host_shim.cc over include/nanort.h, compiled WITHOUT the backend, once per process."""
    global _SHIM
    if _SHIM is None:
        so = os.path.join(tempfile.mkdtemp(prefix="nrt_sdf_shim_"), "libsdf_shim.so")
        cf._compile(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-shared", "-fPIC", "-I",
                     os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tests", "cpp", "sdf_host_shim.cc")])
        L = ctypes.CDLL(so)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        for s in ("f32", "f64"):
            getattr(L, "shs_create_" + s).argtypes = [vp, u32, vp, u32]
            getattr(L, "shs_create_" + s).restype = vp
            getattr(L, "shs_normals_" + s).argtypes = [vp, vp, vp, vp]
            getattr(L, "shs_normals_" + s).restype = None
            getattr(L, "shs_signed_" + s).argtypes = [vp, vp, u64, vp, vp, vp]
            getattr(L, "shs_signed_" + s).restype = ctypes.c_int
            getattr(L, "shs_destroy_" + s).argtypes = [vp]
            getattr(L, "shs_destroy_" + s).restype = None
        _SHIM = L
    return _SHIM


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def num_verts(faces):
    """The context's vertex count: the largest index + 1."""
    return int(np.asarray(faces).max()) + 1 if np.asarray(faces).size else 0


def model_normals(verts, faces, nv=None):
    """The header's host builder: (face_normals [nf, 4, 3], vertex_normals [nv, 3]); nv defaults to the largest index + 1."""
    real = verts.dtype
    verts = np.ascontiguousarray(verts)
    faces = np.ascontiguousarray(faces, dtype=np.uint32)
    nv = num_verts(faces) if nv is None else nv
    fn = np.zeros((faces.shape[0], 4, 3), dtype=real)
    vn = np.zeros((nv, 3), dtype=real)
    getattr(model_lib(), "sdm_normals_" + suffix(real))(_p(verts), _p(faces), faces.shape[0], nv, _p(fn), _p(vn))
    return fn, vn


def brute(verts, faces, normals, pts, opts=None, face_normal_only=False):
    """The model's brute force with the given (face_normals, vertex_normals): (records, found)."""
    real = verts.dtype
    verts = np.ascontiguousarray(verts)
    faces = np.ascontiguousarray(faces, dtype=np.uint32)
    fn, vn = (np.ascontiguousarray(a, dtype=real) for a in normals)
    assert fn.shape == (faces.shape[0], 4, 3) and vn.shape[0] >= num_verts(faces)
    pts = np.ascontiguousarray(pts, dtype=point_dtype(real))
    n = pts.shape[0]
    out = np.zeros((n,), dtype=signed_dtype(real))
    found = np.zeros((n,), dtype=np.uint8)
    getattr(model_lib(), "sdm_brute_" + suffix(real))(_p(verts), _p(faces), faces.shape[0], _p(fn), _p(vn), int(face_normal_only), _p(pts), n,
                                                      _p(cf._opt3(opts)), _p(out), _p(found))
    return out, found


def walk(nodes, indices, verts, faces, normals, pts, opts=None):
    """The model's walk over the given tree: (records, found)."""
    real = verts.dtype
    nodes = np.ascontiguousarray(nodes, dtype=node_dtype(real))
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    verts = np.ascontiguousarray(verts)
    faces = np.ascontiguousarray(faces, dtype=np.uint32)
    fn, vn = (np.ascontiguousarray(a, dtype=real) for a in normals)
    pts = np.ascontiguousarray(pts, dtype=point_dtype(real))
    n = pts.shape[0]
    out = np.zeros((n,), dtype=signed_dtype(real))
    found = np.zeros((n,), dtype=np.uint8)
    getattr(model_lib(), "sdm_walk_" + suffix(real))(_p(nodes), _p(indices), _p(verts), _p(faces), _p(fn), _p(vn), _p(pts), n, _p(cf._opt3(opts)),
                                                     _p(out), _p(found))
    return out, found


def feature_cases(real, cases):
    """cases [n, 12] = p, a, b, c: ([n, 6] u, v, q, dist2 of ClosestFeatureOnTriangle, the same of ClosestPointOnTriangle, codes [n])."""
    cases = np.ascontiguousarray(cases, dtype=real)
    out = np.zeros((cases.shape[0], 12), dtype=real)
    codes = np.zeros((cases.shape[0],), dtype=np.uint32)
    getattr(model_lib(), "sdm_feature_cases_" + suffix(real))(_p(cases), cases.shape[0], _p(out), _p(codes))
    return out[:, :6], out[:, 6:], codes


class HostAccel:
    """include/nanort.h's BVHAccel<T> and FeatureNormals<T> over a TriangleMesh, on the host without the backend."""

    def __init__(self, verts, faces):
        self.real = verts.dtype
        self.s = suffix(self.real)
        self.L = shim_lib()
        verts = np.ascontiguousarray(verts)
        faces = np.ascontiguousarray(faces, dtype=np.uint32)
        self.h = getattr(self.L, "shs_create_" + self.s)(_p(verts), verts.shape[0], _p(faces), faces.shape[0])
        assert self.h, "the header's host Build failed"

    def __del__(self):
        if getattr(self, "h", None):
            getattr(self.L, "shs_destroy_" + self.s)(self.h)
            self.h = None

    def normals(self):
        sz = np.zeros((2,), dtype=np.uint64)
        getattr(self.L, "shs_normals_" + self.s)(self.h, _p(sz), None, None)
        fn = np.zeros((int(sz[0]), 4, 3), dtype=self.real)
        vn = np.zeros((int(sz[1]), 3), dtype=self.real)
        getattr(self.L, "shs_normals_" + self.s)(self.h, _p(sz), _p(fn), _p(vn))
        return fn, vn

    def signed(self, pts, opts=None):
        pts = np.ascontiguousarray(pts, dtype=point_dtype(self.real))
        n = pts.shape[0]
        out = np.zeros((n,), dtype=signed_dtype(self.real))
        found = np.zeros((n,), dtype=np.uint8)
        assert getattr(self.L, "shs_signed_" + self.s)(self.h, _p(pts), n, _p(cf._opt3(opts)), _p(out), _p(found)) == 0
        return out, found


def inside_bits(records):
    return (records["feature"] & INSIDE) != 0


def codes(records):
    return records["feature"] & 7


def assert_word_is_clean(records, found):
    """Bits 0..2 a code 0..6, bit 31 the sign, every other bit 0; a record that found nothing has feature 0."""
    w = records["feature"]
    assert ((w & ~np.uint32(INSIDE | 7)) == 0).all() and ((w & 7) <= 6).all()
    assert (w[np.asarray(found) == 0] == 0).all()


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def _orient_outward_convex(v, f):
    """Faces of a convex solid turned so that a, b, c run counter-clockwise seen from outside."""
    c = v.mean(axis=0)
    f = f.copy()
    for k in range(f.shape[0]):
        a, b, d = v[f[k]]
        if np.dot(np.cross(b - a, d - a), (a + b + d) / 3 - c) < 0:
            f[k, 1], f[k, 2] = f[k, 2], f[k, 1]
    return f


def _cube():
    h = np.array([6.0, 4.0, 3.0])
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64) * h
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.uint32)
    return v, _orient_outward_convex(v, f)


def _wedge():
    v = np.array([[0.0, 0.0, 0.0], [1.1, 0.1, 0.0], [0.5, 1.0, 0.12], [0.6, 0.9, -0.1]])
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], dtype=np.uint32)
    return v, _orient_outward_convex(v, f)


def _torus(nu, nv, jitter, seed):
    rng = np.random.default_rng(seed)
    R, r = 1.0, 0.4
    uu = (np.arange(nu)[:, None] + jitter * rng.uniform(-0.3, 0.3, size=(nu, nv))) * (2 * np.pi / nu)
    vv = (np.arange(nv)[None, :] + jitter * rng.uniform(-0.3, 0.3, size=(nu, nv))) * (2 * np.pi / nv)
    x = (R + r * np.cos(vv)) * np.cos(uu)
    y = (R + r * np.cos(vv)) * np.sin(uu)
    z = r * np.sin(vv)
    v = np.stack([x, y, z], axis=-1).reshape(nu * nv, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            f += [(a, b, c), (a, c, d)]
    return v, np.array(f, dtype=np.uint32)


def _closed_geometry(name):
    """(verts float64, faces, xyz float64) of one closed class."""
    rng = np.random.default_rng(20261022 + 31 * CLOSED_NAMES.index(name))
    if name in ("cube", "cube_grid"):
        v, f = _cube()
    elif name == "wedge":
        v, f = _wedge()
    else:
        v, f = _torus(12, 8, 1.0, 7) if name == "torus" else _torus(40, 20, 0.0, 8)
    bmin, bmax = v.min(0), v.max(0)
    c, h = 0.5 * (bmin + bmax), 0.5 * (bmax - bmin)
    if name == "cube_grid":  # quarter-integer lattice: 3600 points in twice the box, 400 strictly inside it
        q = np.round(h * 4).astype(np.int64)
        wide = np.stack([rng.integers(-2 * q[k], 2 * q[k] + 1, size=3600) for k in range(3)], axis=1)
        inner = np.stack([rng.integers(-q[k] + 1, q[k], size=400) for k in range(3)], axis=1)
        xyz = np.concatenate([wide, inner]) / 4.0
    else:
        xyz = np.concatenate([rng.uniform(c - 2 * h, c + 2 * h, size=(1603, 3)), rng.uniform(c - h, c + h, size=(2400, 3))])
    return v, f, xyz[rng.permutation(xyz.shape[0])]


def closed_classes(real):
    """{name: (verts, faces, points)} in `real`, max_dist = +inf for every point.  Computed once; do not write."""
    real = np.dtype(real)
    if real not in _CLOSED:
        d = {}
        for name in CLOSED_NAMES:
            v, f, xyz = _closed_geometry(name)
            v = np.ascontiguousarray(v.astype(np.float32).astype(real))
            pts = cf.make_points(real, xyz.astype(np.float32).astype(real), np.inf)
            assert pts.shape[0] % 64 != 0
            for a in (v, f, pts):
                a.setflags(write=False)
            d[name] = (v, f, pts)
        _CLOSED[real] = d
    return _CLOSED[real]


def hostile_classes(real):
    """{name: (verts, faces, points)} in `real`: small meshes outside the sign's guarantee.  Computed once; do not write."""
    real = np.dtype(real)
    if real in _HOSTILE:
        return _HOSTILE[real]
    rng = np.random.default_rng(99)
    d = {}
    v, f, pts = cf.hostile_classes(real)["mixed"]
    d["mixed"] = (v, f, pts[:1501])
    # a fan of 2000 faces round vertex 0: its run of corners is longer than a block
    n = 2000
    ang = np.arange(n + 1) * (1.9 * np.pi / n)
    rim = np.stack([np.cos(ang), np.sin(ang), 0.2 * np.sin(5 * ang)], axis=1)
    fv = np.concatenate([[[0.0, 0.0, 0.5]], rim])
    ff = np.stack([np.zeros(n, dtype=np.int64), 1 + np.arange(n), 2 + np.arange(n)], axis=1)
    d["fan"] = (fv, ff, rng.uniform(-1.5, 1.5, size=(1001, 3)))
    cv, cfaces = _cube()
    box = lambda k: rng.uniform(-9.0, 9.0, size=(k, 3))
    # vertex 3 of 11 is named by no face (and the last one is the largest index, so the vertex count still covers it)
    uv = np.concatenate([cv[:3], [[100.0, 100.0, 100.0]], cv[3:], [[0.0, 0.0, 20.0]], [[1.0, 0.0, 20.0]], [[0.0, 1.0, 20.0]]])
    uf = np.where(cfaces >= 3, cfaces + 1, cfaces)
    d["unreferenced"] = (uv, np.concatenate([uf, [[9, 10, 11]]]), box(777))
    rf = np.concatenate([cfaces, [[0, 0, 5], [3, 6, 3], [2, 7, 7], [4, 4, 4]]])
    d["repeated_index"] = (cv, rf, box(777))
    zv = np.concatenate([cv, [0.5 * (cv[0] + cv[7])], [cv[1] + 2.0 * (cv[6] - cv[1])]])  # 8: on the diagonal 0-7; 9: on the line 1-6 beyond 6
    zf = np.concatenate([cfaces, [[0, 8, 7], [1, 6, 9], [2, 2, 5]]])
    d["zero_area"] = (zv, zf, box(777))
    tv = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [-0.5, 0.9, 0.1], [-0.6, -0.8, -0.1]])
    tf = np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]])  # the edge 0-1 in three faces
    d["three_face_edge"] = (tv, tf, rng.uniform(-1.5, 1.5, size=(777, 3)))
    g = 9
    gx, gy = np.meshgrid(np.arange(g), np.arange(g), indexing="ij")
    sv = np.stack([gx.ravel() / 4.0, gy.ravel() / 4.0, 0.1 * np.sin(gx.ravel() * 0.9) * np.cos(gy.ravel() * 0.7)], axis=1)
    sf = []
    for i in range(g - 1):
        for j in range(g - 1):
            a, b, c, e = i * g + j, (i + 1) * g + j, (i + 1) * g + j + 1, i * g + j + 1
            sf += [(a, b, c), (a, c, e)]
    sp = rng.uniform([-0.5, -0.5, -1.0], [2.5, 2.5, 1.0], size=(777, 3))
    sp[::5] = np.round(sp[::5] * 4) / 4
    d["open_sheet"] = (sv, np.array(sf), sp)
    for name in HOSTILE_NAMES[1:]:
        v, f, xyz = d[name]
        md = np.full((xyz.shape[0],), np.inf)
        md[1::4] = 0.7  # a finite radius for a quarter of the points
        d[name] = (np.ascontiguousarray(np.asarray(v).astype(np.float32).astype(real)), np.ascontiguousarray(f, dtype=np.uint32),
                   cf.make_points(real, np.asarray(xyz).astype(np.float32).astype(real), md))
    for name in HOSTILE_NAMES:
        for a in d[name]:
            a.setflags(write=False)
        assert num_verts(d[name][1]) == d[name][0].shape[0]
    _HOSTILE[real] = d
    return d


# ---- the independent reference -----------------------------------------------------------------------------------------------------
def winding_number(verts, faces, xyz):
    """The winding number of the mesh about each point (van Oosterom and Strackee's solid angle per face), np.longdouble."""
    assert cf.reference_available()
    v = np.asarray(verts).astype(LD)
    f = np.asarray(faces, dtype=np.int64)
    p = np.asarray(xyz).astype(LD).reshape(-1, 3)
    out = np.zeros((p.shape[0],), dtype=LD)
    for i in range(0, p.shape[0], 512):
        q = p[i:i + 512, None, :]
        a, b, c = v[f[:, 0]][None] - q, v[f[:, 1]][None] - q, v[f[:, 2]][None] - q
        la, lb, lc = (np.sqrt((x * x).sum(-1)) for x in (a, b, c))
        det = (a * np.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[i:i + 512] = (2 * np.arctan2(det, den)).sum(axis=1) / (4 * LD(np.pi))
    return out


def reference_normals(verts, faces):
    """The pseudonormals in np.longdouble, formulated apart from the header: (face_normals [nf, 4, 3], vertex_normals [nv, 3],
    weight of every face normal entry [nf, 4] = number of faces summed, weight of every vertex [nv] = sum of its corner angles)."""
    assert cf.reference_available()
    v = np.asarray(verts).astype(LD)
    f = np.asarray(faces, dtype=np.int64)
    nf, nv = f.shape[0], num_verts(f)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    x = cf._cross(b - a, c - a)
    ln = np.sqrt((x * x).sum(-1))
    unit = np.where((ln > 0)[:, None], x / np.where(ln > 0, ln, LD(1))[:, None], LD(0))

    def angle(e1, e2):
        y = cf._cross(e1, e2)
        return np.arctan2(np.sqrt((y * y).sum(-1)), (e1 * e2).sum(-1))

    ang = np.stack([angle(b - a, c - a), angle(c - b, a - b), angle(a - c, b - c)], axis=1)
    vn = np.zeros((nv, 3), dtype=LD)
    vw = np.zeros((nv,), dtype=LD)
    for k in range(3):
        np.add.at(vn, f[:, k], ang[:, k, None] * unit)
        np.add.at(vw, f[:, k], ang[:, k])
    fn = np.zeros((nf, 4, 3), dtype=LD)
    fw = np.ones((nf, 4), dtype=LD)
    fn[:, 0] = unit
    holds = [set(map(int, row)) for row in f]
    by_vertex = {}
    for g in range(nf):
        for i in holds[g]:
            by_vertex.setdefault(i, []).append(g)
    for g in range(nf):
        for e, (s0, s1) in enumerate(((0, 1), (0, 2), (1, 2)), start=1):
            i, j = int(f[g, s0]), int(f[g, s1])
            share = [t for t in by_vertex[i] if j in holds[t]]
            fn[g, e] = unit[share].sum(axis=0)
            fw[g, e] = len(share)
    return fn, vn, fw, vw


def normals_error(real, normals, ref):
    """The largest |n_T - n_ref| (infinity norm) in units of eps(T) x the entry's weight, over (face and edge normals, vertex normals)."""
    fn, vn = normals
    rfn, rvn, fw, vw = ref
    eps = LD(np.finfo(real).eps)
    ef = np.abs(fn.astype(LD) - rfn).max(axis=-1) / (eps * np.maximum(fw, LD(1)))
    ev = np.abs(vn.astype(LD) - rvn).max(axis=-1)[vw > 0] / (eps * vw[vw > 0])
    return float(ef.max()), float(ev.max())


# Measured on the closed classes with the model's normals (tests/test_sdf_model.py prints them): the largest error of a face or
# edge normal in eps(T) per face summed, and of a vertex normal in eps(T) x the sum of its corner angles.  The asserted bound is
# eight times the measured value, the project's convention.
MEASURED_FACE_NORMAL_ERROR = {"f32": 1.21, "f64": 1.10}    # (torus; torus_fine)
MEASURED_VERTEX_NORMAL_ERROR = {"f32": 1.05, "f64": 1.19}  # (torus_fine in both)


def closed_reference(name):
    """Of one closed class, from the reference alone (once; do not write): {"inside": winding number above 1/2, "dist": the
    long-double distance to the surface, "face_sign_inside" (wedge only): the side by the plain face normal of the nearest face (smallest id
    among the nearest), "normals": reference_normals}.  The coordinates are the fp32-rounded ones both precisions share."""
    if name in _REF:
        return _REF[name]
    v, f, pts = closed_classes(np.float32)[name]
    xyz = pts["p"]
    w = winding_number(v, f, xyz)
    inside = w > LD(0.5)
    assert (np.abs(w - np.round(w)) < 1e-6).sum() >= 0.9 * w.shape[0], "class %s: the mesh is not closed" % name
    dist = cf.reference_distance(v, f, xyz)
    face_inside = None
    if name == "wedge":  # the side the nearest face's own plane puts the point on (what a shortcut implementation would answer)
        vl, pl = v.astype(LD), xyz.astype(LD)
        fi = f.astype(np.int64)
        a, b, c = vl[fi[:, 0]], vl[fi[:, 1]], vl[fi[:, 2]]
        nrm = cf._cross(b - a, c - a)
        d = cf._reference_pairs(pl[:, None, :], a[None], b[None], c[None])
        near = d <= d.min(axis=1, keepdims=True) * (1 + LD(1e-12))
        first = near.argmax(axis=1)  # (the smallest id among the nearest)
        face_inside = ((pl - a[first]) * nrm[first]).sum(-1) < 0
    ref = {"inside": inside, "dist": dist, "face_sign_inside": face_inside, "normals": reference_normals(v, f)}
    _check_closed(name, v, f, pts, ref)
    _REF[name] = ref
    return ref


def checked(real, name):
    """Which points of closed class `name` the sign is compared on: those farther than tol = 8 eps(T) S from the surface."""
    v, _, pts = closed_classes(real)[name]
    tol = cf.tolerance(real, v, pts["p"])
    ok = closed_reference(name)["dist"] > tol
    assert (~ok).sum() <= 0.05 * ok.shape[0], "class %s: %d of %d points lie within the tolerance of the surface" % (name, (~ok).sum(), ok.shape[0])
    return ok


def _check_closed(name, v, f, pts, ref):
    """What the classes must exercise, from the reference alone."""
    n = pts.shape[0]
    assert 3900 <= n <= 4100
    assert ref["inside"].sum() >= n / 10.0 and (~ref["inside"]).sum() >= n / 10.0, "class %s: %d of %d points inside" % (name, ref["inside"].sum(), n)
    # the convention: a point known to be INSIDE by construction (the centroid of a convex solid, the middle of the tube) has winding number +1
    known_inside = np.asarray([[1.0, 0.0, 0.0]]) if name.startswith("torus") else v.astype(np.float64).mean(axis=0)[None]
    assert abs(float(winding_number(v, f, known_inside)[0]) - 1.0) < 1e-9
    if name == "wedge":
        fn = ref["normals"][0][:, 0].astype(np.float64)
        dihedral = [np.degrees(np.pi - np.arccos(np.clip(np.dot(fn[i], fn[j]), -1, 1))) for i in range(4) for j in range(i + 1, 4)]
        assert min(dihedral) < 20.0, dihedral
        far = ref["dist"] > cf.tolerance(np.float32, v, pts["p"])
        wrong = (ref["face_sign_inside"] != ref["inside"]) & far
        assert wrong.sum() >= far.sum() / 10.0, "wedge: the face normal alone is wrong for only %d of %d points" % (wrong.sum(), far.sum())

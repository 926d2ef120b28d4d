"""Curve-primitive test fixture (nrtSetCurves_f32 / nrtTraverseBatchCurves*_f32): the CPU model (tests/curves_model.c), the live
reference (tests/ref_curves_shim.cc over the unmodified examples/curves_primitive/main.cc, where the reference tree exists),
the scenes, the rays and the list of cases the CPU and the GPU tests share."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from nanort_amd import scenes
from nanort_amd.wire import CURVE_HIT_F32, NODE_F32, RAY_F32
import sphere_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
# the example's thickness argument (its argv[1]; main.cc:852-856).  At its default, 0.01, the 400 strands are 0.02 wide under a
# 64 x 64 grid whose rays are 0.3 apart at the ball: 363 of 4096 rays hit.  At 0.05 it is 1099, with every quarter of u met.
FUR_THICKNESS = 0.05
_MODEL = None
_REF = None


def _compile(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def model_lib():
    """gcc -O2 -ffp-contract=off -fno-fast-math -shared -fPIC tests/curves_model.c, once per process."""
    global _MODEL
    if _MODEL is None:
        so = os.path.join(tempfile.mkdtemp(prefix="nrt_curves_model_"), "libcurves_model.so")
        _compile(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-o", so,
                  os.path.join(ROOT, "tests", "curves_model.c"), "-lm"])
        L = ctypes.CDLL(so)
        vp = ctypes.c_void_p
        L.cvm_traverse.argtypes = [vp, vp, vp, vp, ctypes.c_int, vp, ctypes.c_uint64, vp, vp, vp]
        L.cvm_traverse.restype = None
        L.cvm_boxes.argtypes = [vp, vp, ctypes.c_uint32, vp, vp, vp]
        L.cvm_boxes.restype = None
        _MODEL = L
    return _MODEL


def have_reference():
    return os.path.exists(os.path.join(REFERENCE, "examples", "curves_primitive", "main.cc"))


def ref_lib(out_dir=None):
    """The live reference: tests/ref_curves_shim.cc compiled against the reference tree (contraction off), once per process."""
    global _REF
    if _REF is None or out_dir is not None:
        so = os.path.join(out_dir or tempfile.mkdtemp(prefix="nrt_curves_ref_"), "libcurves_ref.so")
        _compile(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-w", "-I", REFERENCE,
                  "-I", os.path.join(REFERENCE, "examples", "common"), "-I", os.path.join(REFERENCE, "examples", "curves_primitive"),
                  "-o", so, os.path.join(ROOT, "tests", "ref_curves_shim.cc")])
        _REF = load_ref(so)
    return _REF


def load_ref(so):
    L = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.refcv_fur.argtypes = [vp, vp, u32, ctypes.c_float]
    L.refcv_fur.restype = u32
    L.refcv_build.argtypes = [vp, vp, u32, u32, ctypes.POINTER(u32)]
    L.refcv_build.restype = vp
    L.refcv_get_tree.argtypes = [vp, vp, vp]
    L.refcv_get_tree.restype = None
    L.refcv_destroy.argtypes = [vp]
    L.refcv_destroy.restype = None
    L.refcv_traverse.argtypes = [vp, vp, ctypes.c_uint64, u32, u32, ctypes.c_int, vp, vp]
    L.refcv_traverse.restype = ctypes.c_double
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def model_traverse(nodes, indices, cps, radii, rays, num_subdivisions=4, range_=None):
    nodes = np.ascontiguousarray(nodes, dtype=NODE_F32)
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    cps = np.ascontiguousarray(cps, dtype=np.float32)
    radii = np.ascontiguousarray(radii, dtype=np.float32)
    rays = np.ascontiguousarray(rays, dtype=RAY_F32)
    hits = np.zeros(rays.shape[0], dtype=CURVE_HIT_F32)
    mask = np.zeros(rays.shape[0], dtype=np.uint8)
    rg = None if range_ is None else np.asarray(range_, dtype=np.uint32)
    model_lib().cvm_traverse(_p(nodes), _p(indices), _p(cps), _p(radii), int(num_subdivisions), _p(rays), rays.shape[0],
                             None if rg is None else _p(rg), _p(hits), _p(mask))
    return hits, mask


def model_boxes(cps, radii):
    cps = np.ascontiguousarray(cps, dtype=np.float32)
    radii = np.ascontiguousarray(radii, dtype=np.float32)
    n = radii.shape[0]
    out = [np.zeros((n, 3), dtype=np.float32) for _ in range(3)]
    model_lib().cvm_boxes(_p(cps), _p(radii), n, _p(out[0]), _p(out[1]), _p(out[2]))
    return out


class RefAccel:
    """The example's CurveGeometry / CurvePred under the reference's Build, and its CurveIntersector under Traverse."""

    def __init__(self, cps, radii, min_leaf=0, lib=None):
        self.L = lib or ref_lib()
        self.cps = np.ascontiguousarray(cps, dtype=np.float32)
        self.radii = np.ascontiguousarray(radii, dtype=np.float32)
        nn = ctypes.c_uint32(0)
        self.h = self.L.refcv_build(_p(self.cps), _p(self.radii), self.radii.shape[0], int(min_leaf), ctypes.byref(nn))
        assert self.h, "the reference's Build() failed"
        self.nodes = np.zeros(nn.value, dtype=NODE_F32)
        self.indices = np.zeros(self.radii.shape[0], dtype=np.uint32)
        self.L.refcv_get_tree(self.h, _p(self.nodes), _p(self.indices))
        self.last_secs = 0.0

    def traverse(self, rays, num_subdivisions=4, range_=None):
        rays = np.ascontiguousarray(rays, dtype=RAY_F32)
        hits = np.zeros(rays.shape[0], dtype=CURVE_HIT_F32)
        mask = np.zeros(rays.shape[0], dtype=np.uint8)
        r0, r1 = (0, 0x7FFFFFFF) if range_ is None else range_
        self.last_secs = self.L.refcv_traverse(self.h, _p(rays), rays.shape[0], int(r0), int(r1), int(num_subdivisions), _p(hits), _p(mask))
        return hits, mask

    def close(self):
        if self.h:
            self.L.refcv_destroy(self.h)
            self.h = None


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def fur():
    """The example's own 400-curve scene, as the example wrote it (tests/golden/curves_fur.npz): control points (400, 4, 3),
    radii (400, 4)."""
    g = np.load(os.path.join(GOLDEN, "curves_fur.npz"))
    return g["cps"], g["radii"]


def fur_golden():
    return np.load(os.path.join(GOLDEN, "curves_fur.npz"))


def hair(n):
    """Synthetic hair sized for the example's camera: thick enough that a 64 x 64 grid of rays meets it."""
    return scenes.synthetic_hair(n, seed=7 + n, thickness=0.12)


def degenerate():
    """Twelve strands of hair() with: all four control points equal; radius 0; a NaN control point; a curve behind the origin of
    the camera rays; a zero-length first segment; unequal end radii."""
    cps, radii = hair(12)
    cps, radii = cps.copy(), radii.copy()
    cps[0, :] = cps[0, 0]
    radii[1] = 0.0
    cps[2, 2, 1] = np.nan
    cps[3] += np.float32(40.0) * np.array([0, 0, 1], dtype=np.float32)  # z ~ 44: behind the eye at z = 20
    cps[4, 1] = cps[4, 0]
    radii[5] = (0.3, 0.2, 0.1, 0.01)
    return cps, radii


def scene(name):
    if name == "fur":
        return fur()
    if name == "degenerate":
        return degenerate()
    return hair(int(name))


# ---- rays -------------------------------------------------------------------------------------------------------------------
def camera(w=64, h=64):
    return scenes.curves_camera_rays(w, h)


def hostile_rays():
    """sphere_fixture.hostile_rays() moved to the curve camera's scale, plus what the curve intersector branches on: directions
    (0, +-1, 0) (GetZAlign's dxz == 0 branch), zero directions, max_t = inf, NaN origins, short max_t."""
    r = sphere_fixture.hostile_rays()[::4].copy()
    r["org"] *= np.float32(5.0)
    n = 64
    e = np.zeros(n, dtype=RAY_F32)
    rng = np.random.default_rng(99)
    e["org"] = rng.uniform(-6.0, 6.0, size=(n, 3)).astype(np.float32)
    e["dir"] = rng.normal(size=(n, 3)).astype(np.float32)
    e["min_t"], e["max_t"] = 0.0, 1.0e30
    # Along +-y the example's frame has its z axis AGAINST the ray (GetZAlign's else branch: z' = -+(y - org.y)), so such a ray
    # meets what lies behind its origin: half of these start 3 beyond a control point of hair(3000) and look away from it (they
    # hit), half start 3 before it and look at it (they see it at z' = -3, and reject it).
    e["dir"][:16] = (0.0, 1.0, 0.0)
    e["dir"][16:32] = (0.0, -1.0, 0.0)
    target = hair(3000)[0][np.arange(32) * 90, 1]
    side = np.where(np.arange(32) % 4 == 3, -3.0, 3.0) * np.where(np.arange(32) < 16, 1.0, -1.0)
    e["org"][:32] = target
    e["org"][:32, 1] += side.astype(np.float32)
    e["dir"][32:36] = 0.0
    e["max_t"][36:44] = np.inf
    e["org"][44:48, 0] = np.nan
    e["max_t"][48:52] = 3.0
    return np.concatenate([r, e])


def all_rays():
    return np.concatenate([camera(), hostile_rays()])


# ---- the cases of "model == reference" (CPU) --------------------------------------------------------------------------------
# (name, scene, num_subdivisions, prim_ids_range)
CASES = [("n%s_s%d" % (s, k), s, k, None) for s in ("1", "2", "5", "64", "fur", "3000") for k in (4, 7)]
CASES += [("n3000_s4_range", "3000", 4, (500, 2500)), ("degenerate_s4", "degenerate", 4, None), ("degenerate_s7", "degenerate", 7, None)]


def write_fur_golden():
    """(needs the reference tree; `PYTHONPATH=.:tests python tests/curves_fixture.py`) tests/golden/curves_fur.npz: the scene the example writes at FUR_THICKNESS, the tree the
    reference builds over it and the reference's records for camera(), num_subdivisions = 4."""
    L = ref_lib()
    cps, radii = np.zeros((400, 4, 3), np.float32), np.zeros((400, 4), np.float32)
    assert L.refcv_fur(_p(cps), _p(radii), 400, FUR_THICKNESS) == 400
    a = RefAccel(cps, radii)
    hits, mask = a.traverse(camera())
    tree = a.nodes.copy()
    tree["axis"][tree["flag"] == 1] = 0  # (the reference never writes a leaf's axis)
    np.savez_compressed(os.path.join(GOLDEN, "curves_fur.npz"), cps=cps, radii=radii, nodes=tree, indices=a.indices, hits=hits, mask=mask)
    a.close()


if __name__ == "__main__":
    write_fur_golden()

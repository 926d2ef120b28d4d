"""tools/occluded_kinds_probe.py <libnanort_hip.so> <label> <out.json>: what DESIGN.md 3.4c reports.  For 1 M spheres and the cylinder
example's 20 000 needles under the 1920 x 1080 particle camera, and the curve example's fur under its camera at 1024 x 1024, rays
resident in HBM: the kind's closest-hit Device call and, where the library exports it, nrtOccludedBatchPrimsDevice_f32 over the same
rays — 3 warm-up launches, then 20 timed by nrtLastTraverseMs (median, min, max), the two masks compared.  The library is a
command-line argument so that two builds (the commit before, this one) can be run alternately, one process each."""
import ctypes, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from nanort_amd import scenes
import curves_fixture as cf

lib, label, out = sys.argv[1:4]
L = ctypes.CDLL(lib, mode=ctypes.RTLD_GLOBAL)
vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
L.nrtCreate.argtypes = [i32, ctypes.POINTER(vp)]
L.nrtDestroy.argtypes = [vp]; L.nrtDestroy.restype = None
L.nrtLastError.argtypes = [vp]; L.nrtLastError.restype = ctypes.c_char_p
L.nrtLastTraverseMs.argtypes = [vp]; L.nrtLastTraverseMs.restype = ctypes.c_float
L.nrtLastKernelName.argtypes = [vp]; L.nrtLastKernelName.restype = ctypes.c_char_p
L.nrtBuild_f32.argtypes = [vp, vp, vp, ctypes.POINTER(u64)]
L.nrtSetSpheres_f32.argtypes = [vp, vp, vp, u32]
L.nrtSetCylinders_f32.argtypes = [vp, vp, vp, u32, i32]
L.nrtSetCurves_f32.argtypes = [vp, vp, vp, u32, u32]
for nm in ("nrtTraverseBatchDevice_f32", "nrtTraverseBatchCylindersDevice_f32", "nrtTraverseBatchCurvesDevice_f32"):
    getattr(L, nm).argtypes = [vp, vp, u64, vp, vp, vp, vp]
has_prims = hasattr(L, "nrtOccludedBatchPrimsDevice_f32")
if has_prims:
    L.nrtOccludedBatchPrimsDevice_f32.argtypes = [vp, vp, u64, vp, vp, vp]
p = lambda a: a.ctypes.data_as(vp)

def ck(c, st):
    assert st == 0, (st, L.nrtLastError(c))

def series(c, launch):
    for _ in range(3):
        ck(c, launch()); torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        ck(c, launch()); torch.cuda.synchronize()
        ts.append(float(L.nrtLastTraverseMs(c)))
    return {"median_ms": float(np.median(ts)), "min_ms": min(ts), "max_ms": max(ts), "kernel": L.nrtLastKernelName(c).decode()}

res = {"label": label, "rows": {}}
W, H = 1920, 1080
work = []
c_, r_ = scenes.random_spheres(1000000)
work.append(("spheres_1m", lambda c: L.nrtSetSpheres_f32(c, p(c_), p(r_), 1000000), scenes.particle_camera_rays(W, H), 16, "nrtTraverseBatchDevice_f32"))
v_, cr_ = scenes.random_cylinders(20000)
work.append(("cylinders_20k", lambda c: L.nrtSetCylinders_f32(c, p(v_), p(cr_), 20000, 1), scenes.particle_camera_rays(W, H), 28, "nrtTraverseBatchCylindersDevice_f32"))
cps, rad = cf.fur()
cps, rad = np.ascontiguousarray(cps, np.float32), np.ascontiguousarray(rad, np.float32)
work.append(("fur_1024", lambda c: L.nrtSetCurves_f32(c, p(cps), p(rad), rad.shape[0], 4), cf.camera(1024, 1024), 40, "nrtTraverseBatchCurvesDevice_f32"))
for name, setter, rays, hsz, closest in work:
    c = vp()
    assert L.nrtCreate(0, ctypes.byref(c)) == 0
    ck(c, setter(c))
    nn = u64(0)
    ck(c, L.nrtBuild_f32(c, None, None, ctypes.byref(nn)))
    n = rays.shape[0]
    d_r = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1)).cuda()
    d_h = torch.empty(n * hsz, dtype=torch.uint8, device="cuda")
    d_m = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_o = torch.empty(n, dtype=torch.uint8, device="cuda")
    row = {"rays": int(n)}
    row["closest"] = series(c, lambda: getattr(L, closest)(c, d_r.data_ptr(), n, None, d_h.data_ptr(), d_m.data_ptr(), None))
    if has_prims:
        row["occluded"] = series(c, lambda: L.nrtOccludedBatchPrimsDevice_f32(c, d_r.data_ptr(), n, None, d_o.data_ptr(), None))
        row["flags_equal"] = bool(torch.equal(d_o, (d_m != 0).to(torch.uint8)))
    row["hit_share"] = float((d_m != 0).float().mean())
    res["rows"][name] = row
    print(label, name, json.dumps(row), flush=True)
    L.nrtDestroy(c)
json.dump(res, open(out, "w"), indent=1)

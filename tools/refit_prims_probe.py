"""tools/refit_prims_probe.py [--out FILE.json]: what DESIGN.md reports about the sphere / curve refit.  For 1 M spheres (the
particle example's scene under its 1920 x 1080 camera) and the curve example's fur (400 curves, its camera at 1024 x 1024), arrays
and rays resident in HBM, after a jitter of the positions by 1 % of the scene's extent:

  refit       device time of nrtRefitPrimsDevice_f32 (events around the call on its stream)
  set+build   device time of nrtSetSpheresDevice_f32 / nrtSetCurvesDevice_f32 (events around the call on its stream) plus
              nrtBuild_f32 (nrtLastBuildMs: events around the build on the context's stream), and the wall time of the pair
  trace       closest-hit ms (nrtLastTraverseMs) on the refit tree against a fresh build over the same jittered arrays

3 warm-up rounds, then the median (min, max) of 20.  Prints one JSON line per row."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import curves_fixture as cf  # noqa: E402
from nanort_amd import BVHAccel, CurveGeometry, SphereGeometry, scenes  # noqa: E402

WARM, RUNS = 3, 20


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def timed(stream, call):
    """Device milliseconds of what `call` enqueues on `stream`, and the wall milliseconds until it has completed."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    t0 = time.perf_counter()
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def trace_ms(a, d_rays, d_hits, d_mask):
    ts = []
    for k in range(WARM + RUNS):
        a.TraverseBatchDevice(d_rays, d_hits, d_mask)
        torch.cuda.synchronize()
        if k >= WARM:
            ts.append(a.LastTraverseMs())
    return stats(ts)


def row(name, geometry, set_device, pos, rad, rays, hit_bytes):
    rng = np.random.default_rng(1)
    ext = float(np.abs(pos).max())
    p1 = (pos + rng.normal(scale=0.01 * ext, size=pos.shape)).astype(np.float32)
    stream = torch.cuda.Stream()
    d_p0, d_p1, d_r = torch.from_numpy(pos).cuda(), torch.from_numpy(p1).cuda(), torch.from_numpy(rad).cuda()
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1)).cuda()
    d_hits = torch.empty(rays.shape[0] * hit_bytes, dtype=torch.uint8, device="cuda")
    d_mask = torch.empty(rays.shape[0], dtype=torch.uint8, device="cuda")
    a = BVHAccel(np.float32)
    assert a.Build(rad.shape[0], geometry(pos, rad))
    out = {"prims": int(rad.shape[0]), "rays": int(rays.shape[0]), "built_trace": trace_ms(a, d_rays, d_hits, d_mask)}
    refit, refit_wall = [], []
    for k in range(WARM + RUNS):  # alternate the two position sets, so that every refit has boxes to change
        dev, wall = timed(stream, lambda: a.RefitPrimsDevice(d_p1 if k % 2 == 0 else d_p0, d_r, stream=stream))
        if k >= WARM:
            refit.append(dev)
            refit_wall.append(wall)
    a.RefitPrimsDevice(d_p1, d_r, stream=stream)
    stream.synchronize()
    out["refit_device"], out["refit_wall"] = stats(refit), stats(refit_wall)
    out["refit_trace"] = trace_ms(a, d_rays, d_hits, d_mask)
    refit_mask = d_mask.clone()
    b = BVHAccel(np.float32)
    set_ms, build_ms, pair_wall = [], [], []
    for k in range(WARM + RUNS):
        t0 = time.perf_counter()
        dev, _ = timed(stream, lambda: set_device(b, d_p1, d_r, stream))
        assert b.BuildCurrent()
        wall = (time.perf_counter() - t0) * 1e3
        if k >= WARM:
            set_ms.append(dev)
            build_ms.append(b.LastBuildMs())
            pair_wall.append(wall)
    out["set_device"], out["build_device"], out["set_build_wall"] = stats(set_ms), stats(build_ms), stats(pair_wall)
    out["set_build_device_median_ms"] = out["set_device"]["median_ms"] + out["build_device"]["median_ms"]
    out["fresh_trace"] = trace_ms(b, d_rays, d_hits, d_mask)
    out["flags_differing"] = int((d_mask != refit_mask).sum())
    out["hit_share"] = float((d_mask != 0).float().mean())
    print(name, json.dumps(out), flush=True)
    a.close()
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--spheres", type=int, default=1000000)
    args = ap.parse_args()
    res = {}
    c, r = scenes.random_spheres(args.spheres)
    res["spheres_%d" % args.spheres] = row("spheres_%d" % args.spheres, SphereGeometry, lambda b, p, rad, s: b.SetSpheresDevice(p, rad, stream=s), c, r,
                                           scenes.particle_camera_rays(1920, 1080), 16)
    cps, rad = cf.fur()
    cps, rad = np.ascontiguousarray(cps, np.float32), np.ascontiguousarray(rad, np.float32)
    res["fur_400"] = row("fur_400", CurveGeometry, lambda b, p, rr, s: b.SetCurvesDevice(p, rr, 4, stream=s), cps, rad, cf.camera(1024, 1024), 40)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()

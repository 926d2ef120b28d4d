"""Refit against rebuild on C3 — Plane(1000, 500), 1 M triangles, fp32, 1920x1080 objrender camera.  Every frame displaces the
plane by a travelling wave (on the device) and refits with nrtRefitDevice_f32.  Reports, as one JSON line:
  * device time of nrtRefitDevice_f32: the first refit (it builds the tree's level plan) and the steady state (median), timed
    with events behind a device-side sleep so that the host's enqueue cost is not counted; the wall time of the call too;
  * nrtRefit_f32 (host vertices, uploaded from pageable memory): wall time;
  * nrtBuild_f32 device time (nrtLastBuildMs) of a fresh build of the same deformed mesh, in the same process;
  * the device's free memory before and after the steady-state frames (a refit allocates nothing);
  * closest-hit Grays/s for the primary rays on the refit tree and on the fresh build (kernel time, median of `reps`).

    python tools/refit_probe.py [--frames 20] [--reps 9]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from nanort_amd import BVHAccel, TriangleMesh, scenes

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    v, f = scenes.plane(1000, 500)
    a = BVHAccel(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    d_v0 = torch.from_numpy(v).cuda()
    ext = float(v[:, 0].max() - v[:, 0].min())
    d_v = torch.empty_like(d_v0)
    s = torch.cuda.Stream()
    out = {"probe": "refit", "mesh": "C3 plane(1000,500)", "tris": int(f.shape[0]), "verts": int(v.shape[0]), "image": "1920x1080",
           "frames": args.frames, "reps": args.reps}

    def deform(t):  # a travelling wave along x, amplitude 2 % of the plane's extent, normal to the plane (z)
        d_v.copy_(d_v0)
        d_v[:, 2] += 0.02 * ext * torch.sin(d_v0[:, 0] * (12.0 / ext) - 0.9 * t)

    def timed_refit(t):
        with torch.cuda.stream(s):
            deform(t)
            torch.cuda._sleep(2_000_000)  # (the refit's launches queue up behind it: the events time the device work alone)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            w0 = time.perf_counter()
            a.RefitDevice(d_v, stream=s)
            wall = (time.perf_counter() - w0) * 1e3
            e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1), wall

    first_ms, first_wall = timed_refit(0.0)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    dev, wall = [], []
    for k in range(1, args.frames + 1):
        d_ms, w_ms = timed_refit(0.1 * k)
        dev.append(d_ms)
        wall.append(w_ms)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    out["refit_device_first_ms"] = first_ms
    out["refit_device_first_wall_ms"] = first_wall
    out["refit_device_steady_ms"] = float(np.median(dev))
    out["refit_device_steady_wall_ms"] = float(np.median(wall))
    out["free_bytes_delta_steady"] = int(free1 - free0)
    vh = d_v.cpu().numpy()  # the last frame's positions
    host = []
    for _ in range(5):
        w0 = time.perf_counter()
        a.Refit(vh)
        host.append((time.perf_counter() - w0) * 1e3)
    out["refit_host_wall_ms"] = float(np.median(host))
    b = BVHAccel(np.float32)
    builds = []
    for _ in range(5):
        assert b.Build(f.shape[0], TriangleMesh(vh, f))
        builds.append(b.LastBuildMs())
    out["build_device_ms"] = float(np.median(builds))
    out["refit_over_build"] = out["refit_device_steady_ms"] / out["build_device_ms"]

    rays = scenes.camera_rays(1920, 1080)
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.empty((n * 16,), dtype=torch.uint8, device="cuda")
    d_mask = torch.empty((n,), dtype=torch.uint8, device="cuda")
    for name, acc in (("refit_tree", a), ("fresh_build", b)):
        acc.SetLaunchTiming(1)
        for _ in range(2):
            acc.TraverseBatchDevice(d_rays, d_hits, d_mask)
        torch.cuda.synchronize()
        t = []
        for _ in range(args.reps):
            acc.TraverseBatchDevice(d_rays, d_hits, d_mask)
            torch.cuda.synchronize()
            t.append(acc.LastTraverseMs())
        ms = float(np.median(t))
        out[name] = {"ms": ms, "grays_s": n / ms / 1e6, "hits": int(d_mask.sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Motion blur on C3 — Plane(1000, 500), 1 M triangles, fp32, 1920x1080 objrender camera; keyframe 1 is keyframe 0 displaced by
the travelling wave of tools/refit_probe.py.  Primaries and their bounce rays, times uniform in [0, 1), everything resident in HBM.
Per ray set, in one process and over the same rays (launches timed by nrtLastTraverseMs: 3 warm-up launches, then the median,
minimum and maximum of 20):
  * the motion walk (nrtTraverseBatchMotionDevice_f32) and its occlusion query;
  * the motion walk on a context whose keyframe 1 == keyframe 0 — what the second record and the interpolation cost by themselves
    (the boxes are the plain ones);
  * on that same plain tree: nrtMultiHitTraverseBatchDevice at K = 1, the literal walk (tunable wide = 0) and the default
    closest-hit walk.
And the builds: motion build ms against plain build ms (nrtLastBuildMs, median of 5).  Writes profiles/motion_probe_c3.json and
prints it as one JSON line.

    python tools/motion_probe.py [--launches 20] [--warmup 3] [--out profiles/motion_probe_c3.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from nanort_amd import BVHAccel, MotionTriangleMesh, TriangleMesh, scenes

    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_probe_c3.json"))
    args = ap.parse_args()

    v0, f = scenes.plane(1000, 500)
    ext = float(v0[:, 0].max() - v0[:, 0].min())
    v1 = v0.copy()  # the wave of tools/refit_probe.py at t = 1: amplitude 2 % of the plane's extent, normal to the plane
    v1[:, 2] += (0.02 * ext * np.sin(v0[:, 0].astype(np.float64) * (12.0 / ext) - 0.9)).astype(np.float32)

    def median_build(mesh):
        a = BVHAccel(np.float32)
        ms = []
        for _ in range(5):
            assert a.Build(f.shape[0], mesh)
            ms.append(a.LastBuildMs())
        return a, float(np.median(ms))

    plain, plain_ms = median_build(TriangleMesh(v0, f))
    same, same_ms = median_build(MotionTriangleMesh(v0, v0.copy(), f))
    moving, moving_ms = median_build(MotionTriangleMesh(v0, v1, f))
    out = {"probe": "motion", "mesh": "C3 plane(1000,500)", "tris": int(f.shape[0]), "image": "%dx%d" % (args.width, args.height),
           "launches": args.launches, "warmup": args.warmup,
           "build_ms": {"plain": plain_ms, "motion_same_keyframes": same_ms, "motion_wave": moving_ms, "motion_over_plain": moving_ms / plain_ms}}

    cam = scenes.camera_rays(args.width, args.height)
    h, m = plain.TraverseBatch(cam)
    bounce = scenes.secondary_rays("bounce", v0, f, cam, h, m)
    rng = np.random.default_rng(1)

    def timed(launch, acc):
        for _ in range(args.warmup):
            launch()
        torch.cuda.synchronize()
        t = []
        for _ in range(args.launches):
            launch()
            t.append(acc.LastTraverseMs())  # (waits for the launch)
        return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}

    out["rays"] = {}
    for name, rays in (("primary", cam), ("bounce", bounce)):
        n = rays.shape[0]
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_times = torch.from_numpy(rng.random(n, dtype=np.float32)).cuda()
        d_hits = torch.empty((n * 16,), dtype=torch.uint8, device="cuda")
        d_mask = torch.empty((n,), dtype=torch.uint8, device="cuda")
        d_cnt = torch.empty((n,), dtype=torch.int32, device="cuda")
        row = {"n": int(n)}
        row["motion"] = timed(lambda: moving.TraverseBatchMotionDevice(d_rays, d_times, d_hits, d_mask), moving)
        row["motion"]["hits"] = int(d_mask.sum())
        row["motion_occluded"] = timed(lambda: moving.OccludedBatchMotionDevice(d_rays, d_times, d_mask), moving)
        row["motion_same_keyframes"] = timed(lambda: same.TraverseBatchMotionDevice(d_rays, d_times, d_hits, d_mask), same)
        row["multihit_k1"] = timed(lambda: plain.MultiHitTraverseBatchDevice(d_rays, 1, d_hits, d_cnt), plain)
        plain.SetTunable("wide", 0)
        row["literal"] = timed(lambda: plain.TraverseBatchDevice(d_rays, d_hits, d_mask), plain)
        assert plain.LastKernelName() == "nrt::k_traverse<float>"
        plain.SetTunable("wide", 1)
        row["default"] = timed(lambda: plain.TraverseBatchDevice(d_rays, d_hits, d_mask), plain)
        row["default"]["kernel"] = plain.LastKernelName()
        row["default"]["hits"] = int(d_mask.sum())
        for k in ("motion", "motion_occluded", "motion_same_keyframes", "multihit_k1", "literal", "default"):
            row[k]["grays_s"] = n / row[k]["median_ms"] / 1e6
        row["motion_over_literal"] = row["motion"]["median_ms"] / row["literal"]["median_ms"]
        row["motion_over_default"] = row["motion"]["median_ms"] / row["default"]["median_ms"]
        row["same_keyframes_over_literal"] = row["motion_same_keyframes"]["median_ms"] / row["literal"]["median_ms"]
        out["rays"][name] = row
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()

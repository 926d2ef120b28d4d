#!/usr/bin/env python3
"""Occlusion against closest hit on instanced scenes: Mrays/s of Scene.OccludedBatchDevice beside Scene.TraverseBatchDevice on the
shadow rays of a primary wave — from the closest hits of a camera wave towards one point light, max_t = the distance to it — on
the 5-node fixture and on the 10 000- and 100 000-instance scenes bench_rows.py builds.  Stand-alone; bench.py does not call it.

Each figure: `--warmup` untimed calls, then `--steps` timed ones (each call is synchronous and ends with the stream drained);
the median and the spread (min .. max) are reported, and the share of rays the single-pass walk handed to the listing path.

    python3 tools/scene_occlusion_probe.py [--width 1920 --height 1080 --steps 7 --warmup 2 --skip-100k] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LIGHT = np.array([2.0, 14.0, 6.0], dtype=np.float32)


def timed(fn, steps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return np.array(ts)


def rate(n, ts):
    r = n / ts / 1e6
    return {"median": round(float(np.median(r)), 1), "min": round(float(r.min()), 1), "max": round(float(r.max()), 1)}


def probe(name, sc, cam, steps, warmup):
    import torch

    from nanort_amd.wire import RAY_F32, SCENE_HIT_F32

    hits, mask = sc.TraverseBatch(cam)
    hit = mask == 1
    d = cam["dir"][hit].astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = cam["org"][hit] + d * hits["t"][hit, None]
    to_light = LIGHT[None, :] - p
    dist = np.linalg.norm(to_light, axis=1).astype(np.float32)
    rays = np.zeros(int(hit.sum()), dtype=RAY_F32)
    rays["dir"] = (to_light / dist[:, None]).astype(np.float32)
    rays["org"] = (p + 1e-3 * rays["dir"]).astype(np.float32)  # off the surface
    rays["min_t"] = 0.0
    rays["max_t"] = dist
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    d_hits = torch.empty(n * SCENE_HIT_F32.itemsize, dtype=torch.uint8, device="cuda")
    d_m0 = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_m1 = torch.empty(n, dtype=torch.uint8, device="cuda")
    t_closest = timed(lambda: sc.TraverseBatchDevice(d_rays, d_hits, d_m0), steps, warmup)
    redo_closest = sc.LastRedone()
    t_occ = timed(lambda: sc.OccludedBatchDevice(d_rays, d_m1), steps, warmup)
    redo_occ, path = sc.LastRedone(), sc.LastPath()
    same = bool(torch.equal(d_m0, d_m1))
    row = {"scene": name, "shadow_rays": n, "occluded_fraction": round(float(d_m1.float().mean().item()), 4),
           "closest_hit_Mrays_s": rate(n, t_closest), "occluded_Mrays_s": rate(n, t_occ),
           "path": "single-pass walk" if path == 1 else "listing path", "redo_share_closest": round(redo_closest / max(n, 1), 5),
           "redo_share_occluded": round(redo_occ / max(n, 1), 5), "flags_equal": same}
    print(json.dumps(row), flush=True)
    if not same:
        raise SystemExit("occlusion flags differ from the closest-hit flags on " + name)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-100k", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    from nanort_amd import BVHAccel, Scene, TriangleMesh, scenes
    from scene_fixture import instances, xform

    cam = scenes.camera_rays(args.width, args.height)
    rows = []
    sc, keep = Scene(), []
    for v, f, x in instances(sphere_res=(264, 132), plane_res=(1000, 500)):
        a = BVHAccel(np.float32)
        assert a.Build(f.shape[0], TriangleMesh(v, f))
        keep.append(a)
        sc.AddNode(a, x)
    assert sc.Commit()
    rows.append(probe("fixture_5_nodes", sc, cam, args.steps, args.warmup))
    del sc, keep
    sv, sf = scenes.sphere(48, 24)
    sv = sv - np.array([0, 5, 0], dtype=np.float32)
    a = BVHAccel(np.float32)
    assert a.Build(sf.shape[0], TriangleMesh(sv, sf))
    for name, count in (("instances_10k", 10000), ("instances_100k", 100000)):
        if count == 100000 and args.skip_100k:
            continue
        rng = np.random.default_rng(5)  # (the transforms of bench_rows.scene_rows)
        sc = Scene()
        for _ in range(count):
            sc.AddNode(a, xform(tuple(rng.uniform(0.01, 0.04, 3)), rng.uniform(0, 6.28), rng.uniform(0, 6.28), tuple(rng.uniform(-9, 9, 3) + np.array([0, 5, 0]))))
        assert sc.Commit()
        rows.append(probe(name, sc, cam, args.steps, args.warmup))
        del sc
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fp:
            json.dump(rows, fp, indent=1)


if __name__ == "__main__":
    main()

"""The combined ray query on C3 — Plane(1000, 500), 1 M triangles, fp32, 1920x1080 objrender camera, keyframe 1 a jitter of keyframe
0, one random 32-bit word per triangle: primaries and their bounce rays, everything resident in HBM.  Every ray carries a uniform
random time, one of eight words (everything, single bits, two bits: about half of the mesh hidden on average) and — the bounce rays —
the id of the triangle it leaves.  Per ray set, in one process and over the same rays, three launches ALTERNATING round by round
after a ramp of untimed rounds (each launch timed by nrtLastTraverseMs, which waits for it):
  (a) nrtQueryBatchDevice_f32 with MOTION | MASKED and the ids — k_traverse_query<float, 32, true, true>, the code under test;
  (b) nrtTraverseBatchMotionDevice_f32 with the same times  — k_traverse_motion, which sees every triangle and skips none;
  (c) nrtTraverseBatchMaskedDevice_f32 with the same words  — k_traverse_masked, at keyframe 0, which skips none.
(b) and (c) are the yardsticks: the two walks a caller had to choose between.  Writes profiles/query_probe_c3.json and prints it as
one JSON line.

    python tools/query_probe.py [--rounds 30] [--ramp 10] [--out profiles/query_probe_c3.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORDS = (0xFFFFFFFF, 1, 2, 0x80000000, 0x00010000, 3, 0x7FFFFFFF, 0x0000FF00)


def main():
    import torch

    from nanort_amd import BVHAccel, MotionTriangleMesh, scenes

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--ramp", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--jitter", type=float, default=1e-2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_probe_c3.json"))
    args = ap.parse_args()

    v, f = scenes.plane(1000, 500)
    nf = f.shape[0]
    rng = np.random.default_rng(1)
    v1 = np.ascontiguousarray((v + rng.normal(scale=args.jitter, size=v.shape)).astype(np.float32))
    pm = rng.integers(0, 1 << 32, size=nf, dtype=np.uint64).astype(np.uint32)
    acc = BVHAccel(np.float32)
    assert acc.Build(nf, MotionTriangleMesh(v, v1, f))
    acc.SetPrimMasks(pm)

    cam = scenes.camera_rays(args.width, args.height)
    h, m = acc.TraverseBatch(cam)
    bounce = scenes.secondary_rays("bounce", v, f, cam, h, m)
    left = np.ascontiguousarray(h["prim_id"][m != 0]).astype(np.uint32)
    assert left.shape[0] == bounce.shape[0], "one bounce ray per primary hit, in their order"

    out = {"probe": "query", "mesh": "C3 plane(1000,500)", "tris": int(nf), "image": "%dx%d" % (args.width, args.height), "rounds": args.rounds,
           "ramp": args.ramp, "jitter": args.jitter, "rays": {}}
    for name, rays, ids in (("primary", cam, np.full(cam.shape[0], 0xFFFFFFFF, dtype=np.uint32)), ("bounce", bounce, left)):
        n = rays.shape[0]
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_times = torch.from_numpy(rng.uniform(0.0, 1.0, size=n).astype(np.float32)).cuda()
        d_words = torch.from_numpy(np.asarray(WORDS, dtype=np.uint32)[rng.integers(0, len(WORDS), size=n)].view(np.int32).copy()).cuda()
        d_ids = torch.from_numpy(ids.view(np.int32).copy()).cuda()
        d_hits = [torch.zeros((n * 16,), dtype=torch.uint8, device="cuda") for _ in range(3)]
        d_mask = [torch.zeros((n,), dtype=torch.uint8, device="cuda") for _ in range(3)]
        launches = (
            ("query_all_three", lambda: acc.QueryBatchDevice(d_rays, d_hits[0], d_mask[0], times=d_times, ray_masks=d_words, skip_prim_ids=d_ids)),
            ("motion_only", lambda: acc.TraverseBatchMotionDevice(d_rays, d_times, d_hits[1], d_mask[1])),
            ("masked_only", lambda: acc.TraverseBatchMaskedDevice(d_rays, d_words, d_hits[2], d_mask[2])),
        )
        times = {k: [] for k, _ in launches}
        kernels = {}
        for r in range(args.ramp + args.rounds):
            for k, launch in launches:
                launch()
                t = acc.LastTraverseMs()  # (waits for the launch)
                kernels[k] = acc.LastKernelName()
                if r >= args.ramp:
                    times[k].append(t)
        torch.cuda.synchronize()
        assert kernels == {"query_all_three": "nrt::k_traverse_query<float, 32, true, true>", "motion_only": "nrt::k_traverse_motion<float>",
                           "masked_only": "nrt::k_traverse_masked<float>"}, kernels
        row = {"n": int(n)}
        for j, (k, _) in enumerate(launches):
            t = np.asarray(times[k])
            row[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "grays_s": n / float(np.median(t)) / 1e6,
                      "hits": int(d_mask[j].sum())}
        row["query_over_motion"] = row["query_all_three"]["median_ms"] / row["motion_only"]["median_ms"]
        row["query_over_masked"] = row["query_all_three"]["median_ms"] / row["masked_only"]["median_ms"]
        out["rays"][name] = row
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()

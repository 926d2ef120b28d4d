#!/usr/bin/env python3
"""What per-ray skip ids cost: the bounce wave of the 1M-triangle plane (1920x1080 primaries) through the NON-PLAIN walk, timed by
the kernel's own completion stamps (LastTraverseMs), one mode per process so that two builds of the library can be alternated:

    --mode skip_option   options.skip_prim_id = one in-range id        (any build; the parent's way into the non-PLAIN variant)
    --mode skip_ids      an all-sentinel skip_prim_ids array           (builds with nrtTraverseBatchSkipDevice)
    --mode plain         default options                                (the PLAIN variant, for scale)

`--root DIR` imports nanort_amd from another checkout (built there) instead of this one.  Prints one JSON line: the kernel's name,
the median / min / max launch time over `--reps` launches after `--warmup` untimed ones, and a digest of the records (plain and
skip_ids must report the same one: the sentinel skips nothing).
"""
import argparse
import hashlib
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("skip_option", "skip_ids", "plain"), required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    import numpy as np
    import torch

    from nanort_amd import BVHAccel, TriangleMesh, scenes
    from nanort_amd.wire import default_trace_options

    v, f = scenes.plane(1000, 500)
    a = BVHAccel(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    rays1 = scenes.camera_rays(1920, 1080)
    h1, m1 = a.TraverseBatch(rays1)
    bounce = scenes.secondary_rays("bounce", v, f, rays1, h1, m1)
    n = bounce.shape[0]
    d_rays = torch.from_numpy(bounce.view(np.uint8)).cuda()
    d_hits = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    opt, kw = None, {}
    if args.mode == "skip_option":
        opt = default_trace_options()
        opt["skip_prim_id"] = f.shape[0] - 1  # in range (the launch is not PLAIN); the far corner of the plane
    elif args.mode == "skip_ids":
        kw["skip_prim_ids"] = torch.from_numpy(np.full(n, 0xFFFFFFFF, dtype=np.uint32).view(np.uint8)).cuda()
    torch.cuda.synchronize()
    ms = []
    for k in range(args.warmup + args.reps):
        a.TraverseBatchDevice(d_rays, d_hits, d_mask, opt, **kw)
        t = a.LastTraverseMs()  # (waits for the launch)
        if k >= args.warmup:
            ms.append(t)
    torch.cuda.synchronize()
    ms = np.array(ms)
    digest = hashlib.sha256(d_hits.cpu().numpy().tobytes() + d_mask.cpu().numpy().tobytes()).hexdigest()[:16]
    print(json.dumps({"label": args.label, "mode": args.mode, "kernel": a.LastKernelName(), "rays": int(n), "reps": args.reps,
                      "ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4), "ms_max": round(float(ms.max()), 4),
                      "mrays_s_median": round(n / float(np.median(ms)) / 1e3, 1), "records": digest}))


if __name__ == "__main__":
    main()

"""Multi-hit throughput (nrtMultiHitTraverseBatchDevice) on C3 — Plane(1000, 500), 1 M triangles, 1920x1080 objrender camera —
for its primary rays and their bounce wave, K in {1, 4, 8, 16}, next to the default closest-hit walk and the literal binary walk
(tunable wide = 0) on the same rays.  Kernel time of each launch from the library's own launch timing (LastTraverseMs), median of
`reps`; prints one JSON line.

    python tools/multihit_probe.py [--reps 9]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from nanort_amd import BVHAccel, TriangleMesh, scenes

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    v, f = scenes.plane(1000, 500)
    a = BVHAccel(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v, f))
    a.SetLaunchTiming(1)
    r1 = scenes.camera_rays(1920, 1080)
    h1, m1 = a.TraverseBatch(r1)
    waves = {"primary": r1, "bounce": scenes.secondary_rays("bounce", v, f, r1, h1, m1)}
    out = {"probe": "multihit", "mesh": "C3 plane(1000,500)", "tris": int(f.shape[0]), "image": "1920x1080", "reps": args.reps}

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(args.reps):
            fn()
            torch.cuda.synchronize()
            t.append(a.LastTraverseMs())
        return float(np.median(t))

    for name, rays in waves.items():
        n = rays.shape[0]
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_hits = torch.empty((n * 16 * 16,), dtype=torch.uint8, device="cuda")
        d_mask = torch.empty((n,), dtype=torch.uint8, device="cuda")
        d_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
        row = {"rays": n}
        ms = timed(lambda: a.TraverseBatchDevice(d_rays, d_hits, d_mask))
        row["closest_default"] = {"ms": ms, "mrays_s": n / ms / 1e3}
        a.SetTunable("wide", 0)
        ms = timed(lambda: a.TraverseBatchDevice(d_rays, d_hits, d_mask))
        a.SetTunable("wide", 1)
        row["closest_literal"] = {"ms": ms, "mrays_s": n / ms / 1e3}
        for K in (1, 4, 8, 16):
            ms = timed(lambda: a.MultiHitTraverseBatchDevice(d_rays, K, d_hits, d_counts))
            row["multihit_k%d" % K] = {"ms": ms, "mrays_s": n / ms / 1e3, "mean_count": float(d_counts.float().mean())}
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Multi-hit with per-ray skip ids, visibility words and motion times on C3 — Plane(1000, 500), 1 M triangles, fp32, 1920x1080
objrender camera, K = 4, keyframe 1 a small jitter of keyframe 0, one random non-zero 32-bit word per triangle, all-ones ray words:
primaries and their bounce rays, everything resident in HBM.  Per ray set, in one process and over the same rays, three launches
ALTERNATING call by call after a ramp of untimed rounds (each launch timed by nrtLastTraverseMs, which waits for it), median of
--rounds calls each:
  (a) nrtMultiHitTraverseBatchDevice_f32 — k_traverse_multihit<float>, the parent's kernel;
  (b) nrtMultiHitQueryBatchDevice_f32 with MOTION | MASKED and ids, every array neutral: times 0, words all-ones, ids 0xFFFFFFFF —
      k_multihit_query<float, 32, true, true>; its bytes must equal (a)'s;
  (c) the same with the real arrays: a uniform random time per ray, all-ones words, and — the bounce rays — the id of the triangle
      the ray leaves.
b/a is the feature's cost, to be read next to (a)'s own spread (max - min); c/a is the workload's change.  Writes
profiles/multihit_query_probe.json and prints it as one JSON line.

    python tools/multihit_query_probe.py [--rounds 31] [--ramp 10] [--out profiles/multihit_query_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rocm_version():
    try:
        return open("/opt/rocm/.info/version").read().strip()
    except OSError:
        return None


def main():
    import torch

    from nanort_amd import BVHAccel, MotionTriangleMesh, scenes

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--ramp", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--max-hits", type=int, default=4)
    ap.add_argument("--jitter", type=float, default=1e-2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multihit_query_probe.json"))
    args = ap.parse_args()
    K = args.max_hits

    v, f = scenes.plane(1000, 500)
    nf = f.shape[0]
    rng = np.random.default_rng(1)
    v1 = np.ascontiguousarray((v + rng.normal(scale=args.jitter, size=v.shape)).astype(np.float32))
    pm = rng.integers(1, 1 << 32, size=nf, dtype=np.uint64).astype(np.uint32)  # (non-zero: an all-ones ray word sees every triangle)
    acc = BVHAccel(np.float32)
    assert acc.Build(nf, MotionTriangleMesh(v, v1, f))
    acc.SetPrimMasks(pm)

    cam = scenes.camera_rays(args.width, args.height)
    h, m = acc.TraverseBatch(cam)
    bounce = scenes.secondary_rays("bounce", v, f, cam, h, m)
    left = np.ascontiguousarray(h["prim_id"][m != 0]).astype(np.uint32)
    assert left.shape[0] == bounce.shape[0], "one bounce ray per primary hit, in their order"

    out = {"probe": "multihit_query", "mesh": "C3 plane(1000,500)", "tris": int(nf), "image": "%dx%d" % (args.width, args.height), "max_hits": K,
           "rounds": args.rounds, "ramp": args.ramp, "jitter": args.jitter, "rocm": rocm_version(), "hip": torch.version.hip,
           "device": torch.cuda.get_device_name(0), "rays": {}}
    for name, rays, ids in (("primary", cam, np.full(cam.shape[0], 0xFFFFFFFF, dtype=np.uint32)), ("bounce", bounce, left)):
        n = rays.shape[0]
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_times = torch.from_numpy(rng.uniform(0.0, 1.0, size=n).astype(np.float32)).cuda()
        d_zero = torch.zeros((n,), dtype=torch.float32, device="cuda")
        d_ones = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        d_ids = torch.from_numpy(ids.view(np.int32).copy()).cuda()
        d_hits = [torch.zeros((n * K * 16,), dtype=torch.uint8, device="cuda") for _ in range(3)]
        d_cnt = [torch.zeros((n,), dtype=torch.int32, device="cuda") for _ in range(3)]
        launches = (
            ("plain", lambda: acc.MultiHitTraverseBatchDevice(d_rays, K, d_hits[0], d_cnt[0])),
            ("query_neutral", lambda: acc.MultiHitQueryBatchDevice(d_rays, K, d_hits[1], d_cnt[1], times=d_zero, ray_masks=d_ones, skip_prim_ids=d_ones)),
            ("query_real", lambda: acc.MultiHitQueryBatchDevice(d_rays, K, d_hits[2], d_cnt[2], times=d_times, ray_masks=d_ones, skip_prim_ids=d_ids)),
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
        assert kernels == {"plain": "nrt::k_traverse_multihit<float>", "query_neutral": "nrt::k_multihit_query<float, 32, true, true>",
                           "query_real": "nrt::k_multihit_query<float, 32, true, true>"}, kernels
        assert torch.equal(d_hits[0], d_hits[1]) and torch.equal(d_cnt[0], d_cnt[1]), "the neutral query's bytes differ from the plain call's"
        row = {"n": int(n), "neutral_bytes_equal_plain": True}
        for j, (k, _) in enumerate(launches):
            t = np.asarray(times[k])
            row[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                      "spread_over_median": float((t.max() - t.min()) / np.median(t)), "held": int(d_cnt[j].sum())}
        row["b_over_a"] = row["query_neutral"]["median_ms"] / row["plain"]["median_ms"]
        row["c_over_a"] = row["query_real"]["median_ms"] / row["plain"]["median_ms"]
        row["rows_changed_by_the_real_arrays"] = int((d_hits[2].view(n, -1) != d_hits[0].view(n, -1)).any(dim=1).sum())
        out["rays"][name] = row
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()

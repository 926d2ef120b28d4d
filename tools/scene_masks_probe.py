#!/usr/bin/env python3
"""What instance visibility masks cost on instanced scenes: Scene.TraverseBatchDevice / OccludedBatchDevice beside their masked
forms on a 1920x1080 camera wave resident in HBM, on the three scenes of the bench rows — the 5-node fixture and the 10 000- and
100 000-instance scenes bench_rows.py builds.  Stand-alone; bench.py does not call it.

Three arms, ALTERNATED call by call in one process after a clock ramp (so that drift and clock state hit them alike):
    a  the unmasked call
    b  the masked call with all-ones words on both sides (node words and ray words): the same work plus the feature's loads
    c  the masked call with a random half of the instances hidden from every ray (ray words all ones, node words 0 on that half),
       on a second scene committed from the same nodes, so that no arm pays for changing the words between calls
Each figure: the median of `--steps` timed calls per arm (each call is synchronous and ends with the stream drained), the spread
(min .. max) of arm a, and the ratios b/a and c/a of the median TIMES (1.00 = free, above = slower).

    python3 tools/scene_masks_probe.py [--width 1920 --height 1080 --steps 31 --ramp 10 --skip-100k] [--json out.json]
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

ALL = 0xFFFFFFFF


def alternate(arms, steps, ramp):
    """Seconds per call of every arm, the arms taking turns; `ramp` untimed rounds first."""
    import torch

    ts = {k: [] for k in arms}
    for r in range(ramp + steps):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= ramp:
                ts[k].append(time.perf_counter() - t0)
    return {k: np.array(v) for k, v in ts.items()}


def probe(name, sc, sc_half, num_nodes, cam, steps, ramp):
    import torch

    from nanort_amd.wire import SCENE_HIT_F32

    n = cam.shape[0]
    rng = np.random.default_rng(11)
    ones = np.full(num_nodes, ALL, dtype=np.uint32)
    half = ones.copy()
    half[rng.permutation(num_nodes)[: num_nodes // 2]] = 0
    sc.SetNodeMasks(ones)
    sc_half.SetNodeMasks(half)
    d_rays = torch.from_numpy(cam.view(np.uint8)).cuda()
    d_words = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_hits = [torch.empty(n * SCENE_HIT_F32.itemsize, dtype=torch.uint8, device="cuda") for _ in range(3)]
    d_mask = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(3)]
    rows = []
    for kind in ("closest_hit", "occluded"):
        def masked(s, i, kind=kind):
            if kind == "closest_hit":
                s.TraverseBatchMaskedDevice(d_rays, d_words, d_hits[i], d_mask[i])
            else:
                s.OccludedBatchMaskedDevice(d_rays, d_words, d_mask[i])

        def plain(kind=kind):
            if kind == "closest_hit":
                sc.TraverseBatchDevice(d_rays, d_hits[0], d_mask[0])
            else:
                sc.OccludedBatchDevice(d_rays, d_mask[0])

        ts = alternate({"a": plain, "b": lambda: masked(sc, 1), "c": lambda: masked(sc_half, 2)}, steps, ramp)
        path, redone = sc_half.LastPath(), sc_half.LastRedone()
        med = {k: float(np.median(v)) for k, v in ts.items()}
        same = bool(torch.equal(d_mask[0], d_mask[1])) and (kind != "closest_hit" or bool(torch.equal(d_hits[0], d_hits[1])))
        row = {"scene": name, "query": kind, "rays": n, "steps": steps,
               "a_unmasked_ms": round(med["a"] * 1e3, 4), "a_min_ms": round(float(ts["a"].min()) * 1e3, 4), "a_max_ms": round(float(ts["a"].max()) * 1e3, 4),
               "a_spread_pct": round(100.0 * float(ts["a"].max() - ts["a"].min()) / med["a"], 2),
               "b_all_ones_ms": round(med["b"] * 1e3, 4), "c_half_hidden_ms": round(med["c"] * 1e3, 4),
               "b_over_a": round(med["b"] / med["a"], 4), "c_over_a": round(med["c"] / med["a"], 4),
               "a_Mrays_s": round(n / med["a"] / 1e6, 1), "hit_share_a": round(float(d_mask[0].float().mean().item()), 4),
               "hit_share_c": round(float(d_mask[2].float().mean().item()), 4),
               "path_of_c": "single-pass walk" if path == 1 else "listing path", "redo_share_c": round(redone / max(n, 1), 5),
               "b_bytes_equal_a": same}
        print(json.dumps(row), flush=True)
        if not same:
            raise SystemExit("all-ones masks changed the bytes of the %s call on %s" % (kind, name))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=31)
    ap.add_argument("--ramp", type=int, default=10)
    ap.add_argument("--skip-100k", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import torch

    from nanort_amd import BVHAccel, Scene, TriangleMesh, capi, scenes
    from scene_fixture import instances, xform

    cam = scenes.camera_rays(args.width, args.height)
    rows = []
    pair, keep = [Scene(), Scene()], []
    for v, f, x in instances(sphere_res=(264, 132), plane_res=(1000, 500)):
        a = BVHAccel(np.float32)
        assert a.Build(f.shape[0], TriangleMesh(v, f))
        keep.append(a)
        for sc in pair:
            sc.AddNode(a, x)
    assert pair[0].Commit() and pair[1].Commit()
    rows += probe("fixture_5_nodes", pair[0], pair[1], 5, cam, args.steps, args.ramp)
    del pair, sc, keep
    sv, sf = scenes.sphere(48, 24)
    sv = sv - np.array([0, 5, 0], dtype=np.float32)
    a = BVHAccel(np.float32)
    assert a.Build(sf.shape[0], TriangleMesh(sv, sf))
    for name, count in (("instances_10k", 10000), ("instances_100k", 100000)):
        if count == 100000 and args.skip_100k:
            continue
        rng = np.random.default_rng(5)  # (the transforms of bench_rows.scene_rows)
        pair = [Scene(), Scene()]
        for _ in range(count):
            x = xform(tuple(rng.uniform(0.01, 0.04, 3)), rng.uniform(0, 6.28), rng.uniform(0, 6.28), tuple(rng.uniform(-9, 9, 3) + np.array([0, 5, 0])))
            for sc in pair:
                sc.AddNode(a, x)
        assert pair[0].Commit() and pair[1].Commit()
        rows += probe(name, pair[0], pair[1], count, cam, args.steps, args.ramp)
        del pair, sc
    rocm = "/opt/rocm/.info/version"
    out = {"library": capi.lib().nrtVersion().decode(), "hip": torch.version.hip, "rocm": open(rocm).read().strip() if os.path.exists(rocm) else None,
           "device": torch.cuda.get_device_name(0),
           "method": "arms a/b/c alternated call by call in one process after %d untimed rounds; median of %d calls per arm; ratios of median times"
                     % (args.ramp, args.steps),
           "rows": rows}
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()

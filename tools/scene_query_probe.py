#!/usr/bin/env python3
"""What per-ray skip pairs cost on instanced scenes, and what they change: a BOUNCE wave started at the hit points of a 1920x1080
camera wave (random unit directions, no epsilon offset), resident in HBM, on the three scenes of the bench rows — the 5-node fixture
and the 10 000- and 100 000-instance scenes bench_rows.py builds.  Stand-alone; bench.py does not call it.

Three arms, ALTERNATED call by call in one process after a clock ramp (so that drift and clock state hit them alike):
    a  the existing unskipped call (Scene.TraverseBatchDevice / OccludedBatchDevice)
    b  Scene.QueryBatchDevice with SKIP and every pair invalid (0xFFFFFFFF, 0xFFFFFFFF): the same work plus the feature's loads
    c  Scene.QueryBatchDevice with the real pairs: the primary wave's records as they lie (stride 20)
Each figure: the median of `--steps` timed calls per arm (each call is synchronous and ends with the stream drained), the spread
(min .. max) of arm a, and the ratios b/a and c/a of the median TIMES.  b/a is the feature's cost.  c/a is the workload's change:
rays that no longer stop at t ~ 0 on the triangle they start from walk further, so (c) may be slower than (a) while being the
right answer; the share of rays that name their own pair in (a) and in (c) is reported beside it.

    python3 tools/scene_query_probe.py [--width 1920 --height 1080 --steps 31 --ramp 10 --skip-100k] [--json out.json]
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


def own_share(d_hits, d_mask, records, n):
    from nanort_amd.wire import SCENE_HIT_F32
    from scene_query_fixture import own_pair_share, pairs_of  # (tests/: one statement of the wave and of "its own pair")

    h = d_hits.cpu().numpy().view(SCENE_HIT_F32)[:n]
    return own_pair_share(h, d_mask.cpu().numpy()[:n], pairs_of(records))


def probe(name, sc, cam, steps, ramp):
    import torch

    from nanort_amd.wire import SCENE_HIT_F32

    rec = SCENE_HIT_F32.itemsize
    n0 = cam.shape[0]
    d_cam = torch.from_numpy(cam.view(np.uint8)).cuda()
    d_h0 = torch.empty(n0 * rec, dtype=torch.uint8, device="cuda")
    d_m0 = torch.empty(n0, dtype=torch.uint8, device="cuda")
    sc.TraverseBatchDevice(d_cam, d_h0, d_m0)
    from scene_query_fixture import bounce_wave

    rays, _, records = bounce_wave(cam, d_h0.cpu().numpy().view(SCENE_HIT_F32), d_m0.cpu().numpy(), np.random.default_rng(7))
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    d_records = torch.from_numpy(records.view(np.uint8)).cuda()
    d_invalid = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
    d_hits = [torch.empty(n * rec, dtype=torch.uint8, device="cuda") for _ in range(3)]
    d_mask = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(3)]
    rows = []
    for kind in ("closest_hit", "occluded"):
        occ = kind == "occluded"

        def plain(occ=occ):
            if occ:
                sc.OccludedBatchDevice(d_rays, d_mask[0])
            else:
                sc.TraverseBatchDevice(d_rays, d_hits[0], d_mask[0])

        def query(i, pairs, occ=occ):
            sc.QueryBatchDevice(d_rays, None if occ else d_hits[i], d_mask[i], skip_pairs=pairs, occlusion=occ)

        ts = alternate({"a": plain, "b": lambda: query(1, d_invalid), "c": lambda: query(2, d_records)}, steps, ramp)
        path, redone = sc.LastPath(), sc.LastRedone()
        med = {k: float(np.median(v)) for k, v in ts.items()}
        same = bool(torch.equal(d_mask[0], d_mask[1])) and (occ or bool(torch.equal(d_hits[0], d_hits[1])))
        row = {"scene": name, "query": kind, "rays": n, "steps": steps,
               "a_unskipped_ms": round(med["a"] * 1e3, 4), "a_min_ms": round(float(ts["a"].min()) * 1e3, 4), "a_max_ms": round(float(ts["a"].max()) * 1e3, 4),
               "a_spread_pct": round(100.0 * float(ts["a"].max() - ts["a"].min()) / med["a"], 2),
               "b_invalid_pairs_ms": round(med["b"] * 1e3, 4), "c_real_pairs_ms": round(med["c"] * 1e3, 4),
               "b_over_a": round(med["b"] / med["a"], 4), "c_over_a": round(med["c"] / med["a"], 4),
               "a_Mrays_s": round(n / med["a"] / 1e6, 1), "hit_share_a": round(float(d_mask[0].float().mean().item()), 4),
               "hit_share_c": round(float(d_mask[2].float().mean().item()), 4),
               "flags_changed_c": round(float((d_mask[0] != d_mask[2]).float().mean().item()), 4),
               "path_of_c": "single-pass walk" if path == 1 else "listing path", "redo_share_c": round(redone / max(n, 1), 5),
               "b_bytes_equal_a": same}
        if not occ:
            row["own_pair_share_a"] = round(own_share(d_hits[0], d_mask[0], records, n), 4)
            row["own_pair_share_c"] = round(own_share(d_hits[2], d_mask[2], records, n), 4)
        print(json.dumps(row), flush=True)
        if not same:
            raise SystemExit("pairs that skip nothing changed the bytes of the %s call on %s" % (kind, name))
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
    sc, keep = Scene(), []
    for v, f, x in instances(sphere_res=(264, 132), plane_res=(1000, 500)):
        a = BVHAccel(np.float32)
        assert a.Build(f.shape[0], TriangleMesh(v, f))
        keep.append(a)
        sc.AddNode(a, x)
    assert sc.Commit()
    rows += probe("fixture_5_nodes", sc, cam, args.steps, args.ramp)
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
        rows += probe(name, sc, cam, args.steps, args.ramp)
        del sc
    rocm = "/opt/rocm/.info/version"
    out = {"library": capi.lib().nrtVersion().decode(), "hip": torch.version.hip, "rocm": open(rocm).read().strip() if os.path.exists(rocm) else None,
           "device": torch.cuda.get_device_name(0),
           "method": "bounce wave from the camera wave's hits; arms a/b/c alternated call by call in one process after %d untimed rounds; "
                     "median of %d calls per arm; ratios of median times" % (args.ramp, args.steps),
           "rows": rows}
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()

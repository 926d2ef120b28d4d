"""Closest-point queries on instanced scenes (nrtSceneClosestPointBatchDevice_f32) with the points resident in HBM,
on the three scenes of the SURVEY 8(f) row — the 5-node fixture, 10 000 and 100 000 instances of one lumpy sphere — and two point
sets per scene, max_dist = +inf:
  (i)  the hit points of the 1920x1080 camera wave on that scene, each offset by up to 1 % of the scene's diagonal in a random direction;
  (ii) 2 M uniform points in the scene's bounds.
Per scene and set, after --ramp untimed calls, the median (min - max) of --rounds calls as Mqueries/s (the call is synchronous:
wall time around it); nodes opened, instances entered and triangles tested per query from the profiling library's counters (a child
process with NRT_USE_PROF_LIB=1 over the same points).
THE COST OF THE SECOND LEVEL AND THE WORLD TRANSFORM, as a ratio: a scene of ONE identity instance of C3's mesh — Plane(1000, 500) —
against nrtClosestPointBatchDevice_f32 on that mesh's context, closest_probe.py's two point sets, the two calls alternated call by
call.  Writes profiles/scene_closest_probe.json and prints it as one JSON line.

    python tools/scene_closest_probe.py [--rounds 31] [--ramp 10] [--skip-100k] [--out profiles/scene_closest_probe.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms, n):
    t = np.asarray(ms)
    return {"n": int(n), "median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "mqueries_per_s": float(n / np.median(t) / 1e3)}


def make_points(xyz):
    from nanort_amd.wire import POINT_F32

    pts = np.zeros((xyz.shape[0],), dtype=POINT_F32)
    pts["p"] = xyz.astype(np.float32)
    pts["max_dist"] = np.inf
    return pts


def scene_points(sc, cam, uniform):
    rng = np.random.default_rng(1)
    lo, hi = [x.astype(np.float64) for x in sc.GetBoundingBox()]
    diag = float(np.linalg.norm(hi - lo))
    h, m = sc.TraverseBatch(cam)
    m = m != 0
    hp = cam["org"][m].astype(np.float64) + cam["dir"][m].astype(np.float64) * h["t"][m].astype(np.float64)[:, None]
    d = rng.normal(size=hp.shape)
    d /= np.linalg.norm(d, axis=1)[:, None]
    return {"camera_hits_offset_1pct": make_points(hp + d * rng.uniform(0.0, 0.01 * diag, size=(hp.shape[0], 1))),
            "uniform_in_bounds": make_points(rng.uniform(lo, hi, size=(uniform, 3)))}


def scenes_of_the_row(skip_100k):
    """(name, Scene, what to keep alive) for the three scenes, one at a time."""
    from nanort_amd import BVHAccel, Scene, TriangleMesh, scenes
    from scene_fixture import instances, xform

    sc, keep = Scene(), []
    for v, f, x in instances(sphere_res=(264, 132), plane_res=(1000, 500)):
        a = BVHAccel(np.float32)
        assert a.Build(f.shape[0], TriangleMesh(v, f))
        keep.append(a)
        sc.AddNode(a, x)
    assert sc.Commit()
    yield "fixture_5_nodes", sc, keep
    sv, sf = scenes.sphere(48, 24)
    sv = sv - np.array([0, 5, 0], dtype=np.float32)
    a = BVHAccel(np.float32)
    assert a.Build(sf.shape[0], TriangleMesh(sv, sf))
    for name, count in (("instances_10k", 10000), ("instances_100k", 100000)):
        if count == 100000 and skip_100k:
            continue
        rng = np.random.default_rng(5)  # (the transforms of bench_rows.scene_rows)
        sc = Scene()
        for _ in range(count):
            sc.AddNode(a, xform(tuple(rng.uniform(0.01, 0.04, 3)), rng.uniform(0, 6.28), rng.uniform(0, 6.28), tuple(rng.uniform(-9, 9, 3) + np.array([0, 5, 0]))))
        assert sc.Commit()
        yield name, sc, [a]


def main():
    import torch

    from nanort_amd import BVHAccel, Scene, TriangleMesh, scenes

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--ramp", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--uniform", type=int, default=2000000)
    ap.add_argument("--skip-100k", action="store_true")
    ap.add_argument("--counts-only", action="store_true", help="(the child process: print the profiling library's counters per scene and set)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_closest_probe.json"))
    args = ap.parse_args()
    cam = scenes.camera_rays(args.width, args.height)

    if args.counts_only:
        assert os.environ.get("NRT_USE_PROF_LIB") == "1"
        res = {}
        for name, sc, _keep in scenes_of_the_row(args.skip_100k):
            sc._L.nrtSceneDebugCounters.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
            for sname, pts in scene_points(sc, cam, args.uniform).items():
                n = pts.shape[0]
                d_out = torch.zeros((n * 32,), dtype=torch.uint8, device="cuda")
                sc.ClosestPointBatchDevice(torch.from_numpy(pts.view(np.uint8).copy()).cuda(), d_out)
                c = np.zeros(16, dtype=np.uint64)
                assert sc._L.nrtSceneDebugCounters(sc._h, c.ctypes.data_as(ctypes.c_void_p), 16) == 0
                res[name + "/" + sname] = {"nodes_opened_per_query": float(c[0]) / n, "instances_entered_per_query": float(c[1]) / n,
                                           "tris_tested_per_query": float(c[2]) / n}
        print(json.dumps(res))
        return

    out = {"probe": "scene_closest_point", "image": "%dx%d" % (args.width, args.height), "rounds": args.rounds, "ramp": args.ramp,
           "hip": torch.version.hip, "device": torch.cuda.get_device_name(0), "rows": {}, "not_measured": []}
    for name, sc, _keep in scenes_of_the_row(args.skip_100k):
        for sname, pts in scene_points(sc, cam, args.uniform).items():
            n = pts.shape[0]
            d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
            d_out = torch.zeros((n * 32,), dtype=torch.uint8, device="cuda")
            d_found = torch.zeros((n,), dtype=torch.uint8, device="cuda")
            ms = [timed(lambda: sc.ClosestPointBatchDevice(d_pts, d_out, d_found)) for _ in range(args.ramp + args.rounds)][args.ramp:]
            assert sc.LastPath() == 2
            row = stats(ms, n)
            row["found"] = int(d_found.sum())
            out["rows"][name + "/" + sname] = row
            print(json.dumps({name + "/" + sname: row}), flush=True)
    if args.skip_100k:
        out["not_measured"].append("instances_100k")

    # the second level and the world transform, as a ratio: one identity instance of C3's mesh against the single-mesh query
    import closest_probe

    v, f = scenes.plane(1000, 500)
    acc = BVHAccel(np.float32)
    assert acc.Build(f.shape[0], TriangleMesh(v, f))
    one = Scene()
    one.AddNode(acc, np.eye(4, dtype=np.float32))
    assert one.Commit()
    out["one_identity_instance_of_c3"] = {}
    for sname, pts in closest_probe.point_sets(acc, v, f, args.width, args.height, args.uniform).items():
        n = pts.shape[0]
        d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
        d_a = torch.zeros((n * 32,), dtype=torch.uint8, device="cuda")
        d_b = torch.zeros((n * 32,), dtype=torch.uint8, device="cuda")
        ta, tb = [], []
        for r in range(args.ramp + args.rounds):
            a_ms = timed(lambda: acc.ClosestPointBatchDevice(d_pts, d_a))
            b_ms = timed(lambda: one.ClosestPointBatchDevice(d_pts, d_b))
            if r >= args.ramp:
                ta.append(a_ms)
                tb.append(b_ms)
        same = bool(torch.equal(d_a.view(-1, 32)[:, :28], d_b.view(-1, 32)[:, :28]))
        out["one_identity_instance_of_c3"][sname] = {"single_mesh": stats(ta, n), "scene": stats(tb, n),
                                                     "scene_over_single_mesh": float(np.median(tb) / np.median(ta)), "first_28_bytes_equal": same}
        print(json.dumps({sname: out["one_identity_instance_of_c3"][sname]}), flush=True)

    env = dict(os.environ, NRT_USE_PROF_LIB="1")
    try:  # (a slow or failed child loses the counters, not the timings above)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--counts-only", "--width", str(args.width), "--height", str(args.height),
                            "--uniform", str(args.uniform)] + (["--skip-100k"] if args.skip_100k else []), env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-400:])
        for key, row in json.loads(r.stdout.strip().splitlines()[-1]).items():
            out["rows"][key].update(row)
    except (subprocess.TimeoutExpired, RuntimeError, ValueError, IndexError, KeyError) as e:
        out["counters_error"] = str(e)[-400:]
        out["not_measured"].append("nodes opened / instances entered / triangles tested per query")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

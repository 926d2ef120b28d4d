"""Nearest-faces queries on C3's mesh — Plane(1000, 500), 1 M triangles, fp32 — with the points resident in HBM, on the two point
sets of tools/closest_probe.py: (i) the hit points of the objrender primary wave offset by up to 1 % of the diagonal (near the
surface), (ii) uniform points in the mesh's widened bounding box (far from it).

Per set and K in {1, 4, 16, 64}, once with max_dist = +inf and once with one radius for the whole set that admits about K / 2 faces
(the median, over the first --sample points, of the distance to the ceil(K / 2)-th nearest face, itself asked of the query):
nrtClosestPointBatchDevice_f32 and nrtNearestFacesBatchDevice_f32 over the same points with the same max_dist, alternated call by
call, each call timed by nrtLastTraverseMs (which waits for it); after --ramp untimed rounds the median of --rounds calls of each, and
the ratio of the two medians; the mean count; nodes opened and triangles tested per point from the profiling library's counters (a child
process with NRT_USE_PROF_LIB=1, over the same points).  Writes profiles/nearest_probe.json and prints it as one JSON line.

    python tools/nearest_probe.py [--rounds 15] [--ramp 5] [--uniform 2000000] [--out profiles/nearest_probe.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KS = (1, 4, 16, 64)


def radius_for(acc, pts, k, sample):
    """The median distance from the first `sample` points to their ceil(k / 2)-th nearest face."""
    half = -(-k // 2)
    rows, counts = acc.NearestFacesBatch(pts[:sample], half)
    d = np.sqrt(rows[counts == half, half - 1]["dist2"].astype(np.float64))
    return float(np.median(d))


def variants(acc, sets, sample):
    """[(set name, K, 'inf' | 'radius', max_dist)]"""
    out = []
    for name, pts in sets.items():
        for k in KS:
            out.append((name, k, "inf", float("inf")))
            out.append((name, k, "radius", radius_for(acc, pts, k, sample)))
    return out


def main():
    import torch

    import closest_probe
    from nanort_amd import BVHAccel, TriangleMesh, scenes

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--ramp", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--uniform", type=int, default=2000000)
    ap.add_argument("--sample", type=int, default=20000)
    ap.add_argument("--counts-only", action="store_true", help="(the child process: print the profiling library's counters per variant)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_probe.json"))
    args = ap.parse_args()

    v, f = scenes.plane(1000, 500)
    nf = f.shape[0]
    acc = BVHAccel(np.float32)
    assert acc.Build(nf, TriangleMesh(v, f))
    sets = closest_probe.point_sets(acc, v, f, args.width, args.height, args.uniform)
    todo = variants(acc, sets, args.sample)
    n_max = max(p.shape[0] for p in sets.values())
    d_out = torch.zeros((n_max * max(KS) * 32,), dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros((n_max,), dtype=torch.int32, device="cuda")

    def device_points(name, max_dist):
        pts = sets[name].copy()
        pts["max_dist"] = max_dist
        return torch.from_numpy(pts.view(np.uint8).copy()).cuda()

    if args.counts_only:
        assert os.environ.get("NRT_USE_PROF_LIB") == "1"
        acc._L.nrtDebugCounters.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        res = []
        for name, k, kind, max_dist in todo:
            n = sets[name].shape[0]
            acc.NearestFacesBatchDevice(device_points(name, max_dist), k, d_out, d_counts)
            torch.cuda.synchronize()
            c = np.zeros(16, dtype=np.uint64)
            assert acc._L.nrtDebugCounters(acc._h, c.ctypes.data_as(ctypes.c_void_p), 16) == 0
            res.append({"nodes_opened_per_point": float(c[0]) / n, "tris_tested_per_point": float(c[2]) / n})
        print(json.dumps(res))
        return

    out = {"probe": "nearest_faces", "mesh": "C3 plane(1000,500)", "tris": int(nf), "image": "%dx%d" % (args.width, args.height),
           "rounds": args.rounds, "ramp": args.ramp, "rocm": closest_probe.rocm_version(), "hip": torch.version.hip,
           "device": torch.cuda.get_device_name(0), "rows": []}

    for name, k, kind, max_dist in todo:
        n = sets[name].shape[0]
        d_pts = device_points(name, max_dist)
        base, t = [], []
        for r in range(args.ramp + args.rounds):  # (the two queries alternated call by call)
            acc.ClosestPointBatchDevice(d_pts, d_out)
            tb = acc.LastTraverseMs()  # (waits for the launch)
            assert acc.LastKernelName() == "nrt::k_closest_point<float, 32>"
            acc.NearestFacesBatchDevice(d_pts, k, d_out, d_counts)
            tn = acc.LastTraverseMs()
            assert acc.LastKernelName() == "nrt::k_nearest_faces<float, 32>"
            if r >= args.ramp:
                base.append(tb)
                t.append(tn)
        base, t = np.asarray(base), np.asarray(t)
        torch.cuda.synchronize()
        out["rows"].append({"set": name, "n": int(n), "k": k, "max_dist": kind, "radius": None if kind == "inf" else max_dist,
                            "median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                            "closest_point_median_ms": float(np.median(base)), "closest_point_min_ms": float(base.min()),
                            "closest_point_max_ms": float(base.max()), "ratio_to_closest_point": float(np.median(t) / np.median(base)),
                            "mpoints_per_s": float(n / np.median(t) / 1e3), "mean_count": float(d_counts[:n].double().mean())})

    # nodes opened / triangles tested per point: the profiling library, in a process of its own
    env = dict(os.environ, NRT_USE_PROF_LIB="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--counts-only", "--width", str(args.width), "--height", str(args.height),
                        "--uniform", str(args.uniform), "--sample", str(args.sample)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=400)
    if r.returncode == 0:
        for row, counters in zip(out["rows"], json.loads(r.stdout.strip().splitlines()[-1])):
            row.update(counters)
    else:
        out["counters_error"] = r.stderr[-400:]
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()

"""Closest-point queries on C3's mesh — Plane(1000, 500), 1 M triangles, fp32 — with the points resident in HBM:
  (i)  the hit points of the 1920x1080 objrender primary wave, each offset by up to 1 % of the mesh's diagonal in a random direction,
       max_dist = +inf: coherent, near the surface;
  (ii) 2 M uniform points in the mesh's bounding box (its thin axis widened to a tenth of the diagonal), max_dist = +inf: incoherent,
       far from the surface.
Per set, after a ramp of untimed calls, the median of --rounds calls of nrtClosestPointBatchDevice_f32 (each timed by
nrtLastTraverseMs, which waits for it) as Mqueries/s; nodes opened and triangles tested per query from the profiling library's
counters (a child process with NRT_USE_PROF_LIB=1, over the same points); and, as the CPU figure to stand against, the header's host
walk (include/nanort.h, BVHAccel::ClosestPoint through tests/cpp/closest_host_shim.cc, its own host-built tree) over the first
--host-points points of the set on --threads threads.  Writes profiles/closest_probe.json and prints it as one JSON line.

    python tools/closest_probe.py [--rounds 31] [--ramp 10] [--threads 16] [--host-points 200000] [--out profiles/closest_probe.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def rocm_version():
    try:
        return open("/opt/rocm/.info/version").read().strip()
    except OSError:
        return None


def point_sets(acc, v, f, width, height, uniform):
    from nanort_amd import scenes
    from nanort_amd.wire import POINT_F32

    rng = np.random.default_rng(1)
    bmin, bmax = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    diag = float(np.linalg.norm(bmax - bmin))
    cam = scenes.camera_rays(width, height)
    h, m = acc.TraverseBatch(cam)
    m = m != 0
    hp = cam["org"][m].astype(np.float64) + cam["dir"][m].astype(np.float64) * h["t"][m].astype(np.float64)[:, None]
    d = rng.normal(size=hp.shape)
    d /= np.linalg.norm(d, axis=1)[:, None]
    near = hp + d * rng.uniform(0.0, 0.01 * diag, size=(hp.shape[0], 1))
    lo, hi = bmin.copy(), bmax.copy()
    thin = (hi - lo) < 0.1 * diag
    lo[thin] -= 0.05 * diag
    hi[thin] += 0.05 * diag
    box = rng.uniform(lo, hi, size=(uniform, 3))
    sets = {}
    for name, xyz in (("primary_hits_offset_1pct", near), ("uniform_in_box", box)):
        pts = np.zeros((xyz.shape[0],), dtype=POINT_F32)
        pts["p"] = xyz.astype(np.float32)
        pts["max_dist"] = np.inf
        sets[name] = pts
    return sets


def main():
    import torch

    from nanort_amd import BVHAccel, TriangleMesh, scenes

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--ramp", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--uniform", type=int, default=2000000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-points", type=int, default=200000)
    ap.add_argument("--counts-only", action="store_true", help="(the child process: print the profiling library's counters per set)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_probe.json"))
    args = ap.parse_args()

    v, f = scenes.plane(1000, 500)
    nf = f.shape[0]
    acc = BVHAccel(np.float32)
    assert acc.Build(nf, TriangleMesh(v, f))
    sets = point_sets(acc, v, f, args.width, args.height, args.uniform)

    if args.counts_only:
        assert os.environ.get("NRT_USE_PROF_LIB") == "1"
        acc._L.nrtDebugCounters.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        res = {}
        for name, pts in sets.items():
            n = pts.shape[0]
            d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
            d_out = torch.zeros((n * 32,), dtype=torch.uint8, device="cuda")
            acc.ClosestPointBatchDevice(d_pts, d_out)
            torch.cuda.synchronize()
            c = np.zeros(16, dtype=np.uint64)
            assert acc._L.nrtDebugCounters(acc._h, c.ctypes.data_as(ctypes.c_void_p), 16) == 0
            res[name] = {"nodes_opened_per_query": float(c[0]) / n, "tris_tested_per_query": float(c[2]) / n}
        print(json.dumps(res))
        return

    import closest_fixture as cf

    out = {"probe": "closest_point", "mesh": "C3 plane(1000,500)", "tris": int(nf), "image": "%dx%d" % (args.width, args.height),
           "rounds": args.rounds, "ramp": args.ramp, "rocm": rocm_version(), "hip": torch.version.hip, "device": torch.cuda.get_device_name(0),
           "host_threads": args.threads, "sets": {}}
    keep = {}
    for name, pts in sets.items():
        n = pts.shape[0]
        d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
        d_out = torch.zeros((n * 32,), dtype=torch.uint8, device="cuda")
        d_found = torch.zeros((n,), dtype=torch.uint8, device="cuda")
        times = []
        for r in range(args.ramp + args.rounds):
            acc.ClosestPointBatchDevice(d_pts, d_out, d_found)
            t = acc.LastTraverseMs()  # (waits for the launch)
            if r >= args.ramp:
                times.append(t)
        torch.cuda.synchronize()
        assert acc.LastKernelName() == "nrt::k_closest_point<float, 32>"
        t = np.asarray(times)
        keep[name] = d_out.cpu().numpy()
        out["sets"][name] = {"n": int(n), "median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                             "mqueries_per_s": float(n / np.median(t) / 1e3), "found": int(d_found.sum())}

    # nodes opened / triangles tested per query: the profiling library, in a process of its own
    env = dict(os.environ, NRT_USE_PROF_LIB="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--counts-only", "--width", str(args.width), "--height", str(args.height),
                        "--uniform", str(args.uniform)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    if r.returncode == 0:
        for name, row in json.loads(r.stdout.strip().splitlines()[-1]).items():
            out["sets"][name].update(row)
    else:
        out["counters_error"] = r.stderr[-400:]

    # the header's host walk over its own host-built tree, on the same points
    t0 = time.time()
    host = cf.HostAccel(v, f)
    out["host_build_s"] = time.time() - t0
    for name, pts in sets.items():
        m = min(args.host_points, pts.shape[0])
        sub = np.ascontiguousarray(pts[:m])
        cuts = np.linspace(0, m, args.threads * 8 + 1).astype(int)
        t0 = time.time()
        with ThreadPoolExecutor(args.threads) as ex:  # (the shim's calls run outside the interpreter lock)
            parts = list(ex.map(lambda k: host.closest(sub[cuts[k]:cuts[k + 1]])[0], range(len(cuts) - 1)))
        dt = time.time() - t0
        rec = np.concatenate(parts)
        same = rec.tobytes() == keep[name][:m * 32].tobytes()
        out["sets"][name].update({"host_points": int(m), "host_s": dt, "host_mqueries_per_s": float(m / dt / 1e6), "host_records_equal_gpu": bool(same),
                                  "gpu_over_host": out["sets"][name]["mqueries_per_s"] / (m / dt / 1e6)})
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()

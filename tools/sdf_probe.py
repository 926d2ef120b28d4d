"""Signed distance queries on C3's mesh — Plane(1000, 500), 1 M triangles, fp32 — with tools/closest_probe.py's two point sets
resident in HBM: (i) the 1080p primary wave's hit points offset by up to 1 % of the diagonal, (ii) 2 M uniform points in the box.
Per set, after a ramp of untimed calls, nrtSignedDistanceBatchDevice_f32 and nrtClosestPointBatchDevice_f32 ALTERNATED call by call
(each timed by nrtLastTraverseMs, which waits for it), the median of --rounds calls of each and their ratio: the cost of carrying the
feature code and of the one normal fetch per query.  Beside it the time of a normals refresh at 1 M faces: the host wall time of
nrtGetFeatureNormals_f32 (vertex normals only) after an nrtRefit, which marks the normals stale, less that of a second call, which
finds them current and only downloads.
Writes profiles/sdf_probe.json and prints it as one JSON line.

    python tools/sdf_probe.py [--rounds 31] [--ramp 10] [--out profiles/sdf_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import torch

    import closest_probe
    from nanort_amd import BVHAccel, TriangleMesh, scenes

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--ramp", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--uniform", type=int, default=2000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdf_probe.json"))
    args = ap.parse_args()

    v, f = scenes.plane(1000, 500)
    nf = f.shape[0]
    acc = BVHAccel(np.float32)
    assert acc.Build(nf, TriangleMesh(v, f))
    sets = closest_probe.point_sets(acc, v, f, args.width, args.height, args.uniform)
    out = {"probe": "signed_distance", "mesh": "C3 plane(1000,500)", "tris": int(nf), "rounds": args.rounds, "ramp": args.ramp,
           "rocm": closest_probe.rocm_version(), "hip": torch.version.hip, "device": torch.cuda.get_device_name(0), "sets": {}}

    # the normals refresh: a refit to the same vertices marks them stale; the getter (vertex normals only: 12 MB down) derives them.
    # refresh = (stale call) - (current call), the median of five pairs
    vn = np.zeros((v.shape[0], 3), dtype=np.float32)
    get = acc._L.nrtGetFeatureNormals_f32
    stale, current = [], []
    for _ in range(5):
        acc.Refit(v)
        t0 = time.perf_counter()
        assert get(acc._h, None, vn.ctypes.data) == 0
        t1 = time.perf_counter()
        assert get(acc._h, None, vn.ctypes.data) == 0
        t2 = time.perf_counter()
        stale.append((t1 - t0) * 1e3)
        current.append((t2 - t1) * 1e3)
    out["normals_refresh_ms"] = {"stale_call_median": float(np.median(stale)), "current_call_median": float(np.median(current)),
                                 "refresh_median": float(np.median(np.asarray(stale) - np.asarray(current)))}

    for name, pts in sets.items():
        n = pts.shape[0]
        d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
        d_out = [torch.zeros((n * 32,), dtype=torch.uint8, device="cuda") for _ in range(2)]
        d_found = torch.zeros((n,), dtype=torch.uint8, device="cuda")
        times = {"signed": [], "unsigned": []}
        for r in range(args.ramp + args.rounds):
            for arm, call, buf in (("signed", acc.SignedDistanceBatchDevice, d_out[0]), ("unsigned", acc.ClosestPointBatchDevice, d_out[1])):
                call(d_pts, buf, d_found)
                t = acc.LastTraverseMs()  # (waits for the launch)
                if r >= args.ramp:
                    times[arm].append(t)
        torch.cuda.synchronize()
        a, b = d_out[0].cpu().numpy().reshape(n, 32), d_out[1].cpu().numpy().reshape(n, 32)
        row = {"n": int(n), "first_28_bytes_equal": bool(np.array_equal(a[:, :28], b[:, :28])),
               "inside": int((a[:, 31] & 0x80).astype(bool).sum())}
        for arm, t in times.items():
            t = np.asarray(t)
            row[arm] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "mqueries_per_s": float(n / np.median(t) / 1e3)}
        row["signed_over_unsigned"] = row["signed"]["median_ms"] / row["unsigned"]["median_ms"]
        out["sets"][name] = row
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()

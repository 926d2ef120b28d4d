#!/usr/bin/env python3
"""Wall time of setting a mesh from pageable host arrays (nrtSetMesh_f32) and from arrays already in HBM (nrtSetMeshDevice_f32),
alone and followed by nrtBuild_f32, on the same plane mesh (default 1000 x 500 cells = 1 M triangles).  Every timed call ends
synchronised (both set calls and nrtBuild return when their work is complete), so a host clock around it is the
application-visible time.  Warm-up, then the median of --reps alternating repetitions.  Prints one JSON line.

    python tools/time_set_mesh_device.py [--nx 1000 --ny 500 --reps 21 --warmup 5]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nanort_amd import capi, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=1000)
    ap.add_argument("--ny", type=int, default=500)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch

    L = capi.lib()
    v, f = scenes.plane(args.nx, args.ny)
    nv, nf = v.shape[0], f.shape[0]
    d_v, d_f = torch.from_numpy(v).cuda(), torch.from_numpy(f.view(np.int32)).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ctxs = []
    for _ in range(2):
        h = ctypes.c_void_p()
        assert L.nrtCreate(0, ctypes.byref(h)) == capi.NRT_OK, L.nrtLastError(None).decode()
        ctxs.append(h)
    host, dev = ctxs
    nn = ctypes.c_uint64(0)

    def set_host():
        assert L.nrtSetMesh_f32(host, v.ctypes.data, 12, f.ctypes.data, nf) == capi.NRT_OK, L.nrtLastError(host).decode()

    def set_dev():
        assert L.nrtSetMeshDevice_f32(dev, d_v.data_ptr(), nv, 12, d_f.data_ptr(), nf, stream) == capi.NRT_OK, L.nrtLastError(dev).decode()

    def build(h):
        assert L.nrtBuild_f32(h, None, None, ctypes.byref(nn)) == capi.NRT_OK, L.nrtLastError(h).decode()

    arms = {
        "set_mesh_host_ms": set_host,
        "set_mesh_device_ms": set_dev,
        "set_mesh_host_plus_build_ms": lambda: (set_host(), build(host)),
        "set_mesh_device_plus_build_ms": lambda: (set_dev(), build(dev)),
    }
    times = {k: [] for k in arms}
    for rep in range(args.warmup + args.reps):
        for k, fn in arms.items():  # (alternating: every arm sees the same drift of the machine)
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if rep >= args.warmup:
                times[k].append((t1 - t0) * 1e3)
    out = {"triangles": int(nf), "vertices": int(nv), "reps": args.reps, "warmup": args.warmup}
    for k, ts in times.items():
        out[k] = round(statistics.median(ts), 4)
        out[k.replace("_ms", "_min_ms")] = round(min(ts), 4)
    for h in ctxs:
        L.nrtDestroy(h)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Speed of the curve primitive (nrtSetCurves_f32 / nrtTraverseBatchCurvesDevice_f32) against the reference example's own Traverse
loop on the host of the same machine, for the same rays: the example's view (its camera at 1024 x 1024) of the fur fixture
(tests/golden/curves_fur.npz) and of the 3000-strand synthetic hair.

    python tools/curves_probe.py [--size 1024] [--launches 20] [--ref-lib PATH] [--out FILE.json]

GPU: rays and records stay in HBM; 3 warm-up launches, then `--launches` launches, each timed by the library's own completion
record (nrtLastTraverseMs: first wave's start to the post pass's end); median, min and max are reported.  Reference: the
unmodified examples/curves_primitive/main.cc under tests/ref_curves_shim.cc, one thread, as the example runs it; the shared
library is built where the reference tree exists (curves_fixture.ref_lib(out_dir)) and passed with --ref-lib; without it only the
GPU figures are printed.  With it the GPU also adopts the reference's tree and its records are compared with the reference's,
byte for byte, at the measured size."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import curves_fixture as cf  # noqa: E402
from nanort_amd import BVHAccel, CurveGeometry, scenes  # noqa: E402
from nanort_amd.wire import CURVE_HIT_F32  # noqa: E402


def gpu_row(cps, radii, rays, launches):
    import torch

    a = BVHAccel(np.float32)
    assert a.Build(radii.shape[0], CurveGeometry(cps, radii))
    build_ms = a.LastBuildMs()
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    d_hits = torch.empty(n * CURVE_HIT_F32.itemsize, dtype=torch.uint8, device="cuda")
    d_mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    ms = []
    for k in range(3 + launches):
        a.TraverseBatchDevice(d_rays, d_hits, d_mask)
        torch.cuda.synchronize()
        if k >= 3:
            ms.append(a.LastTraverseMs())
    ms = np.array(ms)
    return a, {"build_ms": build_ms, "kernel": a.LastKernelName(), "ms_median": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max()),
               "mrays_per_s": n / float(np.median(ms)) * 1e-3, "hit_fraction": float(d_mask.float().mean().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--ref-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rays = scenes.curves_camera_rays(args.size, args.size)
    n = rays.shape[0]
    ref = cf.load_ref(args.ref_lib) if args.ref_lib else None
    out = {"rays": n, "view": "%dx%d, the example's camera" % (args.size, args.size), "launches": args.launches, "rows": {}}
    for name, (cps, radii) in (("fur_400", cf.fur()), ("hair_3000", cf.hair(3000))):
        _, row = gpu_row(cps, radii, rays, args.launches)
        if ref is not None:
            r = cf.RefAccel(cps, radii, lib=ref)
            secs = []
            for _ in range(3):
                t0 = time.perf_counter()
                rh, rm = r.traverse(rays)
                secs.append(r.last_secs)
                assert time.perf_counter() - t0 >= r.last_secs
            row["reference_host_ms_median"] = float(np.median(secs)) * 1e3
            row["reference_host_mrays_per_s"] = n / float(np.median(secs)) * 1e-6
            row["gpu_over_reference"] = row["reference_host_ms_median"] / row["ms_median"]
            b = BVHAccel(np.float32)  # the reference's tree on the GPU: the same records, byte for byte
            b.SetMesh(CurveGeometry(cps, radii))
            b.SetTree(r.nodes, r.indices)
            h, m = b.TraverseBatch(rays)
            row["records_equal_reference_on_its_tree"] = bool(h.tobytes() == rh.tobytes() and np.array_equal(m, rm))
            r.close()
        out["rows"][name] = row
        print(name, json.dumps(row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()

"""Visibility masks on C3 — Plane(1000, 500), 1 M triangles, fp32, 1920x1080 objrender camera: primaries and their bounce rays,
everything resident in HBM.  Per ray set, in one process and over the same rays, three launches ALTERNATING round by round after a
ramp of untimed rounds (each launch timed by nrtLastTraverseMs, which waits for it):
  (a) nrtTraverseBatchMaskedDevice_f32 with all-ones words on both sides — the masked walk where nothing is hidden;
  (b) the same with a random half of the triangles hidden from the rays (prim word 0 or 1 per face, every ray carries 1);
  (c) the plain closest-hit call forced onto the literal binary walk (tunable wide = 0: k_traverse, the same loop without masks) —
      the yardstick, not the code under test.
(a)'s records must equal (c)'s byte for byte, which the probe checks before it times anything.  Writes profiles/masks_probe_c3.json
and prints it as one JSON line.

    python tools/masks_probe.py [--rounds 30] [--ramp 10] [--out profiles/masks_probe_c3.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from nanort_amd import BVHAccel, TriangleMesh, scenes

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--ramp", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masks_probe_c3.json"))
    args = ap.parse_args()

    v, f = scenes.plane(1000, 500)
    nf = f.shape[0]
    rng = np.random.default_rng(1)
    ones = np.full(nf, 0xFFFFFFFF, dtype=np.uint32)
    half = rng.integers(0, 2, size=nf).astype(np.uint32)  # bit 0 set on a random half of the faces

    # two accels over the same mesh (the build is deterministic: the same tree), so that alternating (a) and (b) sets no masks
    # between the launches; the literal walk runs on a third, whose tunable stays put
    acc_a, acc_b, acc_c = BVHAccel(np.float32), BVHAccel(np.float32), BVHAccel(np.float32)
    for a in (acc_a, acc_b, acc_c):
        assert a.Build(nf, TriangleMesh(v, f))
    acc_a.SetPrimMasks(ones)
    acc_b.SetPrimMasks(half)
    acc_c.SetTunable("wide", 0)

    cam = scenes.camera_rays(args.width, args.height)
    h, m = acc_a.TraverseBatch(cam)
    bounce = scenes.secondary_rays("bounce", v, f, cam, h, m)

    out = {"probe": "masks", "mesh": "C3 plane(1000,500)", "tris": int(nf), "image": "%dx%d" % (args.width, args.height), "rounds": args.rounds,
           "ramp": args.ramp, "hidden_share": float((half == 0).mean()), "rays": {}}
    for name, rays in (("primary", cam), ("bounce", bounce)):
        n = rays.shape[0]
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_one = torch.ones((n,), dtype=torch.int32, device="cuda")  # every ray carries the word 1
        d_hits = [torch.zeros((n * 16,), dtype=torch.uint8, device="cuda") for _ in range(3)]
        d_mask = [torch.zeros((n,), dtype=torch.uint8, device="cuda") for _ in range(3)]
        launches = (
            ("masked_all_visible", acc_a, lambda: acc_a.TraverseBatchMaskedDevice(d_rays, None, d_hits[0], d_mask[0])),
            ("masked_half_hidden", acc_b, lambda: acc_b.TraverseBatchMaskedDevice(d_rays, d_one, d_hits[1], d_mask[1])),
            ("literal", acc_c, lambda: acc_c.TraverseBatchDevice(d_rays, d_hits[2], d_mask[2])),
        )
        times = {k: [] for k, _, _ in launches}
        for r in range(args.ramp + args.rounds):
            for k, acc, launch in launches:
                launch()
                t = acc.LastTraverseMs()  # (waits for the launch)
                if r >= args.ramp:
                    times[k].append(t)
        torch.cuda.synchronize()
        assert acc_a.LastKernelName() == "nrt::k_traverse_masked<float>" and acc_c.LastKernelName() == "nrt::k_traverse<float>"
        assert torch.equal(d_hits[0], d_hits[2]) and torch.equal(d_mask[0], d_mask[2]), "all-ones masks: records differ from the literal walk's"
        row = {"n": int(n)}
        for k, _, _ in launches:
            t = np.asarray(times[k])
            row[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "grays_s": n / float(np.median(t)) / 1e6}
        row["masked_all_visible"]["hits"] = int(d_mask[0].sum())
        row["masked_half_hidden"]["hits"] = int(d_mask[1].sum())
        row["all_visible_over_literal"] = row["masked_all_visible"]["median_ms"] / row["literal"]["median_ms"]
        row["half_hidden_over_literal"] = row["masked_half_hidden"]["median_ms"] / row["literal"]["median_ms"]
        out["rays"][name] = row
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        fp.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()

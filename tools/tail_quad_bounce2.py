"""Tunable tail_quad on a SMALL batch: the second bounce wave of a config (rays generated from the bounce-1 hits; a launch that is
mostly ramp and tail), kernel ms by the launch's own stamps under each threshold, measured round-robin; records compared.

    python tools/tail_quad_bounce2.py C3 0 2 4 8 16 0
"""
import hashlib
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

import bench  # noqa: E402
from nanort_amd import scenes  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "C3"
ths = [int(x) for x in sys.argv[2:]] or [0, 4, 16, 0]
wl = bench.Workload(name, builds=1)
a = wl.accel
a.TraverseBatchDevice(wl.d_rays1, wl.d_hits1, wl.d_mask1)
a.TraverseBatchDevice(wl.d_rays2, wl.d_hits2, wl.d_mask2)
_, _, gh2, gm2 = wl.results()
rays3 = scenes.secondary_rays("bounce", wl.verts32, wl.faces, wl.rays2, gh2, gm2, pixel_base=7 * wl.n1)
n3 = rays3.shape[0]
d_rays = torch.from_numpy(rays3.view(np.uint8).copy()).cuda()
d_hits = torch.zeros(n3 * wl.HIT.itemsize, dtype=torch.uint8, device="cuda")
d_mask = torch.zeros(n3, dtype=torch.uint8, device="cuda")
for _ in range(100):  # (the device's clocks ramp over some tens of milliseconds of work)
    a.TraverseBatchDevice(d_rays, d_hits, d_mask)
ts, hs = [[] for _ in ths], [None] * len(ths)
for rnd in range(7):
    for k, tq in enumerate(ths):
        a.SetTunable("tail_quad", tq)
        for _ in range(5):
            a.TraverseBatchDevice(d_rays, d_hits, d_mask)
            ts[k].append(a.LastTraverseMs())
        if rnd == 0:
            torch.cuda.synchronize()
            hs[k] = hashlib.md5(d_hits.cpu().numpy().tobytes() + d_mask.cpu().numpy().tobytes()).hexdigest()
for k, tq in enumerate(ths):
    ms = float(np.median(ts[k]))
    print("%s bounce-2 (%d rays) tail_quad=%-2d  %.4f ms (min %.4f)  %.0f Mrays/s  same=%s" % (name, n3, tq, ms, min(ts[k]), n3 / ms / 1e3, hs[k] == hs[0]), flush=True)

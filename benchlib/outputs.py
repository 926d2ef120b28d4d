"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, as plain float arrays, so that two builds of the
library can be compared output for output (the inputs are synthetic and the same on every run with the same arguments)."""
import os

import numpy as np

BUDGET_BYTES = 60_000_000  # everything written, at most (64 MB allowed); larger waves are cut to a fixed sample of rays


def dump_outputs(out_dir, wl, bufs):
    """Both waves' hit records and hit flags as the timed path left them after its last step (N > 1: this rank's share), one array
    per field: DIR/<wave>_{t,u,v,prim_id,hit}.npy for <wave> = primary, bounce.  t / u / v keep the config's precision (float32;
    float64 for C5); prim_id (uint32, a miss is 0xFFFFFFFF) is written as float64, which holds every value exactly; hit is the 0 / 1
    flag as float32.  When the two waves would exceed BUDGET_BYTES, each wave is cut to a seeded sample of rays (the same on every
    run) and the sampled ray indices go to DIR/<wave>_ray.npy.  Returns {file name: elements}."""
    import torch

    torch.cuda.synchronize()
    d_h1, d_m1, d_h2, d_m2 = bufs
    waves = (("primary", d_h1, d_m1, wl.n1), ("bounce", d_h2, d_m2, wl.n2))
    per_ray = 3 * wl.rb + 8 + 4  # t, u, v + prim_id + hit
    cap = None
    if (wl.n1 + wl.n2) * per_ray > BUDGET_BYTES:
        cap = BUDGET_BYTES // (len(waves) * (per_ray + 8))  # (+ the float64 ray index of a sampled wave)
    real = np.float64 if wl.rb == 8 else np.float32
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for seed, (wave, d_h, d_m, n) in enumerate(waves):
        hits = d_h[: n * wl.HIT.itemsize].cpu().numpy().view(wl.HIT)
        mask = d_m[:n].cpu().numpy()
        arrays = {}
        if cap is not None and n > cap:
            idx = np.sort(np.random.default_rng(seed).choice(n, size=cap, replace=False))
            hits, mask = hits[idx], mask[idx]
            arrays["ray"] = idx.astype(np.float64)
        for f in ("t", "u", "v"):
            arrays[f] = hits[f].astype(real)
        arrays["prim_id"] = hits["prim_id"].astype(np.float64)
        arrays["hit"] = mask.astype(np.float32)
        for k, a in arrays.items():
            name = "%s_%s.npy" % (wave, k)
            np.save(os.path.join(out_dir, name), np.ascontiguousarray(a))
            written[name] = int(a.size)
    return written

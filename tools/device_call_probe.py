"""Host cost of one nrtTraverseBatchDevice_f32 call at a small batch: the time the call takes to return (nothing is waited for
inside the timed loop), median over rounds of 2000 calls, for the tree the script is started in (run it from the repository root)."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

from nanort_amd import BVHAccel, TriangleMesh, capi, scenes  # noqa: E402
from nanort_amd.wire import HIT_F32  # noqa: E402

v, f = scenes.plane(100, 50)
a = BVHAccel(np.float32)
assert a.Build(f.shape[0], TriangleMesh(v, f))
L = capi.lib()
out = {}
for n in (64, 4096):
    rays = np.ascontiguousarray(scenes.camera_rays(64, 64)[:n])
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    d_hits = torch.zeros(n * HIT_F32.itemsize, dtype=torch.uint8, device="cuda")
    d_mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    args = (a._h, d_rays.data_ptr(), n, None, d_hits.data_ptr(), d_mask.data_ptr(), s)
    fn = L.nrtTraverseBatchDevice_f32
    for _ in range(500):
        assert fn(*args) == 0
    torch.cuda.synchronize()
    per_call = []
    for _ in range(7):
        t0 = time.perf_counter()
        for _ in range(2000):
            fn(*args)
        per_call.append((time.perf_counter() - t0) / 2000 * 1e6)
        torch.cuda.synchronize()
    out["n=%d" % n] = round(float(np.median(per_call)), 3)
print("DEVICE_CALL_US " + json.dumps(out))

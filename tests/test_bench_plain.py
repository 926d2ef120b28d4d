"""A plain `bench.py` run (no --full): the headline figure only, exactly --steps timed steps, and with --dump-outputs the records
of the last timed step, which must be what the hot path computes for the same rays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--builds", "1",
                        "--dump-outputs", str(out_dir)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "Mrays/s" and out["dtype"] == "f32" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and out["value"] > 500.0
    # nothing beside the headline: those need --full
    assert out["roofline"] is None and out["cpu_baseline"] is None
    for k in ("configs", "next_rows", "also", "extras_file"):
        assert k not in out, k

    files = sorted(os.listdir(out_dir))
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64_000_000
    a = {f[:-4]: np.load(out_dir / f) for f in files}
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64), k
    from benchlib.workload import Workload
    from nanort_amd.wire import MISS_PRIM_ID

    wl = Workload("C3", builds=1)  # the same synthetic inputs; its set-up traces wave 1 once
    idx = a["primary_ray"].astype(np.int64)
    assert idx.size > 500_000 and np.all(np.diff(idx) > 0) and idx[-1] < wl.n1
    assert np.array_equal(a["primary_hit"], wl.mask1[idx].astype(np.float32))
    for f in ("t", "u", "v"):
        assert a["primary_" + f].tobytes() == wl.hits1[f][idx].tobytes(), f
    assert np.array_equal(a["primary_prim_id"], wl.hits1["prim_id"][idx].astype(np.float64))
    hit = a["primary_hit"] > 0
    assert hit.any() and np.all(a["primary_prim_id"][hit] < 1_000_000) and np.all(a["primary_prim_id"][~hit] == MISS_PRIM_ID)
    assert a["bounce_ray"].size > 0 and a["bounce_ray"][-1] < wl.n2 and a["bounce_hit"].size == a["bounce_ray"].size

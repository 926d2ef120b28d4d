"""The integer arithmetic of a traversal launch (nanort_amd/csrc/launch_plan.h: grid size, work distribution, overflow-stack
depth).  Hit records are bit-identical under every plan, so no parity test can see a slip in it: tests/cpp/launch_plan_check.cc
prints the plans and this compares them with literals worked out by hand from the expressions (one 64-ray
group per wave at a 16 % static share of a 1080p wave, 256 rays per wave at 75 %), and checks on random launches that the
static slices, the dynamic parts of the bands and the tail cover the batch exactly once."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_FIELDS = ("static_per_wave", "static_bands", "band_static", "dyn_per_band", "band_len", "dyn_banded", "tail_begin", "dyn_total",
               "dyn_per_part")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_check")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "nanort_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "launch_plan_check.cc"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert r.returncode == 0, r.stdout[-3000:]

    def ask(kind, rows):
        text = "".join("%s %s\n" % (kind, " ".join(str(int(x)) for x in row)) for row in rows)
        r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        out = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
        assert len(out) == len(rows)
        return out

    return ask


def plan(planner, rays, waves, parts, static_pct=16, static_bands=8, static_slice_groups=2, chunk=128):
    return dict(zip(PLAN_FIELDS, planner("plan", [(rays, waves, parts, static_pct, static_bands, static_slice_groups, chunk)])[0]))


def test_plan_of_a_1080p_wave_at_the_default_share(planner):
    assert plan(planner, 2073600, 5120, 8) == dict(
        static_per_wave=64, static_bands=1, band_static=327680, dyn_per_band=1745920, band_len=2073600, dyn_banded=1745920,
        tail_begin=2073600, dyn_total=1745920, dyn_per_part=218240)


def test_plan_of_a_1080p_wave_at_75_percent(planner):
    assert plan(planner, 2073600, 5120, 8, static_pct=75) == dict(
        static_per_wave=128, static_bands=2, band_static=655360, dyn_per_band=381440, band_len=1036800, dyn_banded=762880,
        tail_begin=2073600, dyn_total=762880, dyn_per_part=95360)


def test_plan_of_a_small_batch_has_no_static_share(planner):
    p = plan(planner, 1000, 16, 4)
    want = dict(static_per_wave=0, static_bands=0, band_len=0, dyn_banded=0, tail_begin=0, dyn_total=1000, dyn_per_part=128)
    assert {k: p[k] for k in want} == want


def test_grid_sizes(planner):
    rows = [(2073600, 256, 256, 5, 8), (1000, 256, 256, 5, 8), (2305, 256, 256, 5, 8)]  # rays, block, CUs, blocks per CU, partitions
    assert planner("grid", rows) == [(1280, 8, 160), (4, 4, 1), (16, 8, 2)]  # (the last: rounded up above the ten blocks needed)


def test_overflow_stack_levels(planner):
    assert planner("spill", [(20, 1, 12), (185, 0, 10), (8, 0, 32)]) == [(23,), (177,), (0,)]


def test_every_ray_is_handed_out_exactly_once(planner):
    rng = np.random.default_rng(20)
    n = 400
    rays = np.exp(rng.uniform(0.0, np.log(2.0 ** 31 - 1), n)).astype(np.int64).clip(1, 2 ** 31 - 1)
    rays[:4] = (1, 63, 2 ** 31 - 1, 2 ** 31 - 2)
    grids = planner("grid", [(r, 256, 256, rng.integers(1, 9), rng.integers(1, 17)) for r in rays])
    rows = [(r, 4 * g[0], g[1], rng.integers(0, 101), rng.integers(1, 65), rng.integers(1, 65), 32 * rng.integers(1, 33))
            for r, g in zip(rays, grids)]
    shared = 0
    for row, out in zip(rows, planner("plan", rows)):
        p = dict(zip(PLAN_FIELDS, out))
        r, waves, parts, chunk = row[0], row[1], row[2], row[6]
        assert p["static_bands"] * p["band_len"] + (r - p["tail_begin"]) == r, (row, p)
        assert p["band_len"] == p["band_static"] + p["dyn_per_band"], (row, p)
        assert p["band_static"] == p["static_per_wave"] * waves and p["static_per_wave"] % 64 == 0, (row, p)
        assert p["dyn_per_band"] % chunk == 0 and p["dyn_per_part"] % chunk == 0, (row, p)
        assert p["dyn_per_part"] * parts <= p["dyn_total"], (row, p)
        assert p["dyn_total"] == p["dyn_banded"] + (r - p["tail_begin"]) and p["dyn_banded"] == p["static_bands"] * p["dyn_per_band"], (row, p)
        assert p["tail_begin"] <= r and p["static_bands"] <= row[4], (row, p)
        shared += p["static_bands"] > 0
    assert 50 < shared < n - 50  # (both kinds of plan were drawn)

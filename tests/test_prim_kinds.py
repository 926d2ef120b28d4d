"""The table of primitive kinds and the host rule that goes with it (nanort_amd/csrc/prim_kinds.h): what the setters size their
uploads by, and into how many segments nrtSetCylinders cuts a cylinder for the builder.  A slip in either changes no hit record
(a cylinder is tested whole whatever its segments), so no parity test can see it: tests/cpp/prim_kinds_check.cc prints them and
this compares them with literals worked out by hand and, on random cylinders, with a numpy restatement of the expressions."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prim_kinds") / "prim_kinds_check")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "nanort_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "prim_kinds_check.cc"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert r.returncode == 0, r.stdout[-3000:]

    def run(text):
        r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        return [line.split() for line in r.stdout.splitlines()]

    return run


def fl(values):
    return " ".join("%.9g" % np.float32(x) for x in values)  # (nine digits carry a float exactly; "inf" / "nan" read back as such)


def count(ask, p0, p1, r0, r1, seg_radii=8, kmax=32):
    return int(ask("count %s %d %d\n" % (fl(list(p0) + list(p1) + [r0, r1]), seg_radii, kmax))[0][0])


def offsets(ask, ends, radii, seg_radii, split, limit):
    rows = "".join("%s\n" % fl(list(e.reshape(-1)) + list(r)) for e, r in zip(ends, radii))
    out = [int(x) for x in ask("offsets %d %d %d %d\n%s" % (len(radii), seg_radii, split, limit, rows))[0]]
    return out[0], out[1:]


def test_bytes_per_primitive_and_the_rest_of_the_table(ask):
    rows = ask("table\n")
    assert [r[0] for r in rows] == ["triangles", "spheres", "cylinders", "curves"]
    assert [(int(r[1]), int(r[2])) for r in rows] == [(12, 0), (12, 4), (24, 8), (48, 16)]  # position / radius bytes in fp32
    assert [int(r[3]) for r in rows] == [0, 1, 2, 4]  # positions per primitive (a mesh says how many vertices it has)
    assert [int(r[4]) for r in rows] == [1, 1, 0, 0]  # fp64
    assert [int(r[5]) for r in rows] == [0, 0, 0x40000000, 1 << 28]  # first count refused
    assert [(int(r[6]), int(r[7])) for r in rows] == [(0, 0), (1, 0), (1, 28), (1, 40)]  # post pass, its own record


def test_segment_counts_worked_out_by_hand(ask):
    o = (0.0, 0.0, 0.0)
    assert count(ask, (1, 2, 3), (1, 2, 3), 1.0, 1.0) == 1  # length 0
    assert count(ask, o, (100, 0, 0), 0.0, 0.0) == 1  # radius 0: a box
    assert count(ask, o, (np.inf, 0, 0), 1.0, 1.0) == 1  # not finite: whole
    assert count(ask, o, (0, np.nan, 0), 1.0, 1.0) == 1
    assert count(ask, o, (100, 0, 0), np.inf, 1.0) == 1
    assert count(ask, o, (80, 0, 0), 1.0, 0.5) == 10  # 80 / (8 x max(1, 0.5)) == 10 exactly
    assert count(ask, o, (np.nextafter(np.float32(80), np.float32(81)), 0, 0), 0.5, 1.0) == 11  # one ulp longer
    assert count(ask, o, (3, 4, 12), 0.5, 0.25, seg_radii=2) == 13  # |(3, 4, 12)| == 13, 13 / (2 x 0.5)
    assert count(ask, o, (7.5, 0, 0), 1.0, 1.0) == 1  # shorter than one piece
    assert count(ask, o, (248, 0, 0), 1.0, 1.0) == 31  # one below kmax
    assert count(ask, o, (256, 0, 0), 1.0, 1.0) == 32  # want == kmax
    assert count(ask, o, (1000, 0, 0), 1.0, 1.0) == 32  # want == 125: capped
    assert count(ask, o, (1000, 0, 0), 1.0, 1.0, kmax=1) == 1  # cyl_split = 1: never
    assert count(ask, o, (1000, 0, 0), 1.0, 1.0, seg_radii=1024, kmax=64) == 1


def test_second_pass_halves_the_pieces_when_the_total_reaches_the_limit(ask):
    ends = np.zeros((4, 2, 3), np.float32)
    ends[:, 1, 0] = 80.0  # want == 10 each
    radii = np.ones((4, 2), np.float32)
    assert offsets(ask, ends, radii, 8, 32, 64) == (40, [0, 10, 20, 30, 40])
    assert offsets(ask, ends, radii, 8, 32, 41) == (40, [0, 10, 20, 30, 40])  # (the total has to stay BELOW the limit)
    assert offsets(ask, ends, radii, 8, 8, 33) == (32, [0, 8, 16, 24, 32])  # capped at cyl_split = 8
    assert offsets(ask, ends, radii, 8, 8, 32) == (16, [0, 4, 8, 12, 16])  # 32 reaches the limit: at most 8 >> 1 pieces
    assert offsets(ask, ends, radii, 8, 8, 16)[0] == 0  # ... and if that does not fit either: no segments


def test_against_a_numpy_restatement_on_random_cylinders(ask):
    rng = np.random.default_rng(2024)
    n, seg_radii, split = 1000, 8, 32
    ends = rng.uniform(-1, 1, (n, 2, 3)).astype(np.float32)
    radii = (10.0 ** rng.uniform(-4, -0.5, (n, 2))).astype(np.float32)
    radii[::50] = 0.0
    ends[7::100, 1] = ends[7::100, 0]
    ends[11::200, 0, 2] = np.inf
    rr = np.maximum(radii[:, 0], radii[:, 1])
    d = ends[:, 1].astype(np.float64) - ends[:, 0].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        want = np.ceil(length / (np.float64(seg_radii) * rr.astype(np.float64)))
    cut = (rr > 0) & np.isfinite(length) & (length > 0)
    k = np.where(cut, np.clip(np.where(cut, want, 1.0), 1.0, float(split)), 1.0).astype(np.int64)
    assert k.min() == 1 and k.max() == split and len(set(k.tolist())) > 10  # (the scene exercises the rule)
    total, off = offsets(ask, ends, radii, seg_radii, split, 1 << 27)
    assert total == int(k.sum()) and off == np.concatenate([[0], np.cumsum(k)]).tolist()
    for i in (0, 7, 11, 50, 333, 999):
        assert count(ask, ends[i, 0], ends[i, 1], radii[i, 0], radii[i, 1], seg_radii, split) == int(k[i])

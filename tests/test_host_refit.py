"""BVHAccel::Refit of include/nanort.h on the host (no backend): tests/cpp/refit_host_check.cc builds on v0 and refits to
v1.  The refit boxes equal the numpy model (tests/refit_model.py) with the topology unchanged, and the per-ray Traverse on
the refit tree finds what the reference finds on a fresh v1 build: same hit flags and t, the named primitive verified at
every exact tie (helpers.assert_hits_match)."""
import os
import subprocess

import numpy as np
import pytest

from helpers import assert_hits_match
from nanort_amd import scenes
from nanort_amd.wire import hit_dtype, node_dtype, widen_rays
from refit_model import assert_boxes_equal, refit as model_refit, topology_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("refit_host")
    exe = str(d / "refit_host_check")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I", INC, os.path.join(ROOT, "tests", "cpp", "refit_host_check.cc"),
                        "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe, d


def write_mesh(path, v, f):
    with open(path, "wb") as fp:
        fp.write(np.array([v.shape[0], f.shape[0]], dtype=np.uint32).tobytes())
        fp.write(np.ascontiguousarray(v, dtype=np.float32).tobytes())
        fp.write(np.ascontiguousarray(f, dtype=np.uint32).tobytes())


def moved(v, kind):
    w = v.astype(np.float64).copy()
    if kind == "wave":
        w[:, 1] += 0.15 * np.sin(4.0 * w[:, 0]) * np.cos(3.0 * w[:, 2])
    elif kind == "translate":
        w += (0.3, -0.2, 0.1)
    elif kind == "scale":
        c = w.mean(axis=0)
        w = (w - c) * (2.0, 0.5, -1.0) + c
    return w.astype(np.float32)


@pytest.mark.parametrize("real", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["wave", "translate", "scale"])
def test_host_refit_equals_the_model_and_traces_like_a_fresh_build(driver, oracle, c1_mesh, real, kind):
    exe, d = driver
    v0, f = c1_mesh
    v0 = v0.astype(np.float32)
    v1 = moved(v0, kind)
    rays = scenes.camera_rays(96, 64)
    m0, m1, rp, out = (str(d / x) for x in ("m0.bin", "m1.bin", "rays.bin", "out_%s_%s.bin" % (kind, np.dtype(real).name)))
    write_mesh(m0, v0, f)
    write_mesh(m1, v1, f)
    with open(rp, "wb") as fp:
        fp.write(np.array([rays.shape[0]], dtype=np.uint64).tobytes())
        fp.write(rays.tobytes())
    r = subprocess.run([exe, "f64" if real == np.float64 else "f32", m0, m1, rp, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "driver exit %d: %s" % (r.returncode, r.stdout)
    nd, hd = node_dtype(real), hit_dtype(real)
    raw = open(out, "rb").read()
    nn = int(np.frombuffer(raw, np.uint64, 1, 0)[0])
    o = 8
    before = np.frombuffer(raw, nd, nn, o)
    o += nn * nd.itemsize
    after = np.frombuffer(raw, nd, nn, o)
    o += nn * nd.itemsize
    idx = np.frombuffer(raw, np.uint32, f.shape[0], o)
    o += 4 * f.shape[0]
    hits = np.frombuffer(raw, hd, rays.shape[0], o)
    o += rays.shape[0] * hd.itemsize
    mask = np.frombuffer(raw, np.uint8, rays.shape[0], o)
    V0, V1 = v0.astype(real), v1.astype(real)
    assert_boxes_equal(before, model_refit(before, idx, V0, f), "the build's boxes")
    assert topology_bytes(after) == topology_bytes(before), "refit changed the topology"
    assert_boxes_equal(after, model_refit(before, idx, V1, f))
    # per-ray Traverse on the refit tree == the reference on a fresh v1 build (exact t; ties verified)
    wr = widen_rays(rays) if real == np.float64 else rays
    onodes, oidx, _ = oracle.build(V1, f)
    oh, om = oracle.traverse(onodes, oidx, V1, f, wr)
    hits = hits.copy()
    hits["t"][mask == 0] = oh["t"][mask == 0]  # (a miss leaves the record untouched: compare the hit flags only)
    hits["prim_id"][mask == 0] = oh["prim_id"][mask == 0]
    hits["u"][mask == 0] = oh["u"][mask == 0]
    hits["v"][mask == 0] = oh["v"][mask == 0]
    assert mask.any()
    assert_hits_match(oh, om, hits, mask, oracle, onodes, oidx, V1, f, wr)


def test_host_refit_of_a_malformed_tree_is_refused_and_changes_nothing(tmp_path, c1_mesh):
    exe = str(tmp_path / "refit_host_check_ser")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-DNANORT_ENABLE_SERIALIZATION", "-I", INC,
                        os.path.join(ROOT, "tests", "cpp", "refit_host_check.cc"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    v, f = c1_mesh
    mesh = str(tmp_path / "m.bin")
    write_mesh(mesh, v.astype(np.float32), f)
    r = subprocess.run([exe, "malformed", mesh], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, "driver exit %d: %s" % (r.returncode, r.stdout)


class _NoLibrary:
    """Stands in for the C library: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) although the input was refused" % name)


def _offline_accel(real, nv):
    """A BVHAccel that never opened a context, holding a triangle mesh of nv vertices (no GPU needed)."""
    from nanort_amd import BVHAccel, TriangleMesh

    a = BVHAccel.__new__(BVHAccel)
    a.real = np.dtype(real)
    a._s = "f32" if a.real == np.float32 else "f64"
    a._L = _NoLibrary()
    a._h = None
    a.device = 0
    f = np.array([[0, 1, nv - 1]], np.uint32)
    a._mesh = TriangleMesh(np.zeros((nv, 3), real), f)
    return a


@pytest.mark.parametrize("real", [np.float32, np.float64], ids=["f32", "f64"])
def test_short_vertex_arrays_are_refused_before_the_library_reads_them(real):
    a = _offline_accel(real, 100)
    with pytest.raises(ValueError):
        a.Refit(np.zeros((99, 3), real))
    with pytest.raises(ValueError):
        a.Refit(np.zeros((99, 4), real))
    with pytest.raises(ValueError):  # explicit stride: 100 rows of 16 bytes need 99 * 16 + 12
        a.Refit(np.zeros(99 * 4 + 2, real), vertex_stride_bytes=4 * np.dtype(real).itemsize)
    with pytest.raises(ValueError):
        a.Refit(np.zeros((100, 2), real))
    torch = pytest.importorskip("torch")
    tdt = torch.float32 if real == np.float32 else torch.float64
    with pytest.raises(ValueError):  # (checked before the device, so this runs on a CPU tensor)
        a.RefitDevice(torch.zeros((99, 3), dtype=tdt))
    with pytest.raises(ValueError):  # a strided view of too few rows
        a.RefitDevice(torch.zeros((99, 4), dtype=tdt)[:, :3])
    with pytest.raises(ValueError):  # enough rows, but not on the accel's device
        a.RefitDevice(torch.zeros((100, 3), dtype=tdt))

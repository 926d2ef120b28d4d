"""Which kernel a traversal launch runs (api_query.hip: the walk chosen from the context's state, its tunables and the trace options).
Hit records are bit-identical under every variant, so the parity tests cannot see a wrong choice: this pins nrtLastKernelName
per configuration — `nrt::k_traverse_wide<T, STACK, STATS, KIND, PLAIN, CLOCK, WIDTH, ORDER>` — on the C1 mesh with a 96 x 64
camera wave, and walks one context through every primitive kind: at each stage it launches the kernel and returns the records
of a fresh context holding the same stage (the context's cached launch geometry is keyed by what selects the kernel)."""
import ctypes

import numpy as np
import pytest

from helpers import assert_hits_identical
from nanort_amd import BVHAccel, CylinderGeometry, SphereGeometry, TriangleMesh, capi, scenes
from nanort_amd.wire import default_trace_options, widen_rays

pytestmark = pytest.mark.gpu

WIDE = "nrt::k_traverse_wide<%s>"
DEFAULT_F32 = WIDE % "float, 12, false, 0, true, false, 4, 2"
# (the sphere and cylinder names: what the library printed for these two sets at the commit before the launch path was
# restructured — custom primitives walk two levels per step with the id tests kept)
SPHERES_F32 = WIDE % "float, 12, false, 1, false, false, 4, 0"
CYLINDERS_F32 = WIDE % "float, 12, false, 2, false, false, 4, 0"

# (id, precision, tunables set before the build, cull_back_face, expected name)
CONFIGS = [
    ("f32_default", np.float32, {}, False, DEFAULT_F32),
    ("f32_cull", np.float32, {}, True, WIDE % "float, 12, false, 0, false, false, 4, 2"),
    ("order4", np.float32, {"order4": 1}, False, WIDE % "float, 12, false, 0, true, false, 4, 3"),
    ("no_leaf_compact", np.float32, {"leaf_compact": 0}, False, WIDE % "float, 12, false, 0, true, false, 4, 0"),
    ("no_leaf_compact_order4", np.float32, {"leaf_compact": 0, "order4": 1}, False, WIDE % "float, 12, false, 0, true, false, 4, 1"),
    ("wide4_big_forced", np.float32, {"wide4_big": 2}, False, WIDE % "float, 12, false, 0, true, false, 4, 6"),
    ("no_wide4", np.float32, {"wide4": 0}, False, WIDE % "float, 10, false, 0, true, false, 2, 0"),
    ("f64_default", np.float64, {}, False, WIDE % "double, 10, false, 0, true, false, 2, 0"),
    ("f64_cull", np.float64, {}, True, WIDE % "double, 10, false, 0, false, false, 2, 0"),
    ("no_wide", np.float32, {"wide": 0}, False, "nrt::k_traverse<float>"),
    # (the rows below: what the library printed at the commit before the kernels were put into one table)
    ("wide4_big_forced_cull", np.float32, {"wide4_big": 2}, True, WIDE % "float, 12, false, 0, false, false, 4, 6"),
    ("wide4_big_forced_no_leaf_compact", np.float32, {"wide4_big": 2, "leaf_compact": 0}, False, WIDE % "float, 12, false, 0, true, false, 4, 4"),
    ("wide_stack_8", np.float32, {"wide_stack": 8}, False, WIDE % "float, 8, false, 0, false, false, 2, 0"),
    ("wide_stack_12", np.float32, {"wide_stack": 12}, False, WIDE % "float, 12, false, 0, false, false, 2, 0"),
    ("wide_stack_16", np.float32, {"wide_stack": 16}, False, WIDE % "float, 16, false, 0, false, false, 2, 0"),
]
# custom primitives built with wide4 = 0 walk one level per step on ten LDS entries
ONE_LEVEL_CUSTOM = {"spheres": WIDE % "float, 10, false, 1, false, false, 2, 0", "cylinders": WIDE % "float, 10, false, 2, false, false, 2, 0"}


@pytest.fixture(scope="module")
def rays():
    return scenes.camera_rays(96, 64)


def for_precision(rays, real):
    return widen_rays(rays) if real == np.float64 else rays


def built(real, mesh, tunables=()):
    a = BVHAccel(real)
    for k, v in dict(tunables).items():
        a.SetTunable(k, v)  # (before the build: wide4 takes effect with the next tree)
    assert a.Build(mesh.num_faces, mesh)
    return a


@pytest.fixture(scope="module")
def reference_records(c1_mesh, rays):
    """The default walk's records per precision: every variant must return exactly these (order4 = 1 aside)."""
    v, f = c1_mesh
    out = {}
    for real in (np.float32, np.float64):
        a = built(real, TriangleMesh(v.astype(real), f))
        out[np.dtype(real)] = a.TraverseBatch(for_precision(rays, real))
    return out


@pytest.mark.parametrize("real,tunables,cull,want", [c[1:] for c in CONFIGS], ids=[c[0] for c in CONFIGS])
def test_kernel_name_per_configuration(c1_mesh, rays, reference_records, real, tunables, cull, want):
    v, f = c1_mesh
    a = built(real, TriangleMesh(v.astype(real), f), tunables)
    opt = None
    if cull:
        opt = default_trace_options()
        opt["cull_back_face"] = 1
    h, m = a.TraverseBatch(for_precision(rays, real), opt)
    print(a.LastKernelName())
    assert a.LastKernelName() == want
    assert m.any()
    if not cull and not tunables.get("order4"):
        assert_hits_identical(*reference_records[np.dtype(real)], h, m)


def test_occlusion_and_multihit_kernels(c1_mesh, rays, reference_records):
    v, f = c1_mesh
    a = built(np.float32, TriangleMesh(v.astype(np.float32), f))
    occ = a.OccludedBatch(rays)
    print(a.LastKernelName())
    assert a.LastKernelName() == DEFAULT_F32  # an occlusion query is a runtime flag of the closest-hit kernel
    assert np.array_equal(occ, reference_records[np.dtype(np.float32)][1])
    mh, cnt = a.MultiHitTraverseBatch(rays, 4)
    print(a.LastKernelName())
    assert a.LastKernelName() == "nrt::k_traverse_multihit<float>"
    assert np.array_equal(cnt > 0, occ == 1)
    h, m = a.TraverseBatch(rays)
    assert a.LastKernelName() == DEFAULT_F32
    assert_hits_identical(*reference_records[np.dtype(np.float32)], h, m)


def stage_geometry(c1_mesh, rays):
    """Per stage: the primitives, the rays that see them, the kernel that walks them."""
    v, f = c1_mesh
    particle = scenes.particle_camera_rays(96, 64)
    sc, sr = scenes.random_spheres(300)
    cv, cr = scenes.random_cylinders(257)
    return {
        "triangles": (TriangleMesh(v.astype(np.float32), f), rays, DEFAULT_F32),
        "spheres": (SphereGeometry(sc, sr), particle, SPHERES_F32),
        "cylinders": (CylinderGeometry(cv, cr), particle, CYLINDERS_F32),
    }


def assert_same_records(got, want):
    assert_hits_identical(got[0], got[1], want[0], want[1])
    if "normal" in (got[0].dtype.names or ()):  # the cylinder record's fifth field
        assert got[0]["normal"].tobytes() == want[0]["normal"].tobytes()


@pytest.mark.parametrize("kind", sorted(ONE_LEVEL_CUSTOM))
def test_custom_primitives_without_wide4(c1_mesh, rays, kind):
    g, r, _ = stage_geometry(c1_mesh, rays)[kind]
    a = built(np.float32, g, {"wide4": 0})
    got = a.TraverseBatch(r)
    print(a.LastKernelName())
    assert a.LastKernelName() == ONE_LEVEL_CUSTOM[kind]
    assert got[1].any()
    assert_same_records(got, built(np.float32, g).TraverseBatch(r))


def test_one_context_through_every_kind_equals_fresh_contexts(c1_mesh, rays):
    """fp32 triangles -> (fp64 triangles) -> spheres -> cylinders -> fp32 triangles on ONE context.  A context keeps the
    precision of its first primitives (nrtSetMesh_f64 on it: NRT_ERR_PRECISION, nothing changed), so the fp64 stage asserts
    that refusal and that the context still answers as the fp32 stage did; every other stage equals a fresh context's records
    and kernel."""
    geo = stage_geometry(c1_mesh, rays)
    fresh = {}
    for kind, (g, r, want) in geo.items():
        b = built(np.float32, g)
        fresh[kind] = (b.TraverseBatch(r), b.LastKernelName())
        print(kind, fresh[kind][1])
        assert fresh[kind][0][1].any()
    assert {k: fresh[k][1] for k in geo} == {k: geo[k][2] for k in geo}
    one = BVHAccel(np.float32)
    for stage in ("triangles", "f64", "spheres", "cylinders", "triangles"):
        if stage == "f64":
            v64 = np.ascontiguousarray(c1_mesh[0], dtype=np.float64)
            faces = np.ascontiguousarray(c1_mesh[1], dtype=np.uint32)
            st = one._L.nrtSetMesh_f64(one._h, v64.ctypes.data_as(ctypes.c_void_p), 24, faces.ctypes.data_as(ctypes.c_void_p), faces.shape[0])
            assert st == capi.NRT_ERR_PRECISION
            stage = "triangles"  # (still what the context holds)
        else:
            assert one.Build(geo[stage][0].num_faces, geo[stage][0])
        got = one.TraverseBatch(geo[stage][1])
        assert one.LastKernelName() == fresh[stage][1], stage
        assert_same_records(got, fresh[stage][0])


def test_batch_tables_are_checked_batch_by_batch_by_both_entry_points(c1_mesh, rays):
    """nrtTraverseBatches and nrtTraverseBatchesDevice share one check of their tables: per non-empty batch its rays, then an
    occlusion batch's flag array or a closest-hit batch's record array.  With two faulty batches the first batch's fault is the
    one reported, under the entry point's own name (the tables are refused before any pointer in them is used)."""
    v, f = c1_mesh
    a = built(np.float32, TriangleMesh(v.astype(np.float32), f))
    r = np.ascontiguousarray(rays[:8])
    tables = dict(rays=(ctypes.c_void_p * 2)(r.ctypes.data, r.ctypes.data), counts=(ctypes.c_uint64 * 2)(8, 8),
                  hits=(ctypes.c_void_p * 2)(None, None), masks=(ctypes.c_void_p * 2)(None, None), flags=(ctypes.c_uint32 * 2)(0, 1))
    t = tables
    assert a._L.nrtTraverseBatches_f32(a._h, 2, t["rays"], t["counts"], None, t["hits"], t["masks"], t["flags"]) == capi.NRT_ERR_INVALID
    assert a._L.nrtLastError(a._h).decode() == "nrtTraverseBatches: batch 0 has no hit array"
    assert a._L.nrtTraverseBatchesDevice_f32(a._h, 2, t["rays"], t["counts"], None, t["hits"], t["masks"], t["flags"], None) == capi.NRT_ERR_INVALID
    assert a._L.nrtLastError(a._h).decode() == "nrtTraverseBatchesDevice: batch 0 has no hit array"
    t["flags"][0], t["flags"][1] = 1, 0  # now batch 0 is the occlusion batch without flags
    assert a._L.nrtTraverseBatches_f32(a._h, 2, t["rays"], t["counts"], None, t["hits"], t["masks"], t["flags"]) == capi.NRT_ERR_INVALID
    assert a._L.nrtLastError(a._h).decode() == "nrtTraverseBatches: occlusion batch 0 has no flag array"
    assert a._L.nrtTraverseBatchesDevice_f32(a._h, 2, t["rays"], t["counts"], None, t["hits"], t["masks"], t["flags"], None) == capi.NRT_ERR_INVALID
    assert a._L.nrtLastError(a._h).decode() == "nrtTraverseBatchesDevice: occlusion batch 0 has no flag array"

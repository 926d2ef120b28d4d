"""The second trip of every capped grid and pieced host loop (tests/size_thresholds.py names the caps; test_size_thresholds.py pins
them to the sources).  Several kernels and host loops run a fixed number of workgroups or fixed-size pieces and cover the rest by
looping; every case here is sized from those caps, asserts from its own data that it crosses its cap, and compares every record
with a CPU restatement or numpy model, never with the library's own answer at a smaller size (B5 also holds the device-fed
build to the host-fed one byte for byte, the contract of nrtSetMeshDevice, beside the oracle on the tree it built):

  B1  k_refit_leaves past 262 144 list entries, on built triangle trees (Refit, RefitDevice)
  B2  the same leaf pass for spheres (RefitPrims)
  B3  k_plan_expand / k_refit_branches past 262 144 branches on one level, on an adopted complete binary tree
  B4  k_sphere_uv / k_cylinder_post / k_curve_post past 524 288 rays (host and Device forms), and the occlusion query at that size
  B5  k_max_index past 2 097 152 index words (BuildDevice, and its refusal)
  B6  the pipelined host path of nrtTraverseBatch* (page-locked buffers, 2^19-ray pieces, two staging slots)

Rays are a base set of B = 4093 (prime) tiled to the size; the expected records are the restatement's for the base set, tiled the
same way, so a record left unwritten, written from a stale slot or written at another offset cannot match.  Device output buffers
start as 0xA5 bytes."""

import numpy as np
import pytest

import curves_fixture as cf
import refit_prims_model
import size_thresholds as sz
import sphere_fixture
from helpers import assert_hits_identical
from nanort_amd import BVHAccel, CurveGeometry, CylinderGeometry, SphereGeometry, TriangleMesh, scenes
from nanort_amd.capi import NRT_ERR_INVALID, NRT_ERR_PRECISION, NRT_OK, NrtError
from nanort_amd.wire import CURVE_HIT_F32, CYL_HIT_F32, HIT_F32, default_build_options, hit_dtype, ray_dtype, widen_rays
from oracle import bindings as ob
from refit_model import assert_boxes_equal, refit as model_refit, topology_bytes

pytestmark = pytest.mark.gpu

FILL = 0xA5
SENTINEL = 0xFFFFFFFF


def _sfx(real):
    return "f32" if np.dtype(real) == np.float32 else "f64"


def to_device(a):
    """A numpy array (plain or of records) as a flat uint8 tensor on the GPU."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def filled(nbytes, pinned=False):
    """An output buffer of 0xA5 bytes: on the device, or page-locked on the host."""
    import torch

    if pinned:
        t = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        t.fill_(FILL)
        assert t.is_pinned()
        return t
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")


def camera_base(real):
    """B rays of the objrender camera over its whole 96 x 64 image."""
    r = sz.cut(scenes.camera_rays(96, 64))
    return r if np.dtype(real) == np.float32 else widen_rays(r)


def hits_and_misses(mask):
    return 0 < int(mask.sum()) < mask.shape[0]


# ---- B1: the leaf list past the cap, built triangle trees ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plane_300k():
    return scenes.plane(400, 375)  # 300 000 triangles; with min_leaf_primitives = 1 one leaf each


@pytest.mark.parametrize("form", ["f32", "f64", "f32_device"])
def test_b1_refit_of_a_built_tree_with_more_leaves_than_one_grid_trip(oracle, plane_300k, form):
    import torch

    real = np.float64 if form == "f64" else np.float32
    v32, f = plane_300k
    v = np.ascontiguousarray(v32.astype(real))
    bo = default_build_options(real)
    bo["min_leaf_primitives"] = 1
    a = BVHAccel(real)
    assert a.Build(f.shape[0], TriangleMesh(v, f), bo)
    n0, i0 = a.GetTree()
    leaves = sz.reachable_leaves(n0)
    assert leaves > sz.REFIT_CAP and sz.crossing_trips(leaves, sz.REFIT_CAP) >= 2, "%d reachable leaves: the leaf pass takes one trip" % leaves
    assert sz.widest_level(n0) < sz.REFIT_CAP  # (the per-level loops take one trip here: case B3 is theirs)
    rng = np.random.default_rng(11)
    v1 = (v + rng.normal(scale=1e-3, size=v.shape)).astype(real)
    rays = camera_base(real)

    def refit(w):
        if form == "f32_device":
            side = torch.cuda.Stream()
            d_v = torch.from_numpy(w).cuda()
            torch.cuda.synchronize()
            a.RefitDevice(d_v, stream=side)
            side.synchronize()  # (d_v stays unchanged until the stream has reached the refit)
        else:
            a.Refit(w)

    refit(v1)
    n1, i1 = a.GetTree()
    assert topology_bytes(n1) == topology_bytes(n0), "refit changed flag / axis / data"
    assert i1.tobytes() == i0.tobytes(), "refit changed the index array"
    assert_boxes_equal(n1, model_refit(n0, i0, v1, f))
    oh, om = oracle.traverse(n1, i1, v1, f, rays)  # (the re-derived leaf and two-level records at this size)
    assert hits_and_misses(om)
    h, m = a.TraverseBatch(rays)
    assert_hits_identical(oh, om, h, m)
    refit(v)  # back: the boxes of the build return
    n2, i2 = a.GetTree()
    assert topology_bytes(n2) == topology_bytes(n0) and i2.tobytes() == i0.tobytes()
    assert_boxes_equal(n2, model_refit(n0, i0, v, f))
    assert_boxes_equal(n2, n0, "boxes after the refit back")
    a.close()


# ---- B2: the leaf list past the cap, spheres -----------------------------------------------------------------------------------
def test_b2_refit_of_a_sphere_tree_with_more_leaves_than_one_grid_trip():
    n = 300000
    c, r = scenes.random_spheres(n)
    bo = default_build_options(np.float32)
    bo["min_leaf_primitives"] = 1
    a = BVHAccel(np.float32)
    assert a.Build(n, SphereGeometry(c, r), bo)
    n0, i0 = a.GetTree()
    leaves = sz.reachable_leaves(n0)
    assert leaves > sz.REFIT_CAP, "%d reachable leaves: the leaf pass takes one trip" % leaves
    rng = np.random.default_rng(12)
    c1 = (c + rng.normal(scale=0.02, size=c.shape)).astype(np.float32)
    r1 = (r * np.float32(0.5)).astype(np.float32)
    a.RefitPrims(c1, r1)
    n1, i1 = a.GetTree()
    assert topology_bytes(n1) == topology_bytes(n0) and i1.tobytes() == i0.tobytes()
    assert_boxes_equal(n1, refit_prims_model.refit("spheres", n0, i0, c1, r1))
    rays = sz.cut(sphere_fixture.rays())
    oh, om = ob.SphereOracle().traverse(n1, i1, c1, r1, rays)
    assert int(om.sum()) > 0
    h, m = a.TraverseBatch(rays)
    SPHERES.same(h, m, oh, om)
    assert np.array_equal(a.OccludedBatch(rays), om)
    a.close()


# ---- B3: one level past the cap, an adopted tree ---------------------------------------------------------------------------------
def test_b3_refit_of_an_adopted_tree_with_a_level_wider_than_one_grid_trip(oracle):
    v, f = scenes.plane(1024, 512)
    assert f.shape[0] == 1 << 20
    nodes, idx = sz.balanced_tree(1 << 20, np.float32, v, f)
    widest = sz.widest_level(nodes)
    assert widest > sz.REFIT_CAP and sz.crossing_trips(widest, sz.REFIT_CAP) >= 2, "widest level: %d branches" % widest
    assert sz.reachable_leaves(nodes) > sz.REFIT_CAP
    a = BVHAccel(np.float32)
    a.SetMesh(TriangleMesh(v, f))
    a.SetTree(nodes, idx)
    rays = camera_base(np.float32)
    w = v.astype(np.float64)
    w[:, 2] += 0.3 * np.sin(0.9 * w[:, 0]) * np.cos(0.7 * w[:, 1])
    w[:, 0] += 0.125
    v1 = w.astype(np.float32)

    def check(want, verts, what, both=True):
        got, gi = a.GetTree()
        assert topology_bytes(got) == topology_bytes(want), "%s: refit changed flag / axis / data" % what
        assert gi.tobytes() == idx[:gi.shape[0]].tobytes(), "%s: refit changed the index array" % what
        assert_boxes_equal(got, want, "boxes (%s)" % what)
        oh, om = oracle.traverse(got, gi, verts, f, rays)
        assert hits_and_misses(om) or not both, what
        h, m = a.TraverseBatch(rays)
        assert_hits_identical(oh, om, h, m)

    a.Refit(v1)  # plans the tree: k_plan_expand over every level, then k_refit_branches
    check(model_refit(nodes, idx, v1, f), v1, "first refit")
    a.Refit(v)  # the cached plan
    check(nodes, v, "second refit")  # (balanced_tree's boxes are the model's over v)
    small, sidx = sz.balanced_tree(1 << 10, np.float32, v, f)  # over the first 1024 faces of the same mesh
    a.SetTree(small, sidx)  # drops the plan
    a.Refit(v1)
    check(model_refit(small, sidx, v1, f), v1, "refit of the small tree", both=False)  # (a strip of the plane: the camera may miss it)
    a.close()


# ---- B4: the post passes past the cap ----------------------------------------------------------------------------------------------
class SPHERES:
    hit = HIT_F32

    @staticmethod
    def geometry():
        return SphereGeometry(*sphere_fixture.scene())

    @staticmethod
    def rays():
        return sz.cut(sphere_fixture.rays())

    @staticmethod
    def restate(nodes, idx, rays):
        c, r = sphere_fixture.scene()
        return ob.SphereOracle().traverse(nodes, idx, c, r, rays)

    @staticmethod
    def same(h, m, oh, om):
        """t, prim_id and the flags bit for bit; u, v (atan2 / acos in the reference's PostTraversal) within test_gpu_spheres.check's 1e-6."""
        assert np.array_equal(m, om), "hit flags differ at %s" % np.nonzero(m != om)[0][:8]
        assert np.ascontiguousarray(h["t"]).tobytes() == np.ascontiguousarray(oh["t"]).tobytes(), "t differs at %s" % np.nonzero(h["t"] != oh["t"])[0][:8]
        assert np.array_equal(h["prim_id"], oh["prim_id"]), "prim_id differs at %s" % np.nonzero(h["prim_id"] != oh["prim_id"])[0][:8]
        du, dv = np.max(np.abs(h["u"] - oh["u"]), initial=0.0), np.max(np.abs(h["v"] - oh["v"]), initial=0.0)
        print("spheres: max |u - u'| = %g, max |v - v'| = %g" % (du, dv))
        assert du <= 1e-6 and dv <= 1e-6, (du, dv)


class CYLINDERS:
    hit = CYL_HIT_F32
    test_cap = True

    @classmethod
    def geometry(cls):
        v, r = scenes.random_cylinders(sphere_fixture.N_CYLINDERS)
        return CylinderGeometry(v, r, test_cap=cls.test_cap)

    @staticmethod
    def rays():
        return sz.cut(sphere_fixture.rays())

    @classmethod
    def restate(cls, nodes, idx, rays):
        v, r = scenes.random_cylinders(sphere_fixture.N_CYLINDERS)
        return ob.CylinderOracle().traverse(nodes, idx, v, r, rays, test_cap=cls.test_cap)

    @staticmethod
    def same(h, m, oh, om):
        assert np.array_equal(m, om), "hit flags differ at %s" % np.nonzero(m != om)[0][:8]
        for k in ("t", "u", "v", "prim_id", "normal"):
            assert np.ascontiguousarray(h[k]).tobytes() == np.ascontiguousarray(oh[k]).tobytes(), k
        assert h.tobytes() == oh.tobytes()


class CYLINDERS_NO_CAP(CYLINDERS):
    test_cap = False


class CURVES:
    hit = CURVE_HIT_F32

    @staticmethod
    def geometry():
        return CurveGeometry(*cf.scene("fur"))

    @staticmethod
    def rays():
        return sz.cut(cf.all_rays())

    @staticmethod
    def restate(nodes, idx, rays):
        cps, radii = cf.scene("fur")
        return cf.model_traverse(nodes, idx, cps, radii, rays, 4)

    @staticmethod
    def same(h, m, oh, om):
        assert np.array_equal(m, om), "hit flags differ at %s" % np.nonzero(m != om)[0][:8]
        assert h.dtype == CURVE_HIT_F32 and h.tobytes() == oh.tobytes(), "records differ at %s" % np.nonzero(h != oh)[0][:8]


KINDS = {"spheres": SPHERES, "cylinders_cap": CYLINDERS, "cylinders_nocap": CYLINDERS_NO_CAP, "curves": CURVES}
_worlds = {}


def world(kind):
    """(kind's class, accel, n rays tiled from the base, the restatement's records and flags tiled the same way), once per kind."""
    if kind not in _worlds:
        K = KINDS[kind]
        g = K.geometry()
        a = BVHAccel(np.float32)
        assert a.Build(g.num_faces, g)
        nodes, idx = a.GetTree()
        base = K.rays()
        assert base.shape[0] == sz.B
        oh, om = K.restate(nodes, idx, base)
        assert hits_and_misses(om), "%s: %d of %d base rays hit" % (kind, int(om.sum()), om.shape[0])
        n = sz.POST_PASS_N
        assert n > sz.POST_PASS_CAP and n - sz.POST_PASS_CAP >= 2 * sz.B  # the second trip holds every base ray, hits and misses, twice
        _worlds[kind] = (K, a, sz.tiled(base, n), sz.tiled(oh, n), sz.tiled(om, n))
    return _worlds[kind]


@pytest.mark.parametrize("kind", list(KINDS))
def test_b4_post_pass_past_one_grid_trip_host_form(kind):
    K, a, rays, want_h, want_m = world(kind)
    assert sz.crossing_trips(rays.shape[0], sz.POST_PASS_CAP) == 2
    h, m = a.TraverseBatch(rays)
    assert h.dtype == K.hit
    K.same(h, m, want_h, want_m)


@pytest.mark.parametrize("kind", list(KINDS))
def test_b4_post_pass_past_one_grid_trip_device_form(kind):
    import torch

    K, a, rays, want_h, want_m = world(kind)
    n = rays.shape[0]
    assert sz.crossing_trips(n, sz.POST_PASS_CAP) == 2
    d_r, d_h, d_m = to_device(rays), filled(n * K.hit.itemsize), filled(n)
    torch.cuda.synchronize()
    assert a.TraverseBatchDevice(d_r, d_h, d_m) == n
    torch.cuda.synchronize()
    K.same(d_h.cpu().numpy().view(K.hit), d_m.cpu().numpy(), want_h, want_m)


@pytest.mark.parametrize("kind", list(KINDS))
def test_b4_occlusion_query_at_the_same_size(kind):
    """No post pass behind an occlusion launch: the walk closes the completion record itself.  Its flags are the closest-hit flags."""
    import torch

    K, a, rays, want_h, want_m = world(kind)
    n = rays.shape[0]
    assert n > sz.POST_PASS_CAP
    assert np.array_equal(a.OccludedBatch(rays), want_m)
    d_r, d_m = to_device(rays), filled(n)
    torch.cuda.synchronize()
    assert a.OccludedBatchDevice(d_r, d_m) == n
    torch.cuda.synchronize()
    assert np.array_equal(d_m.cpu().numpy(), want_m)
    h, m = a.TraverseBatch(rays[:1000])  # (a closest-hit launch behind it finds the completion record closed)
    K.same(h, m, want_h[:1000], want_m[:1000])


# ---- B5: k_max_index past the cap ------------------------------------------------------------------------------------------------
NF_BIG = 720000  # plane(600, 600): 2 160 000 index words


@pytest.fixture(scope="module")
def plane_720k():
    v, f = scenes.plane(600, 600)
    assert f.shape[0] == NF_BIG and 3 * NF_BIG > sz.MAX_INDEX_CAP_WORDS
    top = v.shape[0] - 1
    assert int(f.max()) == top
    g = f.copy()
    g[g == top] = top - 1  # no face names the last vertex: the cases plant the one largest index themselves
    return v, g


def with_largest_index_at(f, top, word):
    g = f.copy()
    g.reshape(-1)[word] = top
    assert int((g == top).sum()) == 1
    return g


def dev_faces(f):
    import torch

    return torch.from_numpy(np.ascontiguousarray(f).view(np.int32).copy()).cuda()


def check_max_index_case(oracle, v, g, d_f, rays):
    """BuildDevice with exactly max + 1 vertex rows equals the host Build and takes a RefitDevice of the same tensor; one row short
    is refused with the index named and the context left as it was."""
    import torch

    top = v.shape[0] - 1
    a = BVHAccel(np.float32)
    assert a.Build(g.shape[0], TriangleMesh(v, g))
    na, ia = a.GetTree()
    a.close()
    b = BVHAccel(np.float32)
    d_v = torch.from_numpy(v).cuda()
    assert d_v.shape[0] == top + 1
    assert b.BuildDevice(d_v, d_f)
    assert b._refit_rows() == top + 1
    n0, i0 = b.GetTree()
    assert n0.shape[0] > 0 and n0.tobytes() == na.tobytes() and i0.tobytes() == ia.tobytes(), "the tree differs from the host Build's"
    oh, om = oracle.traverse(n0, i0, v, g, rays)
    assert hits_and_misses(om)
    h0, m0 = b.TraverseBatch(rays)
    assert_hits_identical(oh, om, h0, m0)
    b.RefitDevice(d_v)
    n1, i1 = b.GetTree()
    assert n1.tobytes() == n0.tobytes() and i1.tobytes() == i0.tobytes()
    # one row short: refused before a vertex is read, whatever trip of the reduction meets the index
    d_short = d_v[:top].contiguous()
    with pytest.raises(NrtError) as e:
        b.SetMeshDevice(d_short, d_f)
    assert e.value.status == NRT_ERR_INVALID and ("index %d " % top) in str(e.value), str(e.value)
    assert b._refit_rows() == top + 1
    n2, i2 = b.GetTree()
    assert n2.tobytes() == n0.tobytes() and i2.tobytes() == i0.tobytes()
    h2, m2 = b.TraverseBatch(rays)
    assert_hits_identical(oh, om, h2, m2)
    b.close()


@pytest.mark.parametrize("face", [10, 710000, NF_BIG - 1], ids=["face10", "face710000", "last_face"])
def test_b5_largest_index_found_in_either_trip_of_the_reduction(oracle, plane_720k, face):
    v, f = plane_720k
    word = 3 * face + (2 if face == NF_BIG - 1 else 1)
    vecs, cap_vecs = 3 * NF_BIG // 4, sz.MAX_INDEX_CAP_WORDS // 4  # 128-bit loads of the array, and of one trip of k_max_index
    assert sz.crossing_trips(vecs, cap_vecs) == 2
    if face == 10:
        assert word // 4 + cap_vecs < vecs  # read in the first trip, by a lane that then takes a second one
    else:
        assert word // 4 >= cap_vecs  # read in the second trip
    g = with_largest_index_at(f, v.shape[0] - 1, word)
    d_f = dev_faces(g)
    assert d_f.data_ptr() % 16 == 0
    check_max_index_case(oracle, v, g, d_f, camera_base(np.float32))


def test_b5_faces_view_one_word_past_a_16_byte_boundary(oracle, plane_720k):
    """head = 3: the scalar head takes three words, and the 128-bit loads past the cap start three words later."""
    import torch

    v, f = plane_720k
    word = 3 * 710000 + 1
    assert word - 3 >= sz.MAX_INDEX_CAP_WORDS
    g = with_largest_index_at(f, v.shape[0] - 1, word)
    big = torch.full((3 * NF_BIG + 8,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")  # (what surrounds the view is larger than any index)
    assert big.data_ptr() % 16 == 0
    big[1:1 + 3 * NF_BIG] = dev_faces(g).reshape(-1)
    d_f = big[1:1 + 3 * NF_BIG].view(NF_BIG, 3)
    assert d_f.data_ptr() % 16 == 4 and d_f.is_contiguous()
    check_max_index_case(oracle, v, g, d_f, camera_base(np.float32))


# ---- B6: the pipelined host path ---------------------------------------------------------------------------------------------------
class C1World:
    """C1 under one precision: the GPU-built tree, the base rays, the oracle's records for them, and its records with per-ray skip ids."""

    def __init__(self, real, oracle, c1_mesh):
        self.real = real
        v, f = c1_mesh
        self.v, self.f = np.ascontiguousarray(v.astype(real)), f
        self.a = BVHAccel(real)
        assert self.a.Build(f.shape[0], TriangleMesh(self.v, f))
        self.nodes, self.idx = self.a.GetTree()
        self.base = camera_base(real)
        self.oh, self.om = oracle.traverse(self.nodes, self.idx, self.v, f, self.base)
        assert hits_and_misses(self.om)
        # odd base rays skip the primitive they hit first (by the oracle), even ones carry the sentinel
        odd = np.arange(sz.B) % 2 == 1
        self.ids = np.where(odd & (self.om == 1), self.oh["prim_id"], SENTINEL).astype(np.uint32)
        assert int((self.ids != SENTINEL).sum()) > sz.B // 8
        self.sh, self.sm = sz.per_ray_skip(oracle, self.nodes, self.idx, self.v, f, self.base, self.ids)
        sel = self.ids != SENTINEL
        assert (self.sh["prim_id"][sel] != self.ids[sel]).all() and int(self.sm[sel].sum()) > 0
        self.RAY, self.HIT = ray_dtype(real), hit_dtype(real)

    def pageable_check(self):
        """A 100-ray pageable call on the same context (the staging buffers are shared with the pipeline)."""
        h, m = self.a.TraverseBatch(self.base[1000:1100])
        assert_hits_identical(self.oh[1000:1100], self.om[1000:1100], h, m)


@pytest.fixture(scope="module")
def w32(oracle, c1_mesh):
    return C1World(np.float32, oracle, c1_mesh)


@pytest.fixture(scope="module")
def w64(oracle, c1_mesh):
    return C1World(np.float64, oracle, c1_mesh)


def pinned_rays(w, n):
    import torch

    t = torch.empty(n * w.RAY.itemsize, dtype=torch.uint8, pin_memory=True)
    assert t.is_pinned()
    t.numpy().view(w.RAY)[:] = sz.tiled(w.base, n)
    return t


def host_call(w, n, with_mask=True, skip=False, expect=NRT_OK, suffix=None):
    """nrtTraverseBatch*(page-locked rays, hits, mask[, ids]) over the base rays tiled to n; returns (hits, mask or None) as numpy views."""
    import torch

    p_r = pinned_rays(w, n)
    p_h = filled(n * w.HIT.itemsize, pinned=True)
    p_m = filled(n, pinned=True) if with_mask else None
    s = suffix or _sfx(w.real)
    if skip:
        p_i = torch.empty(n, dtype=torch.int32, pin_memory=True)
        assert p_i.is_pinned()
        p_i.numpy().view(np.uint32)[:] = sz.tiled(w.ids, n)
        st = getattr(w.a._L, "nrtTraverseBatchSkip_" + s)(w.a._h, p_r.data_ptr(), n, None, p_i.data_ptr(), p_h.data_ptr(), p_m.data_ptr() if with_mask else None)
    else:
        st = getattr(w.a._L, "nrtTraverseBatch_" + s)(w.a._h, p_r.data_ptr(), n, None, p_h.data_ptr(), p_m.data_ptr() if with_mask else None)
    assert st == expect, (st, w.a._L.nrtLastError(w.a._h).decode())
    return p_h.numpy(), (p_m.numpy() if with_mask else None)


def check_pipelined(w, n, pieces, **kw):
    assert n >= 2 * sz.PIECE and sz.crossing_trips(n, sz.PIECE) == pieces, "n = %d does not take the pipelined path in %d pieces" % (n, pieces)
    assert w.a.GetTunable("host_pipeline") == 1
    h, m = host_call(w, n, **kw)
    want_h, want_m = (w.sh, w.sm) if kw.get("skip") else (w.oh, w.om)
    want_h, want_m = sz.tiled(want_h, n), sz.tiled(want_m, n)
    got = h.view(w.HIT)
    assert_hits_identical(want_h, want_m, got, want_m if m is None else m)
    w.pageable_check()


def test_b6_two_pieces(w32):
    check_pipelined(w32, 2 * sz.PIECE, 2)  # one piece per staging slot, no slot reused


def test_b6_a_third_piece_of_one_ray(w32):
    check_pipelined(w32, 2 * sz.PIECE + 1, 3)  # slot 0 reused for a single ray


def test_b6_both_slots_reused_twice_and_a_ragged_end(w32):
    check_pipelined(w32, 5 * sz.PIECE + 77, 6)


def test_b6_without_a_mask(w32):
    check_pipelined(w32, 2 * sz.PIECE + 1, 3, with_mask=False)


def test_b6_fp64(w64):
    check_pipelined(w64, 2 * sz.PIECE + 1, 3)


def test_b6_per_ray_skip_ids(w32):
    check_pipelined(w32, 5 * sz.PIECE + 77, 6, skip=True)


def test_b6_the_staged_path_just_below_the_switch(w32):
    n = 2 * sz.PIECE - 1
    assert n < 2 * sz.PIECE
    h, m = host_call(w32, n)
    assert_hits_identical(sz.tiled(w32.oh, n), sz.tiled(w32.om, n), h.view(w32.HIT), m)
    w32.pageable_check()


def test_b6_pipeline_switched_off(w32):
    n = 2 * sz.PIECE + 1
    w32.a.SetTunable("host_pipeline", 0)
    try:
        h, m = host_call(w32, n)
    finally:
        w32.a.SetTunable("host_pipeline", 1)
    assert_hits_identical(sz.tiled(w32.oh, n), sz.tiled(w32.om, n), h.view(w32.HIT), m)
    w32.pageable_check()


@pytest.mark.parametrize("ctx,call", [("f32", "f64"), ("f64", "f32")])
def test_b6_a_context_of_the_other_precision_is_refused_and_nothing_is_written(w32, w64, ctx, call):
    w, other = (w32, w64) if ctx == "f32" else (w64, w32)
    n = 2 * sz.PIECE + 1
    assert n >= 2 * sz.PIECE

    class Mixed:  # the context of `w`, the buffers and the entry point of the other precision
        a, real, RAY, HIT, base = w.a, other.real, other.RAY, other.HIT, other.base

    h, m = host_call(Mixed, n, expect=NRT_ERR_PRECISION, suffix=call)
    assert (h == FILL).all() and (m == FILL).all(), "a refused call wrote into the caller's buffers"
    w.pageable_check()
    check_pipelined(w, 2 * sz.PIECE + 1, 3)  # the next call works

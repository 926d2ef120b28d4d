"""Device-resident geometry (nrtSetMeshDevice_* / nrtSetSpheresDevice_f32, nanort_amd/csrc/prims.hip): a context fed from torch
tensors ends in the state the host call leaves, so the tree built over it and every trace of it are byte-identical to the host
path's — no tolerance anywhere (builder determinism across contexts is the library's contract).  Also: the index reduction at
wave / block / 128-bit boundaries, strides, views, a side stream, the lifecycle, the num_vertices guard and the refusals."""
import numpy as np
import pytest

from helpers import assert_hits_identical
from nanort_amd import BVHAccel, Scene, SphereGeometry, TriangleMesh, scenes
from nanort_amd.capi import NRT_ERR_INVALID, NRT_ERR_PRECISION, NRT_OK, NrtError
from nanort_amd.wire import widen_rays

pytestmark = pytest.mark.gpu

REALS = [np.float32, np.float64]
CLOUD = 97  # vertices of the random cloud the small meshes index


def _sfx(real):
    return "f32" if np.dtype(real) == np.float32 else "f64"


def _tdt(real):
    import torch

    return torch.float32 if np.dtype(real) == np.float32 else torch.float64


@pytest.fixture(scope="module")
def cam():
    return scenes.camera_rays(96, 64)


def rays_for(real, cam):
    return cam if np.dtype(real) == np.float32 else widen_rays(cam)


def cloud(real, nv=CLOUD, seed=5):
    """Vertices inside the camera's view (scenes.camera_rays looks down -z from (0, 5, 20))."""
    rng = np.random.default_rng(seed)
    return rng.uniform((-8.0, -3.0, -4.0), (8.0, 13.0, 4.0), size=(nv, 3)).astype(real)


def faces_with_max_at(nf, where, nv=CLOUD, seed=9):
    """nf faces over vertices [0, nv - 1) with the one index nv - 1 planted at position `where` of the flat index array."""
    rng = np.random.default_rng(seed + nf)
    f = rng.integers(0, nv - 1, size=3 * nf, dtype=np.uint32)
    f[{"first": 0, "last": 3 * nf - 1, "middle": (3 * nf) // 2}[where]] = nv - 1
    return f.reshape(nf, 3)


def dev_faces(f, unsigned=False):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(f).view(np.int32).copy()).cuda()
    return t.view(torch.uint32) if unsigned and hasattr(torch, "uint32") else t


def dev_rows(v, k=3, fill=np.nan):
    """[nv, k] tensor whose first three columns are v and whose other columns the library must never read."""
    import torch

    rows = np.full((v.shape[0], k), fill, v.dtype)
    rows[:, :3] = v
    return torch.from_numpy(rows).cuda()


def host_built(real, v, f, options=None):
    a = BVHAccel(real)
    assert a.Build(f.shape[0], TriangleMesh(np.ascontiguousarray(v), f), options)
    return a


def assert_same_tree_and_traces(a, b, rays):
    na, ia = a.GetTree()
    nb, ib = b.GetTree()
    assert na.shape[0] > 0 and na.tobytes() == nb.tobytes(), "node arrays differ"
    assert ia.tobytes() == ib.tobytes(), "index arrays differ"
    ha, ma = a.TraverseBatch(rays)
    hb, mb = b.TraverseBatch(rays)
    assert_hits_identical(ha, ma, hb, mb)
    return ma


def max_index_seen(a, d_v, d_f):
    """The largest face index as the library's reduction sees it: the guard refuses num_vertices == it and names it, and
    refuses nothing at num_vertices == it + 1 (what the callers below then pass)."""
    top = int(d_f.cpu().numpy().view(np.uint32).max())
    L, s = a._L, _sfx(a.real)
    st = getattr(L, "nrtSetMeshDevice_" + s)(a._h, d_v.data_ptr(), top, d_v.stride(0) * d_v.element_size(), d_f.data_ptr(), d_f.shape[0], None)
    assert st == NRT_ERR_INVALID and ("index %d " % top) in L.nrtLastError(a._h).decode()
    return top


# ---- the index reduction ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("nf", [1, 2, 21, 22, 341, 342, 2731])
def test_largest_index_found_wherever_it_sits(cam, nf, where):
    """3 * nf = 3, 6, 63, 66, 1023, 1026, 8193 indices: either side of a wave (64), a block of 128-bit loads (256 x 4) and two
    blocks, lengths that are and are not multiples of four; the one largest index first, last, and in the middle."""
    v, f = cloud(np.float32), faces_with_max_at(nf, where)
    a = host_built(np.float32, v, f)
    b = BVHAccel(np.float32)
    d_v, d_f = dev_rows(v), dev_faces(f)
    assert max_index_seen(b, d_v, d_f) == CLOUD - 1
    assert b.BuildDevice(d_v, d_f)
    assert_same_tree_and_traces(a, b, cam)
    a.close()
    b.close()


def test_faces_view_one_word_past_a_16_byte_boundary(cam):
    """d_faces starts 4 bytes into an allocation: the reduction's scalar head takes three words before its first 128-bit load."""
    import torch

    v, f = cloud(np.float32), faces_with_max_at(342, "first")
    big = torch.full((3 * 342 + 8,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")  # (what surrounds the view is larger than any index)
    assert big.data_ptr() % 16 == 0
    big[1:1 + 3 * 342] = dev_faces(f).reshape(-1)
    d_f = big[1:1 + 3 * 342].view(342, 3)
    assert d_f.data_ptr() % 16 == 4 and d_f.is_contiguous()
    a = host_built(np.float32, v, f)
    b = BVHAccel(np.float32)
    d_v = dev_rows(v)
    assert max_index_seen(b, d_v, d_f) == CLOUD - 1
    assert b.BuildDevice(d_v, d_f)
    assert_same_tree_and_traces(a, b, cam)
    a.close()
    b.close()


def test_vertex_tensor_longer_than_the_faces_use(cam):
    """nv' > max + 1: the context's vertex count is max + 1 — a RefitDevice of exactly max + 1 rows is a whole refit."""
    v = cloud(np.float32, nv=CLOUD + 40)
    f = faces_with_max_at(341, "middle")  # uses vertices 0 .. CLOUD - 1
    a = host_built(np.float32, v, f)
    b = BVHAccel(np.float32)
    assert b.BuildDevice(dev_rows(v), dev_faces(f))
    assert b._refit_rows() == CLOUD
    assert_same_tree_and_traces(a, b, cam)
    v1 = (v[:CLOUD] * np.float32(0.75) + np.float32(0.5)).astype(np.float32)
    a.Refit(v1)
    b.RefitDevice(dev_rows(v1))
    assert_same_tree_and_traces(a, b, cam)
    a.close()
    b.close()


# ---- strides, views, streams -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real,k", [(np.float32, 3), (np.float32, 4), (np.float32, 7), (np.float64, 3), (np.float64, 4), (np.float64, 5)],
                         ids=["f32-12", "f32-16", "f32-28", "f64-24", "f64-32", "f64-40"])
def test_row_strides(cam, real, k):
    v, f = cloud(real), faces_with_max_at(342, "last")
    a = host_built(real, v, f)
    b = BVHAccel(real)
    d_v = dev_rows(v, k)
    assert d_v.stride(0) * d_v.element_size() == k * np.dtype(real).itemsize
    assert b.BuildDevice(d_v, dev_faces(f, unsigned=(k == 4)))
    assert_same_tree_and_traces(a, b, rays_for(real, cam))
    a.close()
    b.close()


@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_row_offset_view(cam, real):
    """t[1:] of a [nv + 1, 4] tensor: the base is one row into the allocation."""
    import torch

    v, f = cloud(real), faces_with_max_at(341, "first")
    t = torch.cat([torch.full((1, 4), float("nan"), dtype=_tdt(real), device="cuda"), dev_rows(v, 4)])
    a = host_built(real, v, f)
    b = BVHAccel(real)
    assert b.BuildDevice(t[1:], dev_faces(f))
    assert_same_tree_and_traces(a, b, rays_for(real, cam))
    a.close()
    b.close()


def test_tensors_filled_on_a_side_stream(cam):
    """The tensors are produced by torch ops on a non-default stream and handed over with that stream, nothing in between."""
    import torch

    v, f = cloud(np.float32, nv=4099), faces_with_max_at(2731, "last", nv=4099)
    h_v = torch.from_numpy(np.concatenate([v, np.zeros((v.shape[0], 1), np.float32)], axis=1)).pin_memory()
    h_f = torch.from_numpy(f.view(np.int32).copy()).pin_memory()
    a = host_built(np.float32, v, f)
    b = BVHAccel(np.float32)
    side = torch.cuda.Stream()
    d_v = torch.zeros((v.shape[0], 4), dtype=torch.float32, device="cuda")
    d_f = torch.zeros((f.shape[0], 3), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):  # (work ahead of the fill on the same stream)
            d_v.mul_(1.0)
        d_v.copy_(h_v, non_blocking=True)
        d_f.copy_(h_f, non_blocking=True)
        d_v.add_(0.0)
        assert b.BuildDevice(d_v, d_f, stream=side)
    assert_same_tree_and_traces(a, b, cam)
    a.close()
    b.close()


@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_real_mesh(cam, c1_mesh, real):
    v, f = c1_mesh
    v = np.ascontiguousarray(v.astype(real))
    a = host_built(real, v, f)
    b = BVHAccel(real)
    assert b.BuildDevice(dev_rows(v, 4), dev_faces(f))
    assert assert_same_tree_and_traces(a, b, rays_for(real, cam)).any()
    a.close()
    b.close()


# ---- lifecycle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_build_device_then_refits(cam, c1_mesh, real):
    v, f = c1_mesh
    v = np.ascontiguousarray(v.astype(real))
    rays = rays_for(real, cam)
    a = host_built(real, v, f)
    b = BVHAccel(real)
    assert b.BuildDevice(dev_rows(v), dev_faces(f))
    w = v.astype(np.float64).copy()
    w[:, 1] += 0.2 * np.sin(3.0 * w[:, 0])
    v1 = w.astype(real)
    a.Refit(v1)
    b.RefitDevice(dev_rows(v1, 4))
    assert_same_tree_and_traces(a, b, rays)
    v2 = (v * real(1.25)).astype(real)
    a.Refit(v2)
    b.Refit(v2)  # host vertices over a device-set mesh
    assert_same_tree_and_traces(a, b, rays)
    with pytest.raises(ValueError):
        b.RefitDevice(dev_rows(v2[:-1]))
    a.close()
    b.close()


def test_set_mesh_device_over_a_context_that_has_just_traced(cam, c1_mesh):
    v, f = c1_mesh
    v = np.ascontiguousarray(v.astype(np.float32))
    v2, f2 = cloud(np.float32), faces_with_max_at(341, "middle")
    b = host_built(np.float32, v, f)
    assert b.TraverseBatch(cam)[1].any()
    b.SetMeshDevice(dev_rows(v2), dev_faces(f2))
    assert not b.IsValid()  # the tree is dropped, as by SetMesh
    assert b.BuildCurrent()
    a = host_built(np.float32, v2, f2)
    assert_same_tree_and_traces(a, b, cam)
    a.close()
    b.close()


def test_committed_scene_refuses_until_committed_again(cam, c1_mesh):
    v, f = c1_mesh
    v = np.ascontiguousarray(v.astype(np.float32))
    a = host_built(np.float32, v, f)
    b = host_built(np.float32, v, f)
    x = np.eye(4, dtype=np.float32)
    sa, sb = Scene(), Scene()
    sa.AddNode(a, x)
    sb.AddNode(b, x)
    assert sa.Commit() and sb.Commit()
    v1 = (v + np.float32(0.125)).astype(np.float32)
    assert a.Build(f.shape[0], TriangleMesh(v1, f))
    assert b.BuildDevice(dev_rows(v1), dev_faces(f))
    with pytest.raises(NrtError):
        sb.TraverseBatch(cam)
    assert sa.Commit() and sb.Commit()
    ha, ma = sa.TraverseBatch(cam)
    hb, mb = sb.TraverseBatch(cam)
    assert ma.any() and np.array_equal(ma, mb) and ha.tobytes() == hb.tobytes()
    sa.close()
    sb.close()


@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_empty_mesh(real):
    import torch

    b = BVHAccel(real)
    assert b.BuildDevice(torch.zeros((0, 3), dtype=_tdt(real), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda")) is False
    assert not b.IsValid()
    v, f = cloud(real), faces_with_max_at(21, "first")
    assert b.BuildDevice(dev_rows(v), dev_faces(f))
    assert b.BuildDevice(dev_rows(v), dev_faces(f[:0])) is False  # ... also over a context that holds a tree
    assert not b.IsValid()
    b.close()


# ---- refusals: none of them reads a vertex ------------------------------------------------------------------------------------
def test_face_index_out_of_range_leaves_the_context_as_it_was(cam, c1_mesh):
    v, f = c1_mesh
    v = np.ascontiguousarray(v.astype(np.float32))
    b = host_built(np.float32, v, f)
    n0, i0 = b.GetTree()
    h0, m0 = b.TraverseBatch(cam)
    bad = f.copy()
    bad[f.shape[0] // 3, 1] = v.shape[0]  # == num_vertices: one past the last row
    with pytest.raises(NrtError) as e:
        b.SetMeshDevice(dev_rows(v), dev_faces(bad))
    assert e.value.status == NRT_ERR_INVALID and ("index %d " % v.shape[0]) in str(e.value)
    assert isinstance(b._mesh, TriangleMesh)
    n1, i1 = b.GetTree()
    assert n1.tobytes() == n0.tobytes() and i1.tobytes() == i0.tobytes()
    h1, m1 = b.TraverseBatch(cam)
    assert_hits_identical(h0, m0, h1, m1)
    b.close()


@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_argument_refusals_leave_the_context_as_it_was(cam, real):
    import torch

    other = np.float64 if real == np.float32 else np.float32
    it = np.dtype(real).itemsize
    v, f = cloud(real), faces_with_max_at(341, "last")
    rays = rays_for(real, cam)
    b = host_built(real, v, f)
    n0, i0 = b.GetTree()
    h0, m0 = b.TraverseBatch(rays)
    L, s, o = b._L, _sfx(real), _sfx(other)
    d_v, d_f = dev_rows(v, 4), dev_faces(f)
    d_o = dev_rows(v.astype(other))
    fn, nf, nv = getattr(L, "nrtSetMeshDevice_" + s), f.shape[0], v.shape[0]
    assert getattr(L, "nrtSetMeshDevice_" + o)(b._h, d_o.data_ptr(), nv, 3 * np.dtype(other).itemsize, d_f.data_ptr(), nf, None) == NRT_ERR_PRECISION
    assert fn(b._h, d_v.data_ptr(), nv, 3 * it - it, d_f.data_ptr(), nf, None) == NRT_ERR_INVALID  # a stride of two elements
    assert "stride" in L.nrtLastError(b._h).decode()
    assert fn(b._h, None, nv, 4 * it, d_f.data_ptr(), nf, None) == NRT_ERR_INVALID
    assert fn(b._h, d_v.data_ptr(), nv, 4 * it, None, nf, None) == NRT_ERR_INVALID
    assert "NULL" in L.nrtLastError(b._h).decode()
    assert fn(b._h, d_v.data_ptr(), 0, 4 * it, d_f.data_ptr(), nf, None) == NRT_ERR_INVALID
    assert fn(b._h, d_v.data_ptr(), nv, 4 * it + 1, d_f.data_ptr(), nf, None) == NRT_ERR_INVALID  # misaligned stride
    assert fn(b._h, d_v.data_ptr() + 1, nv, 4 * it, d_f.data_ptr(), nf, None) == NRT_ERR_INVALID  # misaligned vertex pointer
    assert fn(b._h, d_v.data_ptr(), nv, 4 * it, d_f.data_ptr() + 2, nf, None) == NRT_ERR_INVALID  # misaligned face pointer
    assert "aligned" in L.nrtLastError(b._h).decode()
    with pytest.raises(TypeError):
        b.SetMeshDevice(d_o, d_f)
    with pytest.raises(TypeError) as e:  # 64-bit indices are never converted behind the caller's back
        b.SetMeshDevice(d_v, d_f.to(torch.int64))
    assert "int32" in str(e.value)
    with pytest.raises(ValueError):
        b.SetMeshDevice(d_v.cpu(), d_f)
    with pytest.raises(ValueError):
        b.SetMeshDevice(d_v, d_f.cpu())
    with pytest.raises(ValueError):
        b.SetMeshDevice(d_v[:, :2], d_f)
    with pytest.raises(ValueError):
        b.SetMeshDevice(d_v, d_f.t())
    assert isinstance(b._mesh, TriangleMesh)
    n1, i1 = b.GetTree()
    assert n1.tobytes() == n0.tobytes() and i1.tobytes() == i0.tobytes()
    h1, m1 = b.TraverseBatch(rays)
    assert_hits_identical(h0, m0, h1, m1)
    b.close()


# ---- spheres -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 1000])
def test_spheres_from_device_tensors(n):
    import torch

    c, r = scenes.random_spheres(n)
    rays = scenes.particle_camera_rays(96, 64)
    a = BVHAccel(np.float32)
    assert a.Build(n, SphereGeometry(c, r))
    b = BVHAccel(np.float32)
    b.SetSpheresDevice(torch.from_numpy(c).cuda(), torch.from_numpy(r).cuda())
    assert b.BuildCurrent()
    assert_same_tree_and_traces(a, b, rays)
    a.close()
    b.close()


def test_sphere_refusals_and_replacing_a_mesh(cam):
    import torch

    c, r = scenes.random_spheres(65)
    d_c, d_r = torch.from_numpy(c).cuda(), torch.from_numpy(r).cuda()
    v, f = cloud(np.float32), faces_with_max_at(21, "middle")
    b = host_built(np.float32, v, f)
    h0, m0 = b.TraverseBatch(cam)
    L = b._L
    assert L.nrtSetSpheresDevice_f32(b._h, None, d_r.data_ptr(), 65, None) == NRT_ERR_INVALID
    assert L.nrtSetSpheresDevice_f32(b._h, d_c.data_ptr(), None, 65, None) == NRT_ERR_INVALID
    assert L.nrtSetSpheresDevice_f32(b._h, d_c.data_ptr() + 2, d_r.data_ptr(), 65, None) == NRT_ERR_INVALID
    with pytest.raises(ValueError):
        b.SetSpheresDevice(d_c.cpu(), d_r)
    with pytest.raises(ValueError):
        b.SetSpheresDevice(d_c, d_r[:-1])
    with pytest.raises(TypeError):
        b.SetSpheresDevice(d_c.double(), d_r)
    h1, m1 = b.TraverseBatch(cam)
    assert_hits_identical(h0, m0, h1, m1)
    d = BVHAccel(np.float64)
    d.SetMesh(TriangleMesh(v.astype(np.float64), f))
    assert L.nrtSetSpheresDevice_f32(d._h, d_c.data_ptr(), d_r.data_ptr(), 65, None) == NRT_ERR_PRECISION
    d.close()
    b.SetSpheresDevice(d_c, d_r)  # one primitive kind per context: the spheres replace the mesh
    assert not b.IsValid() and b.BuildCurrent()
    a = BVHAccel(np.float32)
    assert a.Build(65, SphereGeometry(c, r))
    assert_same_tree_and_traces(a, b, scenes.particle_camera_rays(96, 64))
    assert L.nrtSetSpheresDevice_f32(b._h, None, None, 0, None) == NRT_OK
    assert not b.IsValid()
    a.close()
    b.close()

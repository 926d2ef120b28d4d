"""Host-side mirror of the reference's operator interface for the hot path.

`BVHAccel` here plays the role of nanort::BVHAccel<T> (reference
nanort.h:698-860) for the built-in triangle plugin, with the same method names
and argument meaning; every call goes through the C ABI (include/nanort_hip.h)
into the HIP library.  `TraverseBatch` is the one addition: N rays per call
instead of the reference's one (`Traverse`, nanort.h:757-759).

    mesh  = TriangleMesh(vertices, faces, stride_bytes)   # nanort.h:925-930
    accel = BVHAccel(np.float32)
    accel.Build(mesh.num_faces, mesh, options)            # nanort.h:716-718
    hits, mask = accel.TraverseBatch(rays, trace_options) # N x Traverse

numpy arrays carry the reference's PODs (nanort_amd.wire).  torch is used only
by the *Device* variants (HBM-resident tensors, current stream).
"""
import ctypes

import numpy as np

from . import capi
from .wire import (
    BUILD_OPTIONS_F32,
    BUILD_OPTIONS_F64,
    BUILD_STATS,
    TRACE_OPTIONS,
    hit_dtype,
    node_dtype,
    ray_dtype,
    suffix,
)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _opts(options):
    """The caller's trace options as one TRACE_OPTIONS record (None: the library's defaults)."""
    return None if options is None else np.asarray(options, dtype=TRACE_OPTIONS).reshape(1)


class TriangleMesh:
    """nanort::TriangleMesh<T> (reference nanort.h:922-991): caller-owned flat arrays."""

    def __init__(self, vertices, faces, vertex_stride_bytes=None):
        self.vertices = np.ascontiguousarray(vertices)
        if self.vertices.dtype not in (np.float32, np.float64):
            raise TypeError("vertices must be float32 or float64")
        self.faces = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
        self.vertex_stride_bytes = (
            3 * self.vertices.dtype.itemsize if vertex_stride_bytes is None else int(vertex_stride_bytes)
        )
        self.num_faces = int(self.faces.shape[0])

    def GetVertices(self):
        return self.vertices

    def GetFaces(self):
        return self.faces

    def GetVertexStrideBytes(self):
        return self.vertex_stride_bytes


class MotionTriangleMesh(TriangleMesh):
    """A triangle mesh with a second vertex keyframe (include/nanort_hip.h, "motion blur"): `vertices0` at time 0, `vertices1` at
    time 1, the same faces and the same row layout for both."""

    def __init__(self, vertices0, vertices1, faces, vertex_stride_bytes=None):
        TriangleMesh.__init__(self, vertices0, faces, vertex_stride_bytes)
        self.vertices1 = np.ascontiguousarray(vertices1)
        if self.vertices1.dtype != self.vertices.dtype or self.vertices1.shape != self.vertices.shape:
            raise ValueError("the two keyframes must have the same dtype and shape")

    def GetVertices1(self):
        return self.vertices1


class SphereGeometry:
    """The sphere ("particle") custom primitive of the reference (examples/particle_primitive/main.cc:82-291:
    SpherePred + SphereGeometry + SphereIntersector rolled into one description): xyz centres and one radius each."""

    def __init__(self, centers, radii):
        self.centers = np.ascontiguousarray(centers, dtype=np.float32).reshape(-1, 3)
        self.radii = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1)
        if self.centers.shape[0] != self.radii.shape[0]:
            raise ValueError("one radius per centre")
        self.num_spheres = int(self.radii.shape[0])
        self.num_faces = self.num_spheres  # "number of primitives", under the name Build() checks


class CylinderGeometry:
    """The cylinder custom primitive of the reference (examples/cylinder_primitive/main.cc:94-424: CylinderPred +
    CylinderGeometry + CylinderIntersector): two end points (n, 2, 3) and two radii (n, 2) per cylinder, and the
    intersector's test_cap flag."""

    def __init__(self, endpoints, radii, test_cap=True):
        self.endpoints = np.ascontiguousarray(endpoints, dtype=np.float32).reshape(-1, 2, 3)
        self.radii = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1, 2)
        if self.endpoints.shape[0] != self.radii.shape[0]:
            raise ValueError("two radii per cylinder")
        self.test_cap = bool(test_cap)
        self.num_faces = int(self.radii.shape[0])


class CurveGeometry:
    """The cubic Bezier curve primitive of the reference (examples/curves_primitive/main.cc:481-840: CurvePred + CurveGeometry +
    CurveIntersector): four control points (n, 4, 3) and four radii (n, 4) per curve, and the intersector's num_subdivisions."""

    def __init__(self, control_points, radii, num_subdivisions=4):
        self.control_points = np.ascontiguousarray(control_points, dtype=np.float32).reshape(-1, 4, 3)
        self.radii = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1, 4)
        if self.control_points.shape[0] != self.radii.shape[0]:
            raise ValueError("four radii per curve")
        self.num_subdivisions = int(num_subdivisions)
        self.num_faces = int(self.radii.shape[0])


class DeviceGeometry:
    """What the accel remembers of primitives set from device tensors (SetMeshDevice / SetSpheresDevice / SetCurvesDevice): nothing
    of the tensors themselves — the context owns its copy.  `kind` is "triangles", "spheres" or "curves"; `num_verts` is the context's vertex
    count (max(faces) + 1 for triangles), what Refit / RefitDevice check their rows against."""

    def __init__(self, kind, num_faces, num_verts):
        self.kind = kind
        self.num_faces = int(num_faces)
        self.num_verts = int(num_verts)


class BVHAccel:
    """nanort::BVHAccel<T> on one MI355X (built-in triangle geometry, or the sphere / cylinder / curve primitives in fp32)."""

    def __init__(self, real=np.float32, device=0):
        self.real = np.dtype(real)
        if self.real not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError("real must be float32 or float64")
        self._s = suffix(self.real)
        self._L = capi.lib()
        h = ctypes.c_void_p()
        st = self._L.nrtCreate(int(device), ctypes.byref(h))
        if st != capi.NRT_OK:
            raise capi.NrtError(st, self._L.nrtLastError(None).decode())
        self._h = h
        self.device = int(device)
        self._stats = np.zeros((), dtype=BUILD_STATS)
        self._mesh = None

    def close(self):
        if getattr(self, "_h", None):
            self._L.nrtDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != capi.NRT_OK:
            raise capi.NrtError(st, self._L.nrtLastError(self._h).decode())

    # -- mesh / build -------------------------------------------------------
    def SetMesh(self, mesh):
        if isinstance(mesh, CurveGeometry):
            if self.real != np.float32:
                raise TypeError("curve primitives are fp32 (as the reference example)")
            self._check(self._L.nrtSetCurves_f32(self._h, _p(mesh.control_points), _p(mesh.radii), mesh.num_faces, mesh.num_subdivisions))
            self._mesh = mesh
            return
        if isinstance(mesh, CylinderGeometry):
            if self.real != np.float32:
                raise TypeError("cylinder primitives are fp32 (as the reference example)")
            self._check(self._L.nrtSetCylinders_f32(self._h, _p(mesh.endpoints), _p(mesh.radii), mesh.num_faces, int(mesh.test_cap)))
            self._mesh = mesh
            return
        if isinstance(mesh, SphereGeometry):
            if self.real != np.float32:
                raise TypeError("sphere primitives are fp32 (as the reference example)")
            self._check(self._L.nrtSetSpheres_f32(self._h, _p(mesh.centers), _p(mesh.radii), mesh.num_spheres))
            self._mesh = mesh
            return
        if mesh.vertices.dtype != self.real:
            raise TypeError("mesh precision %s != accel precision %s" % (mesh.vertices.dtype, self.real))
        self._check(
            getattr(self._L, "nrtSetMesh_" + self._s)(
                self._h, _p(mesh.vertices), mesh.vertex_stride_bytes, _p(mesh.faces), mesh.num_faces
            )
        )
        self._mesh = mesh
        if isinstance(mesh, MotionTriangleMesh) and mesh.num_faces:
            self._check(getattr(self._L, "nrtSetMeshMotion_" + self._s)(self._h, _p(mesh.vertices1), mesh.vertex_stride_bytes))

    def SetMeshMotion(self, vertices1, vertex_stride_bytes=None):
        """nrtSetMeshMotion: the second vertex keyframe of the triangle mesh last set (None removes it); drops the tree.  `vertices1`:
        a numpy array of the accel's precision with at least the mesh's vertex count of rows, xyz first in each row (the row stride
        defaults to the array's own)."""
        if vertices1 is None:
            self._check(getattr(self._L, "nrtSetMeshMotion_" + self._s)(self._h, None, 0))
            return
        v = np.asarray(vertices1)
        if v.dtype != self.real:
            raise TypeError("vertex precision %s != accel precision %s" % (v.dtype, self.real))
        nv = self._refit_rows()
        if vertex_stride_bytes is None:
            v = np.ascontiguousarray(v.reshape(v.shape[0], -1) if v.ndim > 1 else v.reshape(-1, 3))
            if v.shape[1] < 3:
                raise ValueError("vertices must be [nv, k >= 3]")
            if nv is not None and v.shape[0] < nv:
                raise ValueError("vertices hold %d rows; the mesh has %d vertices" % (v.shape[0], nv))
            vertex_stride_bytes = v.strides[0]
        else:
            if not v.flags["C_CONTIGUOUS"]:
                raise ValueError("an explicit vertex_stride_bytes needs a C-contiguous array")
            need = (nv - 1) * int(vertex_stride_bytes) + 3 * v.itemsize if nv else 0
            if nv is not None and v.nbytes < need:
                raise ValueError("vertices hold %d bytes; %d vertices at stride %d need %d" % (v.nbytes, nv, int(vertex_stride_bytes), need))
        self._check(getattr(self._L, "nrtSetMeshMotion_" + self._s)(self._h, _p(v), int(vertex_stride_bytes)))

    def SetMeshMotionDevice(self, d_vertices1, stream=None):
        """nrtSetMeshMotionDevice: the second keyframe from a torch tensor on the accel's device, [nv', k >= 3] of the accel's
        precision with stride(1) == 1 (the row stride is stride(0)); the library refuses nv' below the mesh's vertex count before it
        enqueues anything.  Read on `stream` (default: torch's current stream); returns when the accel owns its copy.  None removes
        the keyframe."""
        import torch

        if d_vertices1 is None:
            self._check(getattr(self._L, "nrtSetMeshMotionDevice_" + self._s)(self._h, None, 0, 0, self._stream_handle(stream)))
            return
        want = torch.float32 if self.real == np.float32 else torch.float64
        if d_vertices1.dtype != want:
            raise TypeError("vertex dtype %s != accel precision %s" % (d_vertices1.dtype, self.real))
        if d_vertices1.dim() != 2 or d_vertices1.shape[1] < 3 or d_vertices1.stride(1) != 1:
            raise ValueError("vertices must be [nv, k >= 3] with stride(1) == 1")
        self._on_device(d_vertices1, "vertices")
        stride = d_vertices1.stride(0) * d_vertices1.element_size()
        self._check(getattr(self._L, "nrtSetMeshMotionDevice_" + self._s)(
            self._h, d_vertices1.data_ptr(), int(d_vertices1.shape[0]), stride, self._stream_handle(stream)))

    def Build(self, num_primitives, mesh, options=None):
        """BVHAccel::Build (reference nanort.h:1892-2149). Returns False iff n == 0."""
        if num_primitives != mesh.num_faces:
            if isinstance(mesh, CurveGeometry):
                mesh = CurveGeometry(mesh.control_points[:num_primitives], mesh.radii[:num_primitives], mesh.num_subdivisions)
            elif isinstance(mesh, CylinderGeometry):
                mesh = CylinderGeometry(mesh.endpoints[:num_primitives], mesh.radii[:num_primitives], mesh.test_cap)
            elif isinstance(mesh, SphereGeometry):
                mesh = SphereGeometry(mesh.centers[:num_primitives], mesh.radii[:num_primitives])
            elif isinstance(mesh, MotionTriangleMesh):
                mesh = MotionTriangleMesh(mesh.vertices, mesh.vertices1, mesh.faces[:num_primitives], mesh.vertex_stride_bytes)
            else:
                mesh = TriangleMesh(mesh.vertices, mesh.faces[:num_primitives], mesh.vertex_stride_bytes)
        self.SetMesh(mesh)
        return self.BuildCurrent(options)

    def _stream_handle(self, stream):
        import torch

        if stream is None:
            return torch.cuda.current_stream(self.device).cuda_stream
        return stream.cuda_stream if hasattr(stream, "cuda_stream") else stream

    def _n_rays(self, d_rays):
        """Rays of the accel's precision a device tensor of raw bytes (or of any element size) holds."""
        return d_rays.numel() * d_rays.element_size() // ray_dtype(self.real).itemsize

    def _on_device(self, t, what):
        if t.device.type != "cuda" or t.device.index != self.device:
            raise ValueError("%s must live on cuda:%d" % (what, self.device))

    def SetMeshDevice(self, d_vertices, d_faces, stream=None):
        """SetMesh from torch tensors on the accel's device (nrtSetMeshDevice): nothing goes through the host.  `d_vertices`:
        [nv, k >= 3] of the accel's precision with stride(1) == 1 (the row stride is stride(0)); `d_faces`: [nf, 3], contiguous,
        torch.int32 or torch.uint32 (read as u32).  The library refuses a face index >= nv before it reads a vertex.  Enqueued on
        `stream` (default: torch's current stream), behind whatever produced the tensors there; returns when the accel owns
        its copy."""
        import torch

        want = torch.float32 if self.real == np.float32 else torch.float64
        if d_vertices.dtype != want:
            raise TypeError("vertex dtype %s != accel precision %s" % (d_vertices.dtype, self.real))
        index_types = [torch.int32] + ([torch.uint32] if hasattr(torch, "uint32") else [])
        if d_faces.dtype not in index_types:
            raise TypeError("faces must be torch.int32 or torch.uint32 (got %s): convert explicitly, 64-bit indices are not read" % d_faces.dtype)
        if d_vertices.dim() != 2 or d_vertices.shape[1] < 3 or d_vertices.stride(1) != 1:
            raise ValueError("vertices must be [nv, k >= 3] with stride(1) == 1")
        if d_faces.dim() != 2 or d_faces.shape[1] != 3 or not d_faces.is_contiguous():
            raise ValueError("faces must be [nf, 3], contiguous")
        self._on_device(d_vertices, "vertices")
        self._on_device(d_faces, "faces")
        nv, nf = int(d_vertices.shape[0]), int(d_faces.shape[0])
        stride = d_vertices.stride(0) * d_vertices.element_size()
        self._check(getattr(self._L, "nrtSetMeshDevice_" + self._s)(
            self._h, d_vertices.data_ptr() if nv else None, nv, stride, d_faces.data_ptr() if nf else None, nf, self._stream_handle(stream)))
        # The library accepted the indices: all are < nv.  Below 2^31 the int32 view orders them as u32 does; a larger block
        # (never seen) is remembered by its row count, which is at least the context's vertex count.
        if nf == 0:
            rows = 0
        elif nv > 2 ** 31:
            rows = nv
        else:
            rows = int(d_faces.view(torch.int32).max().item()) + 1
        self._mesh = DeviceGeometry("triangles", nf, rows)

    def SetSpheresDevice(self, d_centers, d_radii, stream=None):
        """SetMesh(SphereGeometry) from torch float32 tensors on the accel's device (nrtSetSpheresDevice): `d_centers` [n, 3] and
        `d_radii` [n], both contiguous.  Ordering as SetMeshDevice."""
        import torch

        if self.real != np.float32:
            raise TypeError("sphere primitives are fp32 (as the reference example)")
        if d_centers.dtype != torch.float32 or d_radii.dtype != torch.float32:
            raise TypeError("centers and radii must be torch.float32")
        if d_centers.dim() != 2 or d_centers.shape[1] != 3 or not d_centers.is_contiguous():
            raise ValueError("centers must be [n, 3], contiguous")
        if d_radii.dim() != 1 or d_radii.shape[0] != d_centers.shape[0] or not d_radii.is_contiguous():
            raise ValueError("one radius per centre, contiguous")
        self._on_device(d_centers, "centers")
        self._on_device(d_radii, "radii")
        n = int(d_radii.shape[0])
        self._check(self._L.nrtSetSpheresDevice_f32(
            self._h, d_centers.data_ptr() if n else None, d_radii.data_ptr() if n else None, n, self._stream_handle(stream)))
        self._mesh = DeviceGeometry("spheres", n, n)

    def SetCurvesDevice(self, d_control_points, d_radii, num_subdivisions=4, stream=None):
        """SetMesh(CurveGeometry) from torch float32 tensors on the accel's device (nrtSetCurvesDevice): `d_control_points`
        [n, 4, 3] and `d_radii` [n, 4], both contiguous.  Ordering as SetMeshDevice."""
        import torch

        if self.real != np.float32:
            raise TypeError("curve primitives are fp32 (as the reference example)")
        if d_control_points.dtype != torch.float32 or d_radii.dtype != torch.float32:
            raise TypeError("control points and radii must be torch.float32")
        if d_control_points.dim() != 3 or tuple(d_control_points.shape[1:]) != (4, 3) or not d_control_points.is_contiguous():
            raise ValueError("control points must be [n, 4, 3], contiguous")
        if d_radii.dim() != 2 or d_radii.shape[1] != 4 or d_radii.shape[0] != d_control_points.shape[0] or not d_radii.is_contiguous():
            raise ValueError("four radii per curve, contiguous")
        self._on_device(d_control_points, "control points")
        self._on_device(d_radii, "radii")
        n = int(d_radii.shape[0])
        self._check(self._L.nrtSetCurvesDevice_f32(
            self._h, d_control_points.data_ptr() if n else None, d_radii.data_ptr() if n else None, n, int(num_subdivisions),
            self._stream_handle(stream)))
        self._mesh = DeviceGeometry("curves", n, 4 * n)

    def _is_custom_kind(self):
        """The accel holds spheres, cylinders or curves: its occlusion queries go through nrtOccludedBatchPrims*_f32."""
        m = self._mesh
        return isinstance(m, (SphereGeometry, CylinderGeometry, CurveGeometry)) or (isinstance(m, DeviceGeometry) and m.kind in ("spheres", "curves"))

    def _is_curves(self):
        m = self._mesh
        return isinstance(m, CurveGeometry) or (isinstance(m, DeviceGeometry) and m.kind == "curves")

    def BuildCurrent(self, options=None):
        """nrtBuild over the primitives last set (SetMesh, SetMeshDevice, SetSpheresDevice or SetCurvesDevice).  Returns False iff there are none."""
        if options is not None:
            want = BUILD_OPTIONS_F32 if self.real == np.float32 else BUILD_OPTIONS_F64
            options = np.asarray(options, dtype=want).reshape(1)
        nn = ctypes.c_uint64(0)
        st = getattr(self._L, "nrtBuild_" + self._s)(self._h, _p(options), _p(self._stats.reshape(1)), ctypes.byref(nn))
        if st == capi.NRT_ERR_EMPTY:
            return False
        self._check(st)
        return True

    def BuildDevice(self, d_vertices, d_faces, options=None, stream=None):
        """SetMeshDevice + nrtBuild: Build() for a mesh that lives on the device.  Returns False iff the mesh is empty."""
        self.SetMeshDevice(d_vertices, d_faces, stream)
        return self.BuildCurrent(options)

    def GetStatistics(self):
        return self._stats.copy()

    def LastBuildMs(self):
        return float(self._L.nrtLastBuildMs(self._h))

    def LastTraverseMs(self):
        return float(self._L.nrtLastTraverseMs(self._h))

    def SetLaunchTiming(self, on):
        """nrtSetLaunchTiming: on = bracket every launch with timing events (+ a completion event); off (the default) = no event
        in the stream, the kernel publishes a completion record whose stamps LastTraverseMs() reads."""
        self._check(self._L.nrtSetLaunchTiming(self._h, 1 if on else 0))

    def SetTunable(self, name, value):
        """nrtSetTunable: scheduling / layout tunables by name (include/nanort_hip.h lists them)."""
        self._check(self._L.nrtSetTunable(self._h, name.encode(), int(value)))

    def GetTunable(self, name):
        v = ctypes.c_longlong(0)
        self._check(self._L.nrtGetTunable(self._h, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def LastKernelName(self):
        """The traversal kernel variant the most recent launch used (as rocprofv3 names it)."""
        return self._L.nrtLastKernelName(self._h).decode()

    def _tree_size(self):
        nn, ni = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._L.nrtTreeSize(self._h, ctypes.byref(nn), ctypes.byref(ni)))
        return int(nn.value), int(ni.value)

    def IsValid(self):
        return self._tree_size()[0] > 0

    def GetTree(self):
        nn, ni = self._tree_size()
        nodes = np.zeros((nn,), dtype=node_dtype(self.real))
        indices = np.zeros((ni,), dtype=np.uint32)
        if nn:
            self._check(getattr(self._L, "nrtGetTree_" + self._s)(self._h, _p(nodes), _p(indices)))
        return nodes, indices

    def GetNodes(self):
        return self.GetTree()[0]

    def GetIndices(self):
        return self.GetTree()[1]

    def BoundingBox(self):
        """BVHAccel::BoundingBox (reference nanort.h:792-804)."""
        nodes = self.GetNodes()
        if nodes.shape[0] == 0:
            m = np.finfo(self.real).max
            return np.full(3, m, self.real), np.full(3, -m, self.real)
        return nodes[0]["bmin"].copy(), nodes[0]["bmax"].copy()

    def SetTree(self, nodes, indices):
        """Adopt a tree built elsewhere (BVHAccel::Load, reference nanort.h:2219-2275)."""
        nodes = np.ascontiguousarray(nodes, dtype=node_dtype(self.real))
        indices = np.ascontiguousarray(indices, dtype=np.uint32)
        self._check(
            getattr(self._L, "nrtSetTree_" + self._s)(self._h, _p(nodes), nodes.shape[0], _p(indices), indices.shape[0])
        )

    def _refit_rows(self):
        """The context's vertex count (max(faces) + 1 of the mesh last set), or None when no triangle mesh is set (the library
        then refuses the refit before it reads any vertex)."""
        m = self._mesh
        if isinstance(m, DeviceGeometry) and m.kind == "triangles":
            return m.num_verts
        if not isinstance(m, TriangleMesh):
            return None
        return int(m.faces.max()) + 1 if m.num_faces else 0

    def Refit(self, vertices, vertex_stride_bytes=None):
        """New positions for the mesh's vertices, same faces and topology (include/nanort_hip.h, nrtRefit): the tree's boxes are
        recomputed bottom-up.  `vertices`: a numpy array of the accel's precision holding at least the context's vertex count of
        rows (max(faces) + 1), xyz first in each row; the row stride defaults to the array's own.  With an explicit
        `vertex_stride_bytes` the array is a C-contiguous block of at least (nv - 1) * stride + 3 * itemsize bytes."""
        v = np.asarray(vertices)
        if v.dtype != self.real:
            raise TypeError("vertex precision %s != accel precision %s" % (v.dtype, self.real))
        nv = self._refit_rows()
        if vertex_stride_bytes is None:
            v = np.ascontiguousarray(v.reshape(v.shape[0], -1) if v.ndim > 1 else v.reshape(-1, 3))
            if v.shape[1] < 3:
                raise ValueError("vertices must be [nv, k >= 3]")
            if nv is not None and v.shape[0] < nv:
                raise ValueError("vertices hold %d rows; the mesh has %d vertices" % (v.shape[0], nv))
            vertex_stride_bytes = v.strides[0]
        else:
            if not v.flags["C_CONTIGUOUS"]:
                raise ValueError("an explicit vertex_stride_bytes needs a C-contiguous array")
            need = (nv - 1) * int(vertex_stride_bytes) + 3 * v.itemsize if nv else 0
            if nv is not None and v.nbytes < need:
                raise ValueError("vertices hold %d bytes; %d vertices at stride %d need %d" % (v.nbytes, nv, int(vertex_stride_bytes), need))
        self._check(getattr(self._L, "nrtRefit_" + self._s)(self._h, _p(v), int(vertex_stride_bytes)))

    def RefitDevice(self, d_vertices, stream=None):
        """Refit from a torch tensor on the accel's device (nrtRefitDevice): shape [nv', k >= 3] with nv' at least the mesh's
        vertex count and stride(1) == 1 (the row stride is stride(0)), dtype of the accel's precision.  Asynchronous on `stream`
        (default: torch's current stream); keep the tensor unchanged until the stream reaches the refit."""
        import torch

        want = torch.float32 if self.real == np.float32 else torch.float64
        if d_vertices.dtype != want:
            raise TypeError("vertex dtype %s != accel precision %s" % (d_vertices.dtype, self.real))
        if d_vertices.dim() != 2 or d_vertices.shape[1] < 3 or d_vertices.stride(1) != 1:
            raise ValueError("vertices must be [nv, k >= 3] with stride(1) == 1")
        nv = self._refit_rows()
        if nv is not None and d_vertices.shape[0] < nv:
            raise ValueError("vertices hold %d rows; the mesh has %d vertices" % (d_vertices.shape[0], nv))
        if d_vertices.device.type != "cuda" or d_vertices.device.index != self.device:
            raise ValueError("vertices must live on cuda:%d" % self.device)
        stream = self._stream_handle(stream)
        stride = d_vertices.stride(0) * d_vertices.element_size()
        self._check(getattr(self._L, "nrtRefitDevice_" + self._s)(self._h, d_vertices.data_ptr(), stride, stream))

    def _refit_prims_layout(self):
        """(count, position floats, radius floats per primitive) of the spheres or curves last set, or None when the accel holds
        another kind (the library then refuses the refit, with the reason)."""
        m = self._mesh
        if isinstance(m, SphereGeometry) or (isinstance(m, DeviceGeometry) and m.kind == "spheres"):
            return m.num_faces, 3, 1
        if self._is_curves():
            return m.num_faces, 12, 4
        return None

    def _refit_prims_checked(self, positions, radii, numel):
        """The shapes of RefitPrims / RefitPrimsDevice against the kind and count, before the library is called: `numel` gives
        an array's element count.  Returns the primitive count to pass (0 when the accel holds another kind: the library refuses)."""
        lay = self._refit_prims_layout()
        if lay is None:
            return 0
        n, pf, rf = lay
        if numel(positions) != pf * n:
            raise ValueError("positions hold %d floats; %d primitives need %d" % (numel(positions), n, pf * n))
        if radii is not None and numel(radii) != rf * n:
            raise ValueError("radii hold %d floats; %d primitives need %d" % (numel(radii), n, rf * n))
        return n

    def RefitPrims(self, positions, radii=None):
        """New positions (and radii) for the spheres or curves last set, same count and topology (include/nanort_hip.h,
        nrtRefitPrims): the tree's boxes are recomputed bottom-up.  `positions`: float32, [n, 3] centres or [n, 4, 3] control
        points; `radii`: [n] or [n, 4], or None to keep the accel's radii."""
        p = np.ascontiguousarray(positions, dtype=np.float32)
        r = None if radii is None else np.ascontiguousarray(radii, dtype=np.float32)
        n = self._refit_prims_checked(p, r, lambda a: a.size)
        self._check(self._L.nrtRefitPrims_f32(self._h, _p(p), _p(r), n))

    def RefitPrimsDevice(self, d_positions, d_radii=None, stream=None):
        """RefitPrims from torch float32 tensors on the accel's device, contiguous (nrtRefitPrimsDevice).  Asynchronous on `stream`
        (default: torch's current stream); keep the tensors unchanged until the stream reaches the refit."""
        import torch

        for t, what in ((d_positions, "positions"), (d_radii, "radii")):
            if t is None:
                continue
            if t.dtype != torch.float32:
                raise TypeError("%s must be torch.float32" % what)
            if not t.is_contiguous():
                raise ValueError("%s must be contiguous" % what)
            self._on_device(t, what)
        n = self._refit_prims_checked(d_positions, d_radii, lambda t: t.numel())
        self._check(self._L.nrtRefitPrimsDevice_f32(self._h, d_positions.data_ptr(), None if d_radii is None else d_radii.data_ptr(), n,
                                                    self._stream_handle(stream)))

    # -- traverse -----------------------------------------------------------
    @staticmethod
    def _host_skip_ids(skip_prim_ids, n):
        """One uint32 skip id per ray (include/nanort_hip.h, "per-ray skip ids"), contiguous."""
        ids = np.ascontiguousarray(skip_prim_ids, dtype=np.uint32).reshape(-1)
        if ids.shape[0] != n:
            raise ValueError("skip_prim_ids: %d ids for %d rays" % (ids.shape[0], n))
        return ids

    @staticmethod
    def _device_skip_ids(d_skip_prim_ids, n):
        assert d_skip_prim_ids.numel() * d_skip_prim_ids.element_size() >= 4 * n, "skip_prim_ids: fewer ids than rays"
        return d_skip_prim_ids.data_ptr()

    def TraverseBatch(self, rays, options=None, skip_prim_ids=None):
        """N x BVHAccel::Traverse (reference nanort.h:2487-2556). Returns (hits, mask).  `skip_prim_ids`: one uint32 per ray, traced
        in the place of options.skip_prim_id for that ray (triangle meshes; nrtTraverseBatchSkip)."""
        rays = np.ascontiguousarray(rays, dtype=ray_dtype(self.real))
        n = rays.shape[0]
        mask = np.zeros((n,), dtype=np.uint8)
        options = _opts(options)
        if skip_prim_ids is not None:  # (the library refuses the primitive kinds that have no skip id)
            ids = self._host_skip_ids(skip_prim_ids, n)
            hits = np.zeros((n,), dtype=hit_dtype(self.real))
            self._check(getattr(self._L, "nrtTraverseBatchSkip_" + self._s)(self._h, _p(rays), n, _p(options), _p(ids), _p(hits), _p(mask)))
            return hits, mask
        if self._is_curves():  # the example's 40-byte CurveIntersection records
            from .wire import CURVE_HIT_F32

            hits = np.zeros((n,), dtype=CURVE_HIT_F32)
            self._check(self._L.nrtTraverseBatchCurves_f32(self._h, _p(rays), n, _p(options), _p(hits), _p(mask)))
            return hits, mask
        if isinstance(self._mesh, CylinderGeometry):  # the example's 28-byte CylinderIntersection records
            from .wire import CYL_HIT_F32

            hits = np.zeros((n,), dtype=CYL_HIT_F32)
            self._check(self._L.nrtTraverseBatchCylinders_f32(self._h, _p(rays), n, _p(options), _p(hits), _p(mask)))
            return hits, mask
        hits = np.zeros((n,), dtype=hit_dtype(self.real))
        self._check(
            getattr(self._L, "nrtTraverseBatch_" + self._s)(self._h, _p(rays), n, _p(options), _p(hits), _p(mask))
        )
        return hits, mask

    def TraverseBatchDevice(self, d_rays, d_hits, d_mask=None, options=None, stream=None, skip_prim_ids=None):
        """Same on HBM-resident torch uint8 tensors (raw PODs), async on `stream`
        (default: torch's current stream).  `skip_prim_ids`: a device tensor of one uint32 per ray (nrtTraverseBatchSkipDevice)."""
        cyl, curves = isinstance(self._mesh, CylinderGeometry), self._is_curves()
        hsz = 28 if cyl else (40 if curves else hit_dtype(self.real).itemsize)
        n = self._n_rays(d_rays)
        assert d_hits.numel() * d_hits.element_size() >= n * hsz
        stream = self._stream_handle(stream)
        options = _opts(options)
        if skip_prim_ids is not None:
            self._check(getattr(self._L, "nrtTraverseBatchSkipDevice_" + self._s)(
                self._h, d_rays.data_ptr(), n, _p(options), self._device_skip_ids(skip_prim_ids, n), d_hits.data_ptr(),
                None if d_mask is None else d_mask.data_ptr(), stream))
            return n
        if curves:
            self._check(self._L.nrtTraverseBatchCurvesDevice_f32(
                self._h, d_rays.data_ptr(), n, _p(options), d_hits.data_ptr(), None if d_mask is None else d_mask.data_ptr(), stream))
            return n
        if cyl:
            self._check(self._L.nrtTraverseBatchCylindersDevice_f32(
                self._h, d_rays.data_ptr(), n, _p(options), d_hits.data_ptr(), None if d_mask is None else d_mask.data_ptr(), stream))
            return n
        self._check(
            getattr(self._L, "nrtTraverseBatchDevice_" + self._s)(
                self._h, d_rays.data_ptr(), n, _p(options), d_hits.data_ptr(),
                None if d_mask is None else d_mask.data_ptr(), stream,
            )
        )
        return n

    # -- closest point ------------------------------------------------------
    def ClosestPointBatch(self, points, max_dist=np.inf, options=None):
        """The nearest face of the mesh to each point and where on it (nrtClosestPointBatch; the rule: include/nanort_closest.h).
        `points`: [n, 3] coordinates with `max_dist` a scalar or one value per point, or a wire.point_dtype record array (then
        `max_dist` is not read).  Returns (records, found): wire.closest_dtype records and a uint8 per point."""
        from .wire import closest_dtype

        return self._point_query("nrtClosestPointBatch_", closest_dtype(self.real), points, max_dist, options)

    def ClosestPointBatchDevice(self, d_points, d_out, d_found=None, options=None, stream=None):
        """Same on HBM-resident torch tensors of raw records (wire.point_dtype in, wire.closest_dtype out, a byte per point in
        `d_found`), asynchronous on `stream` (default: torch's current stream).  Returns the number of points."""
        return self._point_query_device("nrtClosestPointBatchDevice_", d_points, d_out, d_found, options, stream)

    # -- signed distance ----------------------------------------------------
    def SignedDistanceBatch(self, points, max_dist=np.inf, options=None):
        """ClosestPointBatch, and on which side of the surface each point lies (nrtSignedDistanceBatch; the rule:
        include/nanort_sdf.h, angle-weighted pseudonormals).  Returns (records, found): wire.signed_dtype records — `feature` holds
        the feature of the face that holds the nearest point in bits 0..2 and wire.SIGNED_INSIDE when the point is inside."""
        from .wire import signed_dtype

        return self._point_query("nrtSignedDistanceBatch_", signed_dtype(self.real), points, max_dist, options)

    def SignedDistanceBatchDevice(self, d_points, d_out, d_found=None, options=None, stream=None):
        """Same on HBM-resident torch tensors of raw records (wire.point_dtype in, wire.signed_dtype out), asynchronous on `stream`."""
        return self._point_query_device("nrtSignedDistanceBatchDevice_", d_points, d_out, d_found, options, stream)

    def FeatureNormals(self):
        """The pseudonormals of the triangle mesh as the library derived them on the GPU (nrtGetFeatureNormals): (face_normals
        [num_faces, 4, 3] — the unit normal and the edge normals of ab, ac, bc — and vertex_normals [num_verts, 3])."""
        m = self._mesh
        nv = self._refit_rows()
        if nv is None:
            raise ValueError("FeatureNormals: no triangle mesh is set")
        fn = np.zeros((int(m.num_faces), 4, 3), dtype=self.real)
        vn = np.zeros((int(nv), 3), dtype=self.real)
        self._check(getattr(self._L, "nrtGetFeatureNormals_" + self._s)(self._h, _p(fn), _p(vn)))
        return fn, vn

    # -- nearest faces -------------------------------------------------------
    def NearestFacesBatch(self, points, max_faces, max_dist=np.inf, options=None):
        """The `max_faces` (1..capi.NRT_MAX_NEAREST) nearest faces of the mesh to each point, in ascending (dist2, prim_id) order
        (nrtNearestFacesBatch; the rule: include/nanort_closest.h).  `points`, `max_dist`: as ClosestPointBatch's.  Returns
        (records[n, max_faces], counts): wire.closest_dtype records — row i holds counts[i] found records, then not-found ones — and a
        uint32 per point."""
        from .wire import closest_dtype

        pts = self._point_records(points, max_dist)
        n, k = pts.shape[0], int(max_faces)
        out = np.zeros((n, k if 0 < k <= capi.NRT_MAX_NEAREST else 0), dtype=closest_dtype(self.real))  # (a K outside 1..64: the library refuses)
        counts = np.zeros((n,), dtype=np.uint32)
        options = _opts(options)
        self._check(getattr(self._L, "nrtNearestFacesBatch_" + self._s)(self._h, _p(pts), n, k, _p(options), _p(out), _p(counts)))
        return out, counts

    def NearestFacesBatchDevice(self, d_points, max_faces, d_out, d_counts=None, options=None, stream=None):
        """Same on HBM-resident torch tensors of raw records (wire.point_dtype in, max_faces wire.closest_dtype records per point out, a
        uint32 per point in `d_counts`), asynchronous on `stream` (default: torch's current stream).  Returns the number of points."""
        from .wire import closest_dtype, point_dtype

        for t, what in ((d_points, "d_points"), (d_out, "d_out"), (d_counts, "d_counts")):
            if t is not None:
                self._on_device(t, what)
        n, k = d_points.numel() * d_points.element_size() // point_dtype(self.real).itemsize, int(max_faces)
        if d_out.numel() * d_out.element_size() < n * k * closest_dtype(self.real).itemsize:
            raise ValueError("d_out holds fewer than max_faces records per point of d_points")
        if d_counts is not None and d_counts.numel() * d_counts.element_size() < 4 * n:
            raise ValueError("d_counts holds fewer words than d_points holds points")
        options = _opts(options)
        self._check(getattr(self._L, "nrtNearestFacesBatchDevice_" + self._s)(
            self._h, d_points.data_ptr(), n, k, _p(options), d_out.data_ptr(), None if d_counts is None else d_counts.data_ptr(),
            self._stream_handle(stream)))
        return n

    def _point_records(self, points, max_dist):
        from .wire import point_dtype

        pd = point_dtype(self.real)
        if isinstance(points, np.ndarray) and points.dtype == pd:
            return np.ascontiguousarray(points).reshape(-1)
        xyz = np.asarray(points, dtype=self.real).reshape(-1, 3)
        pts = np.zeros((xyz.shape[0],), dtype=pd)
        pts["p"] = xyz
        pts["max_dist"] = np.asarray(max_dist, dtype=self.real)
        return pts

    def _point_query(self, fn, record_dtype, points, max_dist, options):
        pts = self._point_records(points, max_dist)
        n = pts.shape[0]
        out = np.zeros((n,), dtype=record_dtype)
        found = np.zeros((n,), dtype=np.uint8)
        options = _opts(options)
        self._check(getattr(self._L, fn + self._s)(self._h, _p(pts), n, _p(options), _p(out), _p(found)))
        return out, found

    def _point_query_device(self, fn, d_points, d_out, d_found, options, stream):
        from .wire import closest_dtype, point_dtype

        for t, what in ((d_points, "d_points"), (d_out, "d_out"), (d_found, "d_found")):
            if t is not None:
                self._on_device(t, what)
        n = d_points.numel() * d_points.element_size() // point_dtype(self.real).itemsize
        if d_out.numel() * d_out.element_size() < n * closest_dtype(self.real).itemsize:  # (both record kinds have this size)
            raise ValueError("d_out holds fewer records than d_points holds points")
        if d_found is not None and d_found.numel() * d_found.element_size() < n:
            raise ValueError("d_found holds fewer bytes than d_points holds points")
        options = _opts(options)
        self._check(getattr(self._L, fn + self._s)(
            self._h, d_points.data_ptr(), n, _p(options), d_out.data_ptr(), None if d_found is None else d_found.data_ptr(),
            self._stream_handle(stream)))
        return n

    def TraverseBatchesDevice(self, batches, options=None, stream=None, skip_prim_ids=None):
        """nrtTraverseBatchesDevice: several independent batches — a list of (d_rays, d_hits, d_mask or None, n or None[, "occlusion"])
        torch uint8 tensors — walked by ONE persistent launch (asynchronous on `stream`).  A batch marked "occlusion" is an
        occlusion query: only its d_mask is written (d_hits may be None).  Returns the ray counts.  `skip_prim_ids`: a list with
        one entry per batch, a device tensor of one uint32 per ray or None (that batch uses options.skip_prim_id)."""
        hsz = hit_dtype(self.real).itemsize
        nb = len(batches)
        rays = (ctypes.c_void_p * nb)()
        hits = (ctypes.c_void_p * nb)()
        masks = (ctypes.c_void_p * nb)()
        counts = (ctypes.c_uint64 * nb)()
        flags = (ctypes.c_uint32 * nb)()
        for k, b in enumerate(batches):
            d_rays, d_hits, d_mask = b[0], b[1], b[2]
            n = b[3] if len(b) > 3 and b[3] is not None else self._n_rays(d_rays)
            occ = len(b) > 4 and b[4] == "occlusion"
            assert occ or d_hits.numel() * d_hits.element_size() >= n * hsz
            flags[k] = 1 if occ else 0
            rays[k], hits[k], counts[k] = d_rays.data_ptr(), (None if d_hits is None else d_hits.data_ptr()), n
            masks[k] = None if d_mask is None else d_mask.data_ptr()
        stream = self._stream_handle(stream)
        options = _opts(options)
        if skip_prim_ids is not None:
            assert len(skip_prim_ids) == nb, "skip_prim_ids: one entry per batch"
            ids = (ctypes.c_void_p * nb)()
            for k, t in enumerate(skip_prim_ids):
                ids[k] = None if t is None else self._device_skip_ids(t, counts[k])
            self._check(getattr(self._L, "nrtTraverseBatchesSkipDevice_" + self._s)(self._h, nb, rays, counts, _p(options), ids, hits, masks, flags,
                                                                                  stream))
            return [int(c) for c in counts]
        self._check(getattr(self._L, "nrtTraverseBatchesDevice_" + self._s)(self._h, nb, rays, counts, _p(options), hits, masks, flags, stream))
        return [int(c) for c in counts]

    def TraverseBatches(self, batches, options=None, skip_prim_ids=None):
        """nrtTraverseBatches: several independent HOST batches — a list of ray arrays or (rays, "occlusion") pairs — uploaded
        together, walked by ONE persistent launch, downloaded together.  Returns a list of (hits, mask) per closest-hit batch
        and (None, mask) per occlusion batch: exactly what TraverseBatch / OccludedBatch return for each of them.
        `skip_prim_ids`: a list with one entry per batch, an array of one uint32 per ray or None (that batch uses options.skip_prim_id)."""
        RAY, HIT = ray_dtype(self.real), hit_dtype(self.real)
        nb = len(batches)
        rays = (ctypes.c_void_p * nb)()
        hits = (ctypes.c_void_p * nb)()
        masks = (ctypes.c_void_p * nb)()
        counts = (ctypes.c_uint64 * nb)()
        flags = (ctypes.c_uint32 * nb)()
        keep, out = [], []
        for k, b in enumerate(batches):
            occ = isinstance(b, tuple) and len(b) > 1 and b[1] == "occlusion"
            r = np.ascontiguousarray(b[0] if isinstance(b, tuple) else b, dtype=RAY)
            h = None if occ else np.zeros((r.shape[0],), dtype=HIT)
            m = np.zeros((r.shape[0],), dtype=np.uint8)
            keep.append(r)
            out.append((h, m))
            rays[k], counts[k], flags[k] = (r.ctypes.data if r.shape[0] else None), r.shape[0], (1 if occ else 0)
            hits[k] = None if (occ or not r.shape[0]) else h.ctypes.data
            masks[k] = m.ctypes.data if r.shape[0] else None
        options = _opts(options)
        if skip_prim_ids is not None:
            assert len(skip_prim_ids) == nb, "skip_prim_ids: one entry per batch"
            ids = (ctypes.c_void_p * nb)()
            for k, a in enumerate(skip_prim_ids):
                if a is None or not counts[k]:
                    ids[k] = None
                    continue
                a = self._host_skip_ids(a, counts[k])
                keep.append(a)
                ids[k] = a.ctypes.data
            self._check(getattr(self._L, "nrtTraverseBatchesSkip_" + self._s)(self._h, nb, rays, counts, _p(options), ids, hits, masks, flags))
            return out
        self._check(getattr(self._L, "nrtTraverseBatches_" + self._s)(self._h, nb, rays, counts, _p(options), hits, masks, flags))
        return out

    def OccludedBatch(self, rays, options=None, skip_prim_ids=None):
        """Opt-in extension: only the hit flags of TraverseBatch() (0 / 1: `mask != 0` of it), each ray stopping at the first
        primitive that settles it.  Sphere, cylinder and curve accels go through nrtOccludedBatchPrims_f32.
        `skip_prim_ids`: as for TraverseBatch (nrtOccludedBatchSkip; triangle meshes only: raises on another kind)."""
        rays = np.ascontiguousarray(rays, dtype=ray_dtype(self.real))
        mask = np.zeros((rays.shape[0],), dtype=np.uint8)
        options = _opts(options)
        if self._is_custom_kind():
            if skip_prim_ids is not None:
                raise ValueError("skip_prim_ids: triangle meshes only (the sphere, cylinder and curve intersectors have no skip id)")
            self._check(self._L.nrtOccludedBatchPrims_f32(self._h, _p(rays), rays.shape[0], _p(options), _p(mask)))
            return mask
        if skip_prim_ids is not None:
            ids = self._host_skip_ids(skip_prim_ids, rays.shape[0])
            self._check(getattr(self._L, "nrtOccludedBatchSkip_" + self._s)(self._h, _p(rays), rays.shape[0], _p(options), _p(ids), _p(mask)))
            return mask
        self._check(getattr(self._L, "nrtOccludedBatch_" + self._s)(self._h, _p(rays), rays.shape[0], _p(options), _p(mask)))
        return mask

    def OccludedBatchDevice(self, d_rays, d_mask, options=None, stream=None, skip_prim_ids=None):
        n = self._n_rays(d_rays)
        assert d_mask.numel() >= n
        stream = self._stream_handle(stream)
        options = _opts(options)
        if self._is_custom_kind():  # (as OccludedBatch)
            if skip_prim_ids is not None:
                raise ValueError("skip_prim_ids: triangle meshes only (the sphere, cylinder and curve intersectors have no skip id)")
            self._check(self._L.nrtOccludedBatchPrimsDevice_f32(self._h, d_rays.data_ptr(), n, _p(options), d_mask.data_ptr(), stream))
            return n
        if skip_prim_ids is not None:
            self._check(getattr(self._L, "nrtOccludedBatchSkipDevice_" + self._s)(self._h, d_rays.data_ptr(), n, _p(options),
                                                                                self._device_skip_ids(skip_prim_ids, n), d_mask.data_ptr(),
                                                                                stream))
            return n
        self._check(getattr(self._L, "nrtOccludedBatchDevice_" + self._s)(self._h, d_rays.data_ptr(), n, _p(options), d_mask.data_ptr(), stream))
        return n

    # -- motion blur (include/nanort_hip.h, "motion blur") -------------------
    def _host_times(self, times, n):
        """One time per ray in the accel's precision, contiguous (None: every ray at time 0)."""
        if times is None:
            return None
        t = np.ascontiguousarray(times, dtype=self.real).reshape(-1)
        if t.shape[0] != n:
            raise ValueError("times: %d values for %d rays" % (t.shape[0], n))
        return t

    def _device_times(self, d_times, n):
        if d_times is None:
            return None
        assert d_times.numel() * d_times.element_size() >= self.real.itemsize * n, "times: fewer values than rays"
        return d_times.data_ptr()

    def TraverseBatchMotion(self, rays, times, options=None):
        """nrtTraverseBatchMotion: TraverseBatch with one shutter time per ray over the mesh's two vertex keyframes.  Returns
        (hits, mask)."""
        rays = np.ascontiguousarray(rays, dtype=ray_dtype(self.real))
        n = rays.shape[0]
        t = self._host_times(times, n)
        hits = np.zeros((n,), dtype=hit_dtype(self.real))
        mask = np.zeros((n,), dtype=np.uint8)
        options = _opts(options)
        self._check(getattr(self._L, "nrtTraverseBatchMotion_" + self._s)(self._h, _p(rays), _p(t), n, _p(options), _p(hits), _p(mask)))
        return hits, mask

    def TraverseBatchMotionDevice(self, d_rays, d_times, d_hits, d_mask=None, options=None, stream=None):
        """Same on HBM-resident torch tensors (raw PODs; `d_times`: one value of the accel's precision per ray, or None),
        asynchronous on `stream` (default: torch's current stream).  Returns n."""
        hsz = hit_dtype(self.real).itemsize
        n = self._n_rays(d_rays)
        assert d_hits.numel() * d_hits.element_size() >= n * hsz
        options = _opts(options)
        self._check(getattr(self._L, "nrtTraverseBatchMotionDevice_" + self._s)(
            self._h, d_rays.data_ptr(), self._device_times(d_times, n), n, _p(options), d_hits.data_ptr(),
            None if d_mask is None else d_mask.data_ptr(), self._stream_handle(stream)))
        return n

    def OccludedBatchMotion(self, rays, times, options=None):
        """nrtOccludedBatchMotion: only the hit flags of TraverseBatchMotion, each ray stopping at the first triangle that settles it."""
        rays = np.ascontiguousarray(rays, dtype=ray_dtype(self.real))
        n = rays.shape[0]
        t = self._host_times(times, n)
        mask = np.zeros((n,), dtype=np.uint8)
        options = _opts(options)
        self._check(getattr(self._L, "nrtOccludedBatchMotion_" + self._s)(self._h, _p(rays), _p(t), n, _p(options), _p(mask)))
        return mask

    def OccludedBatchMotionDevice(self, d_rays, d_times, d_mask, options=None, stream=None):
        n = self._n_rays(d_rays)
        assert d_mask.numel() >= n
        options = _opts(options)
        self._check(getattr(self._L, "nrtOccludedBatchMotionDevice_" + self._s)(
            self._h, d_rays.data_ptr(), self._device_times(d_times, n), n, _p(options), d_mask.data_ptr(), self._stream_handle(stream)))
        return n

    # -- visibility masks (include/nanort_hip.h, "visibility masks") ----------
    def SetPrimMasks(self, masks, stream=None):
        """nrtSetPrimMasks / nrtSetPrimMasksDevice: one uint32 per face of the triangle mesh last set, in face order; a triangle
        exists for a ray iff (prim_mask & ray_mask) != 0.  `masks`: a numpy array (or anything numpy converts), or a torch tensor on
        the accel's device (int32 or uint32, contiguous: read as u32 on `stream`, default torch's current stream); None removes the
        masks.  The tree stays as it is."""
        if masks is None:
            self._check(self._L.nrtSetPrimMasks(self._h, None, 0))
            return
        if hasattr(masks, "data_ptr"):  # a torch tensor
            return self.SetPrimMasksDevice(masks, stream)
        m = np.ascontiguousarray(masks, dtype=np.uint32).reshape(-1)
        self._check(self._L.nrtSetPrimMasks(self._h, _p(m), m.shape[0]))

    def SetPrimMasksDevice(self, d_masks, stream=None):
        """nrtSetPrimMasksDevice: the masks from a contiguous torch tensor of 32-bit integers on the accel's device, copied on
        `stream` (default: torch's current stream); returns when the accel owns its copy.  None removes the masks."""
        if d_masks is None:
            self._check(self._L.nrtSetPrimMasksDevice(self._h, None, 0, self._stream_handle(stream)))
            return
        if d_masks.element_size() != 4 or d_masks.is_floating_point() or not d_masks.is_contiguous():
            raise TypeError("masks: a contiguous tensor of 32-bit integers")
        self._on_device(d_masks, "masks")
        self._check(self._L.nrtSetPrimMasksDevice(self._h, d_masks.data_ptr(), int(d_masks.numel()), self._stream_handle(stream)))

    def _host_ray_masks(self, ray_masks, n):
        """One uint32 per ray, contiguous (None: every ray 0xFFFFFFFF)."""
        if ray_masks is None:
            return None
        v = np.ascontiguousarray(ray_masks, dtype=np.uint32).reshape(-1)
        if v.shape[0] != n:
            raise ValueError("ray_masks: %d values for %d rays" % (v.shape[0], n))
        return v

    def _device_ray_masks(self, d_ray_masks, n):
        if d_ray_masks is None:
            return None
        assert d_ray_masks.numel() * d_ray_masks.element_size() >= 4 * n, "ray_masks: fewer values than rays"
        return d_ray_masks.data_ptr()

    def TraverseBatchMasked(self, rays, ray_masks, options=None):
        """nrtTraverseBatchMasked: TraverseBatch in which ray i sees only the triangles whose mask shares a bit with ray_masks[i]
        (None: every ray 0xFFFFFFFF).  Returns (hits, mask)."""
        rays = np.ascontiguousarray(rays, dtype=ray_dtype(self.real))
        n = rays.shape[0]
        v = self._host_ray_masks(ray_masks, n)
        hits = np.zeros((n,), dtype=hit_dtype(self.real))
        mask = np.zeros((n,), dtype=np.uint8)
        options = _opts(options)
        self._check(getattr(self._L, "nrtTraverseBatchMasked_" + self._s)(self._h, _p(rays), _p(v), n, _p(options), _p(hits), _p(mask)))
        return hits, mask

    def TraverseBatchMaskedDevice(self, d_rays, d_ray_masks, d_hits, d_mask=None, options=None, stream=None):
        """Same on HBM-resident torch tensors (raw PODs; `d_ray_masks`: one 32-bit word per ray, or None), asynchronous on `stream`
        (default: torch's current stream).  Returns n."""
        hsz = hit_dtype(self.real).itemsize
        n = self._n_rays(d_rays)
        assert d_hits.numel() * d_hits.element_size() >= n * hsz
        options = _opts(options)
        self._check(getattr(self._L, "nrtTraverseBatchMaskedDevice_" + self._s)(
            self._h, d_rays.data_ptr(), self._device_ray_masks(d_ray_masks, n), n, _p(options), d_hits.data_ptr(),
            None if d_mask is None else d_mask.data_ptr(), self._stream_handle(stream)))
        return n

    def OccludedBatchMasked(self, rays, ray_masks, options=None):
        """nrtOccludedBatchMasked: only the hit flags of TraverseBatchMasked, each ray stopping at the first triangle that settles it."""
        rays = np.ascontiguousarray(rays, dtype=ray_dtype(self.real))
        n = rays.shape[0]
        v = self._host_ray_masks(ray_masks, n)
        mask = np.zeros((n,), dtype=np.uint8)
        options = _opts(options)
        self._check(getattr(self._L, "nrtOccludedBatchMasked_" + self._s)(self._h, _p(rays), _p(v), n, _p(options), _p(mask)))
        return mask

    def OccludedBatchMaskedDevice(self, d_rays, d_ray_masks, d_mask, options=None, stream=None):
        n = self._n_rays(d_rays)
        assert d_mask.numel() >= n
        options = _opts(options)
        self._check(getattr(self._L, "nrtOccludedBatchMaskedDevice_" + self._s)(
            self._h, d_rays.data_ptr(), self._device_ray_masks(d_ray_masks, n), n, _p(options), d_mask.data_ptr(), self._stream_handle(stream)))
        return n

    # -- one descriptor for every triangle ray query (include/nanort_hip.h) ----
    @staticmethod
    def _query_flags(times, ray_masks, motion, masked, occlusion):
        motion = (times is not None) if motion is None else bool(motion)
        masked = (ray_masks is not None) if masked is None else bool(masked)
        return (capi.NRT_QUERY_OCCLUSION if occlusion else 0) | (capi.NRT_QUERY_MOTION if motion else 0) | (capi.NRT_QUERY_MASKED if masked else 0)

    def QueryBatch(self, rays, times=None, ray_masks=None, skip_prim_ids=None, motion=None, masked=None, occlusion=False, options=None):
        """nrtQueryBatch: one call for whichever of a shutter time, a visibility word and a skip id every ray carries.  `motion` /
        `masked`: whether the query interpolates the keyframes / applies the masks (None: iff the array is given; True with no array:
        every ray at time 0 / with the word 0xFFFFFFFF).  Returns (hits, mask), or with `occlusion` only the flags."""
        rays = np.ascontiguousarray(rays, dtype=ray_dtype(self.real))
        n = rays.shape[0]
        t = self._host_times(times, n)
        v = self._host_ray_masks(ray_masks, n)
        ids = None if skip_prim_ids is None else self._host_skip_ids(skip_prim_ids, n)
        hits = None if occlusion else np.zeros((n,), dtype=hit_dtype(self.real))
        mask = np.zeros((n,), dtype=np.uint8)
        options = _opts(options)
        q = capi.RayQuery(ctypes.sizeof(capi.RayQuery), self._query_flags(times, ray_masks, motion, masked, occlusion), rays.ctypes.data, n,
                          None if options is None else options.ctypes.data, None if ids is None else ids.ctypes.data,
                          None if t is None else t.ctypes.data, None if v is None else v.ctypes.data,
                          None if hits is None else hits.ctypes.data, mask.ctypes.data)
        self._check(getattr(self._L, "nrtQueryBatch_" + self._s)(self._h, ctypes.addressof(q)))
        return mask if occlusion else (hits, mask)

    def QueryBatchDevice(self, d_rays, d_hits=None, d_mask=None, times=None, ray_masks=None, skip_prim_ids=None, motion=None, masked=None,
                         occlusion=False, options=None, stream=None):
        """nrtQueryBatchDevice: the same on HBM-resident torch tensors (raw PODs; `times` in the accel's precision, `ray_masks` and
        `skip_prim_ids` 32-bit words, one per ray), asynchronous on `stream` (default: torch's current stream).  With `occlusion`
        only `d_mask` is written and `d_hits` is not read.  Returns n."""
        n = self._n_rays(d_rays)
        if not occlusion and d_hits is not None:
            assert d_hits.numel() * d_hits.element_size() >= n * hit_dtype(self.real).itemsize
        assert d_mask is None or d_mask.numel() >= n
        options = _opts(options)
        q = capi.RayQuery(ctypes.sizeof(capi.RayQuery), self._query_flags(times, ray_masks, motion, masked, occlusion), d_rays.data_ptr(), n,
                          None if options is None else options.ctypes.data,
                          None if skip_prim_ids is None else self._device_skip_ids(skip_prim_ids, n), self._device_times(times, n),
                          self._device_ray_masks(ray_masks, n), None if d_hits is None else d_hits.data_ptr(),
                          None if d_mask is None else d_mask.data_ptr())
        self._check(getattr(self._L, "nrtQueryBatchDevice_" + self._s)(self._h, ctypes.addressof(q), self._stream_handle(stream)))
        return n

    def MultiHitTraverseBatch(self, rays, max_hits, options=None):
        """The K = max_hits frontmost hits of every ray (include/nanort_hip.h, nrtMultiHitTraverseBatch): returns (hits[n, K],
        counts[n]); row i holds ray i's hits by ascending (t, prim_id), then miss records {0, 0, max_t, 0xFFFFFFFF}."""
        rays = np.ascontiguousarray(rays, dtype=ray_dtype(self.real))
        n = rays.shape[0]
        hits = np.zeros((n, max(int(max_hits), 1)), dtype=hit_dtype(self.real))
        counts = np.zeros((n,), dtype=np.uint32)
        options = _opts(options)
        self._check(getattr(self._L, "nrtMultiHitTraverseBatch_" + self._s)(self._h, _p(rays), n, int(max_hits), _p(options), _p(hits), _p(counts)))
        return hits, counts

    def MultiHitTraverseBatchDevice(self, d_rays, max_hits, d_hits, d_counts=None, options=None, stream=None):
        """Same on HBM-resident torch tensors (raw PODs: d_hits holds n * max_hits records, d_counts n uint32), asynchronous on
        `stream` (default: torch's current stream).  Returns n."""
        hsz = hit_dtype(self.real).itemsize
        n = self._n_rays(d_rays)
        assert d_hits.numel() * d_hits.element_size() >= n * int(max_hits) * hsz
        assert d_counts is None or d_counts.numel() * d_counts.element_size() >= n * 4
        stream = self._stream_handle(stream)
        options = _opts(options)
        self._check(getattr(self._L, "nrtMultiHitTraverseBatchDevice_" + self._s)(
            self._h, d_rays.data_ptr(), n, int(max_hits), _p(options), d_hits.data_ptr(),
            None if d_counts is None else d_counts.data_ptr(), stream))
        return n

    def MultiHitQueryBatch(self, rays, max_hits, times=None, ray_masks=None, skip_prim_ids=None, motion=None, masked=None, options=None):
        """nrtMultiHitQueryBatch: MultiHitTraverseBatch for whichever of a shutter time, a visibility word and a skip id every ray
        carries.  `motion` / `masked`: as QueryBatch's (None: iff the array is given).  Returns (hits[n, K], counts[n])."""
        rays = np.ascontiguousarray(rays, dtype=ray_dtype(self.real))
        n = rays.shape[0]
        t = self._host_times(times, n)
        v = self._host_ray_masks(ray_masks, n)
        ids = None if skip_prim_ids is None else self._host_skip_ids(skip_prim_ids, n)
        hits = np.zeros((n, max(int(max_hits), 1)), dtype=hit_dtype(self.real))
        counts = np.zeros((n,), dtype=np.uint32)
        options = _opts(options)
        q = capi.MultiHitQuery(ctypes.sizeof(capi.MultiHitQuery), self._query_flags(times, ray_masks, motion, masked, False), rays.ctypes.data, n,
                               None if options is None else options.ctypes.data, None if ids is None else ids.ctypes.data,
                               None if t is None else t.ctypes.data, None if v is None else v.ctypes.data, hits.ctypes.data, counts.ctypes.data,
                               int(max_hits), 0)
        self._check(getattr(self._L, "nrtMultiHitQueryBatch_" + self._s)(self._h, ctypes.addressof(q)))
        return hits, counts

    def MultiHitQueryBatchDevice(self, d_rays, max_hits, d_hits, d_counts=None, times=None, ray_masks=None, skip_prim_ids=None, motion=None,
                                 masked=None, options=None, stream=None):
        """nrtMultiHitQueryBatchDevice: the same on HBM-resident torch tensors (raw PODs: d_hits holds n * max_hits records, d_counts n
        uint32; `times` in the accel's precision, `ray_masks` and `skip_prim_ids` 32-bit words, one per ray), asynchronous on `stream`
        (default: torch's current stream).  Returns n."""
        n = self._n_rays(d_rays)
        assert d_hits.numel() * d_hits.element_size() >= n * int(max_hits) * hit_dtype(self.real).itemsize
        assert d_counts is None or d_counts.numel() * d_counts.element_size() >= n * 4
        options = _opts(options)
        q = capi.MultiHitQuery(ctypes.sizeof(capi.MultiHitQuery), self._query_flags(times, ray_masks, motion, masked, False), d_rays.data_ptr(), n,
                               None if options is None else options.ctypes.data,
                               None if skip_prim_ids is None else self._device_skip_ids(skip_prim_ids, n), self._device_times(times, n),
                               self._device_ray_masks(ray_masks, n), d_hits.data_ptr(), None if d_counts is None else d_counts.data_ptr(),
                               int(max_hits), 0)
        self._check(getattr(self._L, "nrtMultiHitQueryBatchDevice_" + self._s)(self._h, ctypes.addressof(q), self._stream_handle(stream)))
        return n

    def TraverseCountDevice(self, d_rays, options=None):
        """Work counters (nodes visited, leaves, triangle tests, max stack) of one batch."""
        n = self._n_rays(d_rays)
        c = capi.TraceCounters()
        options = _opts(options)
        self._check(
            getattr(self._L, "nrtTraverseCountDevice_" + self._s)(self._h, d_rays.data_ptr(), n, _p(options), ctypes.byref(c))
        )
        return {
            "nodes_visited": int(c.nodes_visited),
            "leaves_tested": int(c.leaves_tested),
            "tris_tested": int(c.tris_tested),
            "max_stack": int(c.max_stack),
            "num_rays": int(n),
        }


class Scene:
    """nanosg::Scene<float, M> on one MI355X (reference examples/nanosg/nanosg.h:668-905): instanced two-level
    traversal.  Nodes are built `BVHAccel(np.float32)` objects plus nanosg's 4x4 local transform (row 3 =
    translation); `Traverse` of the reference becomes `TraverseBatch`."""

    def __init__(self, device=0):
        self._L = capi.lib()
        h = ctypes.c_void_p()
        st = self._L.nrtSceneCreate(int(device), ctypes.byref(h))
        if st != capi.NRT_OK:
            raise capi.NrtError(st, self._L.nrtSceneLastError(None).decode())
        self._h = h
        self._keep = []

    def close(self):
        if getattr(self, "_h", None):
            self._L.nrtSceneDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != capi.NRT_OK:
            raise capi.NrtError(st, self._L.nrtSceneLastError(self._h).decode())

    def AddNode(self, accel, local_xform):
        x = np.ascontiguousarray(local_xform, dtype=np.float32).reshape(16)
        nid = ctypes.c_uint32(0)
        self._check(self._L.nrtSceneAddNode_f32(self._h, accel._h, _p(x), ctypes.byref(nid)))
        self._keep.append(accel)
        return int(nid.value)

    def Commit(self):
        st = self._L.nrtSceneCommit(self._h)
        if st == capi.NRT_ERR_EMPTY:
            return False
        self._check(st)
        return True

    def GetBoundingBox(self):
        """Scene::GetBoundingBox (reference nanosg.h:761-769): (bmin, bmax) of a committed scene."""
        bmin = np.zeros(3, dtype=np.float32)
        bmax = np.zeros(3, dtype=np.float32)
        self._check(self._L.nrtSceneBounds_f32(self._h, _p(bmin), _p(bmax)))
        return bmin, bmax

    def NodeState(self, node_id):
        """xform, inv_xform, inv_xform33, inv_transpose_xform33 of a committed node (reference nanosg.h:397-437)."""
        out = np.zeros(64, dtype=np.float32)
        self._check(self._L.nrtSceneNodeState_f32(self._h, int(node_id), _p(out)))
        m = out.reshape(4, 4, 4)
        return {"xform": m[0], "inv_xform": m[1], "inv_xform33": m[2], "inv_transpose_xform33": m[3]}

    def SetTunable(self, name, value):
        """Scheduling knobs of the scene kernels (nrtSceneSetTunable): "single_pass", "trav_min", "refill_min", ..."""
        self._check(self._L.nrtSceneSetTunable(self._h, name.encode(), int(value)))

    def LastRedone(self):
        """Rays of the last call that the single-pass walk handed to the listing path (nrtSceneLastRedone)."""
        return int(self._L.nrtSceneLastRedone(self._h))

    def LastPath(self):
        """1: the last call went through the single-pass walk, 0: the listing path alone; 2: it was a closest-point query, whose one
        kernel is nrt::k_scene_closest_point<32> (nrtSceneLastPath)."""
        return int(self._L.nrtSceneLastPath(self._h))

    def TraverseBatch(self, rays):
        from .wire import RAY_F32, SCENE_HIT_F32

        rays = np.ascontiguousarray(rays, dtype=RAY_F32)
        hits = np.zeros((rays.shape[0],), dtype=SCENE_HIT_F32)
        mask = np.zeros((rays.shape[0],), dtype=np.uint8)
        self._check(self._L.nrtSceneTraverseBatch_f32(self._h, _p(rays), rays.shape[0], _p(hits), _p(mask)))
        return hits, mask

    def TraverseBatchDevice(self, d_rays, d_hits, d_mask=None):
        """Rays and results in HBM: torch uint8 tensors holding RAY_F32 records in, SCENE_HIT_F32 records (20 B) and the
        optional hit flags out.  Synchronous (see nrtSceneTraverseBatchDevice_f32); waits for torch's current stream first."""
        import torch

        from .wire import RAY_F32, SCENE_HIT_F32

        n = d_rays.numel() // RAY_F32.itemsize
        assert d_rays.is_cuda and d_hits.is_cuda and d_hits.numel() >= n * SCENE_HIT_F32.itemsize
        torch.cuda.current_stream().synchronize()
        self._check(self._L.nrtSceneTraverseBatchDevice_f32(self._h, d_rays.data_ptr(), n, d_hits.data_ptr(),
                                                            d_mask.data_ptr() if d_mask is not None else None))

    def OccludedBatch(self, rays):
        """Occlusion query (nrtSceneOccludedBatch_f32): the hit flags `TraverseBatch` would return, and nothing else — a ray
        stops at its first hit, no hit record is produced or copied."""
        from .wire import RAY_F32

        rays = np.ascontiguousarray(rays, dtype=RAY_F32)
        mask = np.zeros((rays.shape[0],), dtype=np.uint8)
        self._check(self._L.nrtSceneOccludedBatch_f32(self._h, _p(rays), rays.shape[0], _p(mask)))
        return mask

    def OccludedBatchDevice(self, d_rays, d_mask):
        """Rays and flags in HBM: torch uint8 tensors holding RAY_F32 records in, one flag byte per ray out.  Synchronous (see
        nrtSceneOccludedBatchDevice_f32); waits for torch's current stream first."""
        import torch

        from .wire import RAY_F32

        n = d_rays.numel() // RAY_F32.itemsize
        assert d_rays.is_cuda and d_mask.is_cuda and d_mask.numel() >= n
        torch.cuda.current_stream().synchronize()
        self._check(self._L.nrtSceneOccludedBatchDevice_f32(self._h, d_rays.data_ptr(), n, d_mask.data_ptr()))

    def SetNodeMasks(self, masks):
        """Instance visibility masks (nrtSceneSetNodeMasks): one uint32 per node in node-id order, or None = every node
        0xFFFFFFFF.  An instance exists for a ray of a masked query iff (node word & ray word) != 0.  No part of the top-level tree:
        before or after Commit, and a change needs no new Commit."""
        if masks is None:
            self._check(self._L.nrtSceneSetNodeMasks(self._h, None, 0))
            return
        masks = np.ascontiguousarray(masks, dtype=np.uint32)
        self._check(self._L.nrtSceneSetNodeMasks(self._h, _p(masks), masks.shape[0]))

    @staticmethod
    def _ray_words(ray_masks, n):
        if ray_masks is None:
            return None
        ray_masks = np.ascontiguousarray(ray_masks, dtype=np.uint32)
        assert ray_masks.shape == (n,), "one uint32 word per ray"
        return ray_masks

    def TraverseBatchMasked(self, rays, ray_masks=None):
        """`TraverseBatch` on the nodes each ray sees (nrtSceneTraverseBatchMasked_f32): `ray_masks` is one uint32 per ray,
        None = every ray 0xFFFFFFFF.  Node ids are this scene's."""
        from .wire import RAY_F32, SCENE_HIT_F32

        rays = np.ascontiguousarray(rays, dtype=RAY_F32)
        words = self._ray_words(ray_masks, rays.shape[0])
        hits = np.zeros((rays.shape[0],), dtype=SCENE_HIT_F32)
        mask = np.zeros((rays.shape[0],), dtype=np.uint8)
        self._check(self._L.nrtSceneTraverseBatchMasked_f32(self._h, _p(rays), _p(words), rays.shape[0],
                                                            _p(hits), _p(mask)))
        return hits, mask

    def TraverseBatchMaskedDevice(self, d_rays, d_ray_masks, d_hits, d_mask=None):
        """`TraverseBatchDevice` with the rays' words in HBM: `d_ray_masks` is a torch tensor of one 32-bit word per ray (or None).
        Synchronous (see nrtSceneTraverseBatchMaskedDevice_f32); waits for torch's current stream first."""
        import torch

        from .wire import RAY_F32, SCENE_HIT_F32

        n = d_rays.numel() // RAY_F32.itemsize
        assert d_rays.is_cuda and d_hits.is_cuda and d_hits.numel() >= n * SCENE_HIT_F32.itemsize
        assert d_ray_masks is None or (d_ray_masks.is_cuda and d_ray_masks.numel() * d_ray_masks.element_size() >= 4 * n)
        torch.cuda.current_stream().synchronize()
        self._check(self._L.nrtSceneTraverseBatchMaskedDevice_f32(self._h, d_rays.data_ptr(), d_ray_masks.data_ptr() if d_ray_masks is not None else None,
                                                                  n, d_hits.data_ptr(), d_mask.data_ptr() if d_mask is not None else None))

    def OccludedBatchMasked(self, rays, ray_masks=None):
        """`OccludedBatch` on the nodes each ray sees (nrtSceneOccludedBatchMasked_f32): the flags `TraverseBatchMasked` would
        return, and nothing else."""
        from .wire import RAY_F32

        rays = np.ascontiguousarray(rays, dtype=RAY_F32)
        words = self._ray_words(ray_masks, rays.shape[0])
        mask = np.zeros((rays.shape[0],), dtype=np.uint8)
        self._check(self._L.nrtSceneOccludedBatchMasked_f32(self._h, _p(rays), _p(words), rays.shape[0], _p(mask)))
        return mask

    def OccludedBatchMaskedDevice(self, d_rays, d_ray_masks, d_mask):
        """`OccludedBatchDevice` with the rays' words in HBM (see TraverseBatchMaskedDevice).  Synchronous."""
        import torch

        from .wire import RAY_F32

        n = d_rays.numel() // RAY_F32.itemsize
        assert d_rays.is_cuda and d_mask.is_cuda and d_mask.numel() >= n
        assert d_ray_masks is None or (d_ray_masks.is_cuda and d_ray_masks.numel() * d_ray_masks.element_size() >= 4 * n)
        torch.cuda.current_stream().synchronize()
        self._check(self._L.nrtSceneOccludedBatchMaskedDevice_f32(self._h, d_rays.data_ptr(), d_ray_masks.data_ptr() if d_ray_masks is not None else None,
                                                                  n, d_mask.data_ptr()))

    # -- one descriptor for the scene queries, with per-ray skip pairs (include/nanort_hip.h) ----
    @staticmethod
    def _scene_query_flags(ray_masks, skip_pairs, occlusion):
        return ((capi.NRT_SCENE_QUERY_OCCLUSION if occlusion else 0) | (capi.NRT_SCENE_QUERY_MASKED if ray_masks is not None else 0) |
                (capi.NRT_SCENE_QUERY_SKIP if skip_pairs is not None else 0))

    @staticmethod
    def _host_skip_pairs(skip_pairs, n):
        """(array to keep alive, address of ray 0's pair, stride): an (n, 2) uint32 array {prim_id, node_id}, or the SCENE_HIT_F32
        records of a previous wave, which are passed as they lie (their last two fields are the pair)."""
        from .wire import SCENE_HIT_F32

        if skip_pairs is None:
            return None, None, 0
        if getattr(skip_pairs, "dtype", None) == SCENE_HIT_F32:
            a = skip_pairs if skip_pairs.flags["C_CONTIGUOUS"] else np.ascontiguousarray(skip_pairs)
            assert a.shape == (n,), "one record per ray"
            return a, a.ctypes.data + SCENE_HIT_F32.fields["prim_id"][1], SCENE_HIT_F32.itemsize
        a = np.ascontiguousarray(skip_pairs, dtype=np.uint32)
        assert a.shape == (n, 2), "one {prim_id, node_id} pair per ray"
        return a, a.ctypes.data, 8

    def QueryBatch(self, rays, ray_masks=None, skip_pairs=None, occlusion=False):
        """nrtSceneQueryBatch_f32: `TraverseBatch` / `OccludedBatch` (with `ray_masks`: their Masked forms) in which ray i does not
        see primitive p of node n for its pair skip_pairs[i] = (p, n) — a bounce ray leaves the triangle it starts on.  `skip_pairs`:
        an (n, 2) uint32 array, or the SCENE_HIT_F32 records of the previous wave (passed strided, without a copy; a miss record skips
        nothing).  Returns (hits, mask), or with `occlusion` only the flags."""
        from .wire import RAY_F32, SCENE_HIT_F32

        rays = np.ascontiguousarray(rays, dtype=RAY_F32)
        n = rays.shape[0]
        words = self._ray_words(ray_masks, n)
        keep, pairs, stride = self._host_skip_pairs(skip_pairs, n)
        hits = None if occlusion else np.zeros((n,), dtype=SCENE_HIT_F32)
        mask = np.zeros((n,), dtype=np.uint8)
        q = capi.SceneQuery(ctypes.sizeof(capi.SceneQuery), self._scene_query_flags(ray_masks, skip_pairs, occlusion), rays.ctypes.data, n,
                            None if words is None else words.ctypes.data, pairs, stride, 0,
                            None if hits is None else hits.ctypes.data, mask.ctypes.data)
        self._check(self._L.nrtSceneQueryBatch_f32(self._h, ctypes.addressof(q)))
        del keep
        return mask if occlusion else (hits, mask)

    def QueryBatchDevice(self, d_rays, d_hits=None, d_mask=None, ray_masks=None, skip_pairs=None, occlusion=False):
        """nrtSceneQueryBatchDevice_f32: the same on HBM-resident torch tensors.  `ray_masks`: one 32-bit word per ray.  `skip_pairs`:
        a tensor of 32-bit words, two per ray (stride 8), or a uint8 tensor holding the previous wave's SCENE_HIT_F32 records, read
        where they lie (stride 20) — never the tensor this call writes.  With `occlusion` only `d_mask` is written.  Synchronous;
        waits for torch's current stream first."""
        import torch

        from .wire import RAY_F32, SCENE_HIT_F32

        n = d_rays.numel() // RAY_F32.itemsize
        assert d_rays.is_cuda and (d_hits is None or (d_hits.is_cuda and d_hits.numel() * d_hits.element_size() >= n * SCENE_HIT_F32.itemsize))
        assert d_mask is None or (d_mask.is_cuda and d_mask.numel() >= n)
        assert ray_masks is None or (ray_masks.is_cuda and ray_masks.numel() * ray_masks.element_size() >= 4 * n)
        pairs, stride = None, 0
        if skip_pairs is not None:
            assert skip_pairs.is_cuda
            if skip_pairs.element_size() == 1:  # records
                assert skip_pairs.numel() >= n * SCENE_HIT_F32.itemsize
                pairs, stride = skip_pairs.data_ptr() + SCENE_HIT_F32.fields["prim_id"][1], SCENE_HIT_F32.itemsize
            else:
                assert skip_pairs.element_size() == 4 and skip_pairs.numel() >= 2 * n, "two 32-bit words per ray"
                pairs, stride = skip_pairs.data_ptr(), 8
        torch.cuda.current_stream().synchronize()
        q = capi.SceneQuery(ctypes.sizeof(capi.SceneQuery), self._scene_query_flags(ray_masks, skip_pairs, occlusion), d_rays.data_ptr(), n,
                            None if ray_masks is None else ray_masks.data_ptr(), pairs, stride, 0,
                            None if d_hits is None else d_hits.data_ptr(), None if d_mask is None else d_mask.data_ptr())
        self._check(self._L.nrtSceneQueryBatchDevice_f32(self._h, ctypes.addressof(q)))
        return n

    # -- closest point (include/nanort_hip.h, "closest-point queries on scenes") ----
    def ClosestPointBatch(self, points, max_dist=np.inf, point_masks=None):
        """The nearest face of the nearest node to each point and where on it, in world space (nrtSceneClosestPointBatch_f32; the rule:
        include/nanort_closest.h).  `points`: [n, 3] coordinates with `max_dist` a scalar or one value per point, or a wire.POINT_F32
        record array (then `max_dist` is not read).  `point_masks`: one uint32 per point — a node is admitted iff its word
        (SetNodeMasks) shares a bit with the point's — or None: every node.  Returns (records, found): wire.SCENE_CLOSEST_F32 records and
        a uint8 per point."""
        from .wire import POINT_F32, SCENE_CLOSEST_F32

        if isinstance(points, np.ndarray) and points.dtype == POINT_F32:
            pts = np.ascontiguousarray(points).reshape(-1)
        else:
            xyz = np.asarray(points, dtype=np.float32).reshape(-1, 3)
            pts = np.zeros((xyz.shape[0],), dtype=POINT_F32)
            pts["p"] = xyz
            pts["max_dist"] = np.asarray(max_dist, dtype=np.float32)
        n = pts.shape[0]
        words = self._ray_words(point_masks, n)
        out = np.zeros((n,), dtype=SCENE_CLOSEST_F32)
        found = np.zeros((n,), dtype=np.uint8)
        self._check(self._L.nrtSceneClosestPointBatch_f32(self._h, _p(pts), n, _p(words), _p(out), _p(found)))
        return out, found

    def ClosestPointBatchDevice(self, d_points, d_out, d_found=None, d_point_masks=None):
        """The same on HBM-resident torch tensors of raw records (wire.POINT_F32 in, wire.SCENE_CLOSEST_F32 out, a byte per point in
        `d_found`, one 32-bit word per point in `d_point_masks`).  Synchronous (see nrtSceneClosestPointBatchDevice_f32); waits for
        torch's current stream first.  Returns the number of points."""
        import torch

        from .wire import POINT_F32, SCENE_CLOSEST_F32

        for t, what in ((d_points, "d_points"), (d_out, "d_out"), (d_found, "d_found"), (d_point_masks, "d_point_masks")):
            if t is not None and not t.is_cuda:
                raise ValueError("%s is not a device tensor" % what)
        n = d_points.numel() * d_points.element_size() // POINT_F32.itemsize
        if d_out.numel() * d_out.element_size() < n * SCENE_CLOSEST_F32.itemsize:
            raise ValueError("d_out holds fewer records than d_points holds points")
        if d_found is not None and d_found.numel() * d_found.element_size() < n:
            raise ValueError("d_found holds fewer bytes than d_points holds points")
        if d_point_masks is not None and d_point_masks.numel() * d_point_masks.element_size() < 4 * n:
            raise ValueError("d_point_masks holds fewer words than d_points holds points")
        torch.cuda.current_stream().synchronize()
        self._check(self._L.nrtSceneClosestPointBatchDevice_f32(self._h, d_points.data_ptr(), n, None if d_point_masks is None else d_point_masks.data_ptr(),
                                                                d_out.data_ptr(), None if d_found is None else d_found.data_ptr()))
        return n

"""ctypes view of the C ABI in include/nanort_hip.h (libnanort_hip.so).

Plumbing only: argument marshalling and a loud failure when the HIP library
is missing.  There is no CPU fallback of any kind behind these calls.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (NRT_USE_PROF_LIB=1: the profiling build of the same sources — include/nanort_hip_prof.h — for tools/ that read loop counters
# or per-wave time stamps; never set by the package, the tests or bench.py)
LIB_PATH = os.path.join(_HERE, "lib", "libnanort_hip_prof.so" if os.environ.get("NRT_USE_PROF_LIB") == "1" else "libnanort_hip.so")

NRT_OK, NRT_ERR_INVALID, NRT_ERR_EMPTY, NRT_ERR_DEVICE, NRT_ERR_PRECISION = 0, 1, 2, 3, 4

class NrtError(RuntimeError):
    def __init__(self, status, message):
        RuntimeError.__init__(self, "nanort_hip status %d: %s" % (status, message))
        self.status = status


class TraceCounters(ctypes.Structure):
    _fields_ = [
        ("nodes_visited", ctypes.c_uint64),
        ("leaves_tested", ctypes.c_uint64),
        ("tris_tested", ctypes.c_uint64),
        ("max_stack", ctypes.c_uint64),
    ]


NRT_QUERY_OCCLUSION, NRT_QUERY_MOTION, NRT_QUERY_MASKED = 1, 2, 4


class RayQuery(ctypes.Structure):
    """nrt_ray_query_f32 / nrt_ray_query_f64: the two differ in what their pointers point at, not in their layout."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("rays", ctypes.c_void_p),
        ("num_rays", ctypes.c_uint64),
        ("options", ctypes.c_void_p),
        ("skip_prim_ids", ctypes.c_void_p),
        ("times", ctypes.c_void_p),
        ("ray_masks", ctypes.c_void_p),
        ("hits_out", ctypes.c_void_p),
        ("mask_out", ctypes.c_void_p),
    ]


NRT_MAX_MULTIHIT = 64
NRT_MAX_NEAREST = 64


class MultiHitQuery(ctypes.Structure):
    """nrt_multihit_query_f32 / nrt_multihit_query_f64: RayQuery's first 56 bytes, then the rows, the counts and K."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("rays", ctypes.c_void_p),
        ("num_rays", ctypes.c_uint64),
        ("options", ctypes.c_void_p),
        ("skip_prim_ids", ctypes.c_void_p),
        ("times", ctypes.c_void_p),
        ("ray_masks", ctypes.c_void_p),
        ("hits_out", ctypes.c_void_p),
        ("counts_out", ctypes.c_void_p),
        ("max_hits", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


NRT_SCENE_QUERY_OCCLUSION, NRT_SCENE_QUERY_MASKED, NRT_SCENE_QUERY_SKIP = 1, 2, 4


class SceneQuery(ctypes.Structure):
    """nrt_scene_query_f32: one descriptor for the scene queries.  A skip pair is two uint32 {prim_id, node_id}, ray i's at
    skip_pairs + i * skip_stride_bytes."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("rays", ctypes.c_void_p),
        ("num_rays", ctypes.c_uint64),
        ("ray_masks", ctypes.c_void_p),
        ("skip_pairs", ctypes.c_void_p),
        ("skip_stride_bytes", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("hits_out", ctypes.c_void_p),
        ("mask_out", ctypes.c_void_p),
    ]


_LIB = None

vp, u32, u64, sz, i32, P = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER
_BOTH, _F32 = ("f32", "f64"), ("f32",)
_Q = [vp, vp, u64, vp]       # ctx, rays, num_rays, options: how every ray query starts
_QT = [vp, vp, vp, u64, vp]  # ... with the per-ray times of the motion queries (the per-ray words of the masked ones) behind the rays
_QB = [vp, u32, vp, vp, vp]  # ctx, num_batches, rays[], num_rays[], options: the multi-batch forms

# The binding of include/nanort_hip.h, one row per declaration in the header's order: (name, precision suffixes or None,
# argtypes, restype).  lib() applies it; SYMBOLS is derived from it (tests/test_capi.py checks SYMBOLS against the header and the
# built library, tests/test_capi_signatures.py the argument counts against the header).
SIGNATURES = [
    ("nrtCreate", None, [i32, P(vp)], i32),
    ("nrtDestroy", None, [vp], None),
    ("nrtLastError", None, [vp], ctypes.c_char_p),
    ("nrtVersion", None, [], ctypes.c_char_p),
    ("nrtHostAlloc", None, [sz, P(vp)], i32),
    ("nrtHostFree", None, [vp], None),
    ("nrtSetMesh", _BOTH, [vp, vp, sz, vp, u32], i32),
    ("nrtOccludedBatch", _BOTH, _Q + [vp], i32),
    ("nrtOccludedBatchDevice", _BOTH, _Q + [vp, vp], i32),
    ("nrtMultiHitTraverseBatch", _BOTH, [vp, vp, u64, u32, vp, vp, vp], i32),
    ("nrtMultiHitTraverseBatchDevice", _BOTH, [vp, vp, u64, u32, vp, vp, vp, vp], i32),
    ("nrtSetSpheres", _F32, [vp, vp, vp, u32], i32),
    ("nrtSetCylinders", _F32, [vp, vp, vp, u32, i32], i32),
    ("nrtTraverseBatchCylinders", _F32, _Q + [vp, vp], i32),
    ("nrtTraverseBatchCylindersDevice", _F32, _Q + [vp, vp, vp], i32),
    ("nrtSetCurves", _F32, [vp, vp, vp, u32, u32], i32),
    ("nrtSetCurvesDevice", _F32, [vp, vp, vp, u32, u32, vp], i32),
    ("nrtTraverseBatchCurves", _F32, _Q + [vp, vp], i32),
    ("nrtTraverseBatchCurvesDevice", _F32, _Q + [vp, vp, vp], i32),
    ("nrtOccludedBatchPrims", _F32, _Q + [vp], i32),
    ("nrtOccludedBatchPrimsDevice", _F32, _Q + [vp, vp], i32),
    ("nrtBuild", _BOTH, [vp, vp, vp, P(u64)], i32),
    ("nrtGetTree", _BOTH, [vp, vp, vp], i32),
    ("nrtTreeSize", None, [vp, P(u64), P(u64)], i32),
    ("nrtGetTreeBounds", _BOTH, [vp, vp, vp], i32),
    ("nrtSetTree", _BOTH, [vp, vp, u64, vp, u64], i32),
    ("nrtRefit", _BOTH, [vp, vp, sz], i32),
    ("nrtRefitDevice", _BOTH, [vp, vp, sz, vp], i32),
    ("nrtRefitPrims", _F32, [vp, vp, vp, u32], i32),
    ("nrtRefitPrimsDevice", _F32, [vp, vp, vp, u32, vp], i32),
    ("nrtSetMeshDevice", _BOTH, [vp, vp, u32, sz, vp, u32, vp], i32),
    ("nrtSetSpheresDevice", _F32, [vp, vp, vp, u32, vp], i32),
    ("nrtTraverseBatch", _BOTH, _Q + [vp, vp], i32),
    ("nrtTraverseBatchDevice", _BOTH, _Q + [vp, vp, vp], i32),
    ("nrtTraverseBatchesDevice", _BOTH, _QB + [vp, vp, vp, vp], i32),
    ("nrtTraverseBatches", _BOTH, _QB + [vp, vp, vp], i32),
    # per-ray skip ids: the rows above with the id array behind the options
    ("nrtTraverseBatchSkip", _BOTH, _Q + [vp, vp, vp], i32),
    ("nrtTraverseBatchSkipDevice", _BOTH, _Q + [vp, vp, vp, vp], i32),
    ("nrtOccludedBatchSkip", _BOTH, _Q + [vp, vp], i32),
    ("nrtOccludedBatchSkipDevice", _BOTH, _Q + [vp, vp, vp], i32),
    ("nrtTraverseBatchesSkipDevice", _BOTH, _QB + [vp, vp, vp, vp, vp], i32),
    ("nrtTraverseBatchesSkip", _BOTH, _QB + [vp, vp, vp, vp], i32),
    ("nrtSetMeshMotion", _BOTH, [vp, vp, sz], i32),
    ("nrtSetMeshMotionDevice", _BOTH, [vp, vp, u32, sz, vp], i32),
    ("nrtTraverseBatchMotion", _BOTH, _QT + [vp, vp], i32),
    ("nrtTraverseBatchMotionDevice", _BOTH, _QT + [vp, vp, vp], i32),
    ("nrtOccludedBatchMotion", _BOTH, _QT + [vp], i32),
    ("nrtOccludedBatchMotionDevice", _BOTH, _QT + [vp, vp], i32),
    # visibility masks: one word per face (no precision), and the motion rows' shape with the per-ray words where those have the times
    ("nrtSetPrimMasks", None, [vp, vp, u64], i32),
    ("nrtSetPrimMasksDevice", None, [vp, vp, u64, vp], i32),
    ("nrtTraverseBatchMasked", _BOTH, _QT + [vp, vp], i32),
    ("nrtTraverseBatchMaskedDevice", _BOTH, _QT + [vp, vp, vp], i32),
    ("nrtOccludedBatchMasked", _BOTH, _QT + [vp], i32),
    ("nrtOccludedBatchMaskedDevice", _BOTH, _QT + [vp, vp], i32),
    # one descriptor for every triangle ray query (RayQuery below): ctx, descriptor[, stream]
    ("nrtQueryBatch", _BOTH, [vp, vp], i32),
    ("nrtQueryBatchDevice", _BOTH, [vp, vp, vp], i32),
    # multi-hit under the same three per-ray inputs (MultiHitQuery above): ctx, descriptor[, stream]
    ("nrtMultiHitQueryBatch", _BOTH, [vp, vp], i32),
    ("nrtMultiHitQueryBatchDevice", _BOTH, [vp, vp, vp], i32),
    # closest-point queries: ctx, points, num_points, options, closest_out, found_out[, stream]
    ("nrtClosestPointBatch", _BOTH, _Q + [vp, vp], i32),
    ("nrtClosestPointBatchDevice", _BOTH, _Q + [vp, vp, vp], i32),
    # signed distance queries: the same arguments; the mesh's pseudonormals: ctx, face_normals_out, vertex_normals_out
    ("nrtSignedDistanceBatch", _BOTH, _Q + [vp, vp], i32),
    ("nrtSignedDistanceBatchDevice", _BOTH, _Q + [vp, vp, vp], i32),
    ("nrtGetFeatureNormals", _BOTH, [vp, vp, vp], i32),
    # nearest-faces queries: ctx, points, num_points, max_faces, options, nearest_out, counts_out[, stream]
    ("nrtNearestFacesBatch", _BOTH, [vp, vp, u64, u32, vp, vp, vp], i32),
    ("nrtNearestFacesBatchDevice", _BOTH, [vp, vp, u64, u32, vp, vp, vp, vp], i32),
    ("nrtTraverseBatchMulti", _BOTH, [vp, u32, vp, u64, u64, vp, vp, vp], i32),
    ("nrtDeviceCount", None, [], i32),
    ("nrtTraverseCountDevice", _BOTH, _Q + [P(TraceCounters)], i32),
    ("nrtLastTraverseMs", None, [vp], ctypes.c_float),
    ("nrtLastBuildMs", None, [vp], ctypes.c_float),
    ("nrtSetLaunchTiming", None, [vp, i32], i32),
    ("nrtSetTunable", None, [vp, ctypes.c_char_p, ctypes.c_longlong], i32),
    ("nrtGetTunable", None, [vp, ctypes.c_char_p, P(ctypes.c_longlong)], i32),
    ("nrtLastKernelName", None, [vp], ctypes.c_char_p),
    ("nrtSceneCreate", None, [i32, P(vp)], i32),
    ("nrtSceneDestroy", None, [vp], None),
    ("nrtSceneLastError", None, [vp], ctypes.c_char_p),
    ("nrtSceneAddNode", _F32, [vp, vp, vp, P(u32)], i32),
    ("nrtSceneCommit", None, [vp], i32),
    ("nrtSceneNodeState", _F32, [vp, u32, vp], i32),
    ("nrtSceneBounds", _F32, [vp, vp, vp], i32),
    ("nrtSceneTraverseBatch", _F32, [vp, vp, u64, vp, vp], i32),
    ("nrtSceneTraverseBatchDevice", _F32, [vp, vp, u64, vp, vp], i32),
    ("nrtSceneSetTunable", None, [vp, ctypes.c_char_p, i32], i32),
    ("nrtSceneLastRedone", None, [vp], u64),
    ("nrtSceneLastPath", None, [vp], i32),
    ("nrtSceneOccludedBatch", _F32, [vp, vp, u64, vp], i32),
    ("nrtSceneOccludedBatchDevice", _F32, [vp, vp, u64, vp], i32),
    # instance visibility masks: one word per node (no precision), and the four scene queries with the per-ray words behind the rays
    ("nrtSceneSetNodeMasks", None, [vp, vp, u32], i32),
    ("nrtSceneTraverseBatchMasked", _F32, [vp, vp, vp, u64, vp, vp], i32),
    ("nrtSceneTraverseBatchMaskedDevice", _F32, [vp, vp, vp, u64, vp, vp], i32),
    ("nrtSceneOccludedBatchMasked", _F32, [vp, vp, vp, u64, vp], i32),
    ("nrtSceneOccludedBatchMaskedDevice", _F32, [vp, vp, vp, u64, vp], i32),
    # one descriptor for the scene queries, with per-ray skip pairs (SceneQuery above): scene, descriptor
    ("nrtSceneQueryBatch", _F32, [vp, vp], i32),
    ("nrtSceneQueryBatchDevice", _F32, [vp, vp], i32),
    # closest-point queries on scenes: scene, points, num_points, point_masks, closest_out, found_out
    ("nrtSceneClosestPointBatch", _F32, [vp, vp, u64, vp, vp, vp], i32),
    ("nrtSceneClosestPointBatchDevice", _F32, [vp, vp, u64, vp, vp, vp], i32),
]
# Declared by the header, bound elsewhere: nanort_amd/dist.py sets the signatures of the nrtGroup* calls when a Group is made.
BOUND_ELSEWHERE = [
    "nrtGroupUniqueId", "nrtGroupCreate", "nrtGroupCreateRanked", "nrtGroupDestroy", "nrtGroupLastError", "nrtGroupSetTunable", "nrtGroupInfo",
    "nrtGroupTileRays", "nrtGroupTraverseGather_f32", "nrtGroupTraverseGather_f64", "nrtGroupTraverseGatherTiles_f32", "nrtGroupTraverseGatherTiles_f64",
    "nrtGroupSynchronize", "nrtGroupLastTraffic",
]


def _bound(row):
    """(symbol, argtypes, restype) of every precision of one SIGNATURES row."""
    name, suffixes, argtypes, restype = row
    return [(name if s is None else name + "_" + s, argtypes, restype) for s in (suffixes or (None,))]


# Every symbol include/nanort_hip.h declares.
SYMBOLS = [symbol for row in SIGNATURES for symbol, _, _ in _bound(row)] + BOUND_ELSEWHERE


def lib():
    """Load libnanort_hip.so (once). Raises if it was not built — never falls back."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "%s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C nanort_amd/csrc`. nanort_amd has no CPU fallback." % LIB_PATH
        )
    try:
        # When torch is in the process its bundled HIP runtime (same SONAME,
        # libamdhip64.so.7) must be the one we bind to, so device pointers and
        # streams are shared.  Importing it first makes the loader reuse it.
        import torch  # noqa: F401
    except Exception:
        pass
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for row in SIGNATURES:
        for symbol, argtypes, restype in _bound(row):
            f = getattr(L, symbol)
            f.argtypes, f.restype = argtypes, restype
    _LIB = L
    return L

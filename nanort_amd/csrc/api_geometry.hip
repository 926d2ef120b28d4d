// nanort_amd/csrc/api_geometry.hip — the setters behind the C ABI (include/nanort_hip.h): the four primitive kinds from host
// memory or from HBM, the motion keyframe of a triangle mesh, and its visibility masks.
#include "ctx.h"

// ---------------------------------------------------------------------------
// primitives: one path for the setters of every kind (prim_kinds.h), from host memory or (the *Device forms: copied on the
// caller's stream) from HBM.  Every refusal comes before anything changes; the counts are set once the primitives are in place,
// so a failed upload leaves an empty context.
// ---------------------------------------------------------------------------
// The first refusal of every setter.
static nrt_status refuse_precision(nrt_ctx *c, const char *fn, int kind, int prec) {
  if (!c) return NRT_ERR_INVALID;
  if (c->prec == 0 || c->prec == prec) return NRT_OK;
  return fail(c, NRT_ERR_PRECISION, kind == kPrimTriangles ? "%s: context already holds a %s mesh" : "%s: context already holds %s primitives", fn,
              c->prec == 4 ? "f32" : "f64");
}

// Nothing is refused any more: the old tree and primitives go, the context is of this kind and precision.
static void drop_primitives(nrt_ctx *c, int kind, int prec) {
  free_tree(c);
  free_mesh(c);
  c->prec = prec;
  c->prim_kind = kind;
}
static nrt_status begin_set(nrt_ctx *c, int kind, int prec) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, wait_for_launches(c));
  drop_primitives(c, kind, prec);
  return NRT_OK;
}

// What remains of a Device set call once the old primitives are gone and a HIP call fails: an empty context and the reason.
static nrt_status set_device_failed(nrt_ctx *c, const char *fn, hipStream_t s, hipError_t e) {
  (void)hipStreamSynchronize(s);
  free_mesh(c);
  return fail(c, NRT_ERR_DEVICE, "%s: %s (the context's primitives were dropped: set them again)", fn, hipGetErrorString(e));
}

// `src` (null: nothing to copy yet) into the grow-only buffer `b`: from the host, or (`device`) from HBM on `s`.
static nrt_status upload(nrt_ctx *c, const char *fn, DevBuf &b, const void *src, size_t bytes, bool device, hipStream_t s) {
  if (!device) {
    if (nrt_status st = ensure(c, b, bytes)) return st;
    if (src) HIPCHK(c, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return NRT_OK;
  }
  hipError_t e = devbuf_ensure(&b, bytes);
  if (e == hipSuccess && src) e = hipMemcpyAsync(b.p, src, bytes, hipMemcpyDeviceToDevice, s);
  return e == hipSuccess ? NRT_OK : set_device_failed(c, fn, s, e);
}
// The tail of every setter: a Device form waits for its copies (the context owns its copy: the caller's buffers are free again),
// and the primitives are in place.
static nrt_status adopt_primitives(nrt_ctx *c, const char *fn, bool device, hipStream_t s, bool faces, bool radii, uint32_t n, uint32_t num_verts) {
  if (device) {
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return set_device_failed(c, fn, s, e);
  }
  c->d_verts = c->b_verts.p;
  c->d_faces = faces ? (uint32_t *)c->b_faces.p : nullptr;
  c->d_radii = radii ? c->b_radii.p : nullptr;
  c->num_faces = n;
  c->num_verts = num_verts;
  return NRT_OK;
}

template <typename T>
static nrt_status set_mesh(nrt_ctx *c, const T *vertices, size_t stride, const uint32_t *faces,
                           uint32_t num_faces) {
  const char *fn = "nrtSetMesh";
  if (nrt_status st = refuse_precision(c, fn, kPrimTriangles, (int)sizeof(T))) return st;
  if (num_faces && (!vertices || !faces)) return fail(c, NRT_ERR_INVALID, "nrtSetMesh: NULL mesh pointer");
  if (stride < 3 * sizeof(T) && num_faces)
    return fail(c, NRT_ERR_INVALID, "nrtSetMesh: vertex stride %zu < %zu", stride, 3 * sizeof(T));
  NRT_RANGE("nrtSetMesh (compaction + upload)");
  if (nrt_status st = begin_set(c, kPrimTriangles, (int)sizeof(T))) return st;
  if (num_faces == 0) return NRT_OK;
  // The reference's mesh carries no vertex count (nanort.h:925-930): derive it.
  uint32_t maxv = 0;
  const size_t ni = 3 * (size_t)num_faces;
  for (size_t i = 0; i < ni; i++) maxv = faces[i] > maxv ? faces[i] : maxv;
  const uint32_t nv = maxv + 1;
  // Compact the strided vertex array (get_vertex_addr, nanort.h:467-472) to tight xyz.
  const T *src = vertices;
  std::vector<T> tight;
  if (stride != 3 * sizeof(T)) {
    tight.resize(3 * (size_t)nv);
    const unsigned char *base = reinterpret_cast<const unsigned char *>(vertices);
    for (uint32_t v = 0; v < nv; v++) {
      const T *p = reinterpret_cast<const T *>(base + (size_t)v * stride);
      tight[3 * (size_t)v + 0] = p[0];
      tight[3 * (size_t)v + 1] = p[1];
      tight[3 * (size_t)v + 2] = p[2];
    }
    src = tight.data();
  }
  nrt_status st;
  if ((st = upload(c, fn, c->b_verts, src, 3 * (size_t)nv * sizeof(T), false, nullptr)) || (st = upload(c, fn, c->b_faces, faces, ni * sizeof(uint32_t), false, nullptr)))
    return st;
  return adopt_primitives(c, fn, false, nullptr, true, false, num_faces, nv);
}

// nrtSetMesh for arrays in HBM: the same state as set_mesh leaves, the vertex count derived and the caller's `num_vertices`
// checked on the device before any vertex is read and before anything of the context is dropped.
template <typename T>
static nrt_status set_mesh_device(nrt_ctx *c, const T *vertices, uint32_t num_vertices, size_t stride, const uint32_t *faces,
                                  uint32_t num_faces, hipStream_t s) {
  const char *fn = "nrtSetMeshDevice";
  if (nrt_status st = refuse_precision(c, fn, kPrimTriangles, (int)sizeof(T))) return st;
  if (num_faces) {
    if (!vertices || !faces) return fail(c, NRT_ERR_INVALID, "%s: NULL mesh pointer", fn);
    if (num_vertices == 0) return fail(c, NRT_ERR_INVALID, "%s: num_vertices == 0 with %u faces", fn, num_faces);
    if (stride < 3 * sizeof(T)) return fail(c, NRT_ERR_INVALID, "%s: vertex stride %zu < %zu", fn, stride, 3 * sizeof(T));
    if (stride % sizeof(T) != 0 || (uintptr_t)vertices % sizeof(T) != 0)
      return fail(c, NRT_ERR_INVALID, "%s: vertex stride %zu or pointer not aligned to %zu bytes", fn, stride, sizeof(T));
    if ((uintptr_t)faces % sizeof(uint32_t) != 0) return fail(c, NRT_ERR_INVALID, "%s: face pointer not aligned to 4 bytes", fn);
  }
  NRT_RANGE("nrtSetMeshDevice");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, wait_for_launches(c));
  uint32_t nv = 0;
  const size_t ni = 3 * (size_t)num_faces;
  if (num_faces) { // the guard: nothing of the context has changed yet
    if (!c->h_max_index) HIPCHK(c, hipHostMalloc((void **)&c->h_max_index, sizeof(uint32_t), hipHostMallocDefault));
    nrt_status st;
    if ((st = ensure(c, c->b_max_index, sizeof(uint32_t)))) return st;
    HIPCHK(c, launch_max_index(faces, ni, (uint32_t *)c->b_max_index.p, s));
    HIPCHK(c, hipMemcpyAsync(c->h_max_index, c->b_max_index.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const uint32_t maxv = *c->h_max_index;
    if (maxv >= num_vertices)
      return fail(c, NRT_ERR_INVALID, "%s: face index %u is out of range: the vertex block holds %u rows", fn, maxv, num_vertices);
    nv = maxv + 1;
  }
  drop_primitives(c, kPrimTriangles, (int)sizeof(T));
  if (num_faces == 0) return NRT_OK;
  const bool tight = stride == 3 * sizeof(T); // (tight already: a copy; else the gather kernel)
  nrt_status st;
  if ((st = upload(c, fn, c->b_verts, tight ? vertices : nullptr, 3 * (size_t)nv * sizeof(T), true, s))) return st;
  if (!tight) {
    const hipError_t e = launch_gather_vertices<T>(vertices, stride, nv, (T *)c->b_verts.p, s);
    if (e != hipSuccess) return set_device_failed(c, fn, s, e);
  }
  if ((st = upload(c, fn, c->b_faces, faces, ni * sizeof(uint32_t), true, s))) return st;
  return adopt_primitives(c, fn, true, s, true, false, num_faces, nv);
}

// The kinds with radii — spheres (SphereGeometry of examples/particle_primitive/main.cc:113-147), cylinders (CylinderGeometry of
// examples/cylinder_primitive/main.cc:124-210), curves (CurveGeometry of examples/curves_primitive/main.cc:513-604) — as their
// row of kPrimKinds describes them: `n` times pos_floats positions and radius_floats radii of `prec` bytes each.
// `extra_refusal`: the caller's own refusal (null: none), in its place among the shared ones.
static nrt_status set_radius_prims(nrt_ctx *c, const char *fn, int kind, int prec, const void *positions, const void *radii, uint32_t n, bool device,
                                   hipStream_t s, const char *extra_refusal = nullptr) {
  const PrimKind &k = kPrimKinds[kind];
  if (nrt_status st = refuse_precision(c, fn, kind, prec)) return st;
  if (extra_refusal) return fail(c, NRT_ERR_INVALID, "%s: %s", fn, extra_refusal);
  if (n && (!positions || !radii)) return fail(c, NRT_ERR_INVALID, "%s: NULL pointer", fn);
  if (k.max_count && n >= k.max_count) return fail(c, NRT_ERR_INVALID, "%s: too many %s", fn, k.name);
  if (device && n && ((uintptr_t)positions % (size_t)prec != 0 || (uintptr_t)radii % (size_t)prec != 0))
    return fail(c, NRT_ERR_INVALID, "%s: pointer not aligned to %d bytes", fn, prec);
  if (nrt_status st = begin_set(c, kind, prec)) return st;
  if (n == 0) return NRT_OK;
  nrt_status st;
  if ((st = upload(c, fn, c->b_verts, positions, (size_t)k.pos_floats * n * (size_t)prec, device, s)) ||
      (st = upload(c, fn, c->b_radii, radii, (size_t)k.radius_floats * n * (size_t)prec, device, s)))
    return st;
  return adopt_primitives(c, fn, device, s, false, true, n, (uint32_t)k.num_verts * n);
}

// Segments for the builder (prims.hip, k_cylinder_segments): a cylinder many radii long is handed over as several pieces
// with their own tight boxes and the cylinder's id.  Counts on the host (the arrays are here anyway), pieces on the device.
static nrt_status segment_cylinders(nrt_ctx *c, const float *endpoints, const float *radii, uint32_t n) {
  c->num_segs = 0;
  c->segment_ms = 0.f;
  // (zero-radius "cylinders" are boxes — the top-level tree of a scene is built over them — and cyl_split = 1 asks for the
  // example's own boxes: neither needs the counting pass or its array)
  bool any_radius = false;
  for (size_t i = 0; i < 2 * (size_t)n && !any_radius; i++) any_radius = radii[i] > 0.0f;
  if (c->cyl_split <= 1 || !any_radius) return NRT_OK;
  const auto seg_t0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> off((size_t)n + 1);
  const uint64_t total = cylinder_segment_offsets(endpoints, radii, n, c->cyl_seg_radii, (uint32_t)c->cyl_split, kPackedFirstMask, off.data());
  if (total > (uint64_t)n) {
    nrt_status st;
    if ((st = ensure(c, c->b_seg_off, ((size_t)n + 1) * sizeof(uint32_t))) || (st = ensure(c, c->b_seg_verts, 6 * (size_t)total * sizeof(float))) ||
        (st = ensure(c, c->b_seg_radii, 2 * (size_t)total * sizeof(float))) || (st = ensure(c, c->b_seg_prim, (size_t)total * sizeof(uint32_t))))
      return st;
    HIPCHK(c, hipMemcpyAsync(c->b_seg_off.p, off.data(), ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_cylinder_segments((const float *)c->d_verts, (const float *)c->d_radii, (const uint32_t *)c->b_seg_off.p, n,
                                       (float *)c->b_seg_verts.p, (float *)c->b_seg_radii.p, (uint32_t *)c->b_seg_prim.p, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (`off` is pageable host memory)
    c->num_segs = (uint32_t)total;
  }
  // the segmentation is part of building this tree: its wall time is added to the build's (nrtLastBuildMs, build_secs)
  c->segment_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - seg_t0).count();
  return NRT_OK;
}

static nrt_status set_cylinders(nrt_ctx *c, const float *endpoints, const float *radii, uint32_t n, int test_cap) {
  if (nrt_status st = set_radius_prims(c, "nrtSetCylinders", kPrimCylinders, 4, endpoints, radii, n, false, nullptr)) return st;
  c->cyl_test_cap = test_cap ? 1u : 0u;
  return n ? segment_cylinders(c, endpoints, radii, n) : NRT_OK;
}

static nrt_status set_curves(nrt_ctx *c, const float *cps, const float *radii, uint32_t n, uint32_t subdiv, bool device, hipStream_t s) {
  char refusal[64] = "";
  if (subdiv < 1u || subdiv > 64u) snprintf(refusal, sizeof(refusal), "num_subdivisions %u outside 1..64", subdiv);
  if (nrt_status st = set_radius_prims(c, device ? "nrtSetCurvesDevice" : "nrtSetCurves", kPrimCurves, 4, cps, radii, n, device, s, refusal[0] ? refusal : nullptr))
    return st;
  c->curve_subdiv = subdiv;
  return NRT_OK;
}

// ---------------------------------------------------------------------------
// motion blur (include/nanort_hip.h, nrtSetMeshMotion*; the queries nrt*BatchMotion*: api_query.hip)
// ---------------------------------------------------------------------------
// The second vertex keyframe of the context's triangle mesh, from host memory or (`device`: read on `s`) from HBM, into the context's
// own tight array through launch_gather_vertices.  Every refusal comes before anything changes or is enqueued; then the tree goes
// (its boxes and leaf records belong to the keyframes it was built over) and the call returns when the context owns its copy.
// `vertices` == NULL removes the keyframe.
template <typename T>
static nrt_status set_mesh_motion(nrt_ctx *c, const T *vertices, uint32_t num_vertices, size_t stride, bool device, hipStream_t s) {
  const char *fn = device ? "nrtSetMeshMotionDevice" : "nrtSetMeshMotion";
  if (!c) return NRT_ERR_INVALID;
  if (c->prec != 0 && c->prec != (int)sizeof(T))
    return fail(c, NRT_ERR_PRECISION, "%s: the context holds %s primitives", fn, c->prec == 8 ? "f64" : "f32");
  if (c->prec == 0 || c->prim_kind != kPrimTriangles || !c->d_verts || c->num_faces == 0)
    return fail(c, NRT_ERR_INVALID, "%s: set a triangle mesh first (nrtSetMesh): the keyframe shares its faces and its vertex count", fn);
  if (vertices) {
    if (stride < 3 * sizeof(T)) return fail(c, NRT_ERR_INVALID, "%s: vertex stride %zu < %zu", fn, stride, 3 * sizeof(T));
    if (device && (stride % sizeof(T) != 0 || (uintptr_t)vertices % sizeof(T) != 0))
      return fail(c, NRT_ERR_INVALID, "%s: vertex stride %zu or pointer not aligned to %zu bytes", fn, stride, sizeof(T));
    // (the faces were validated against num_verts when the mesh was set: a block of that many rows is all the gather reads — what
    // DESIGN 3.7 asks of nrtSetMeshDevice, without an index reduction)
    if (device && num_vertices < c->num_verts)
      return fail(c, NRT_ERR_INVALID, "%s: the vertex block holds %u rows, the context's mesh has %u vertices", fn, num_vertices, c->num_verts);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, wait_for_launches(c));
  free_tree(c); // (bumps generation)
  c->d_verts1 = nullptr;
  if (!vertices) return NRT_OK;
  const uint32_t nv = c->num_verts;
  if (nrt_status st = ensure(c, c->b_verts1, 3 * (size_t)nv * sizeof(T))) return st;
  if (!device) s = c->stream;
  const void *src = vertices;
  if (!device) { // the caller's block, as it lies, into the staging buffer the host refit uses
    const size_t block = (size_t)(nv - 1) * stride + 3 * sizeof(T);
    if (nrt_status st = ensure(c, c->b_refit_stage, block)) return st;
    HIPCHK(c, hipMemcpyAsync(c->b_refit_stage.p, vertices, block, hipMemcpyHostToDevice, s));
    src = c->b_refit_stage.p;
  }
  HIPCHK(c, launch_gather_vertices<T>(src, stride, nv, (T *)c->b_verts1.p, s));
  HIPCHK(c, hipStreamSynchronize(s)); // the context owns its copy: the caller's buffer is free again
  c->d_verts1 = c->b_verts1.p;
  return NRT_OK;
}

// ---------------------------------------------------------------------------
// visibility masks (include/nanort_hip.h, nrtSetPrimMasks*; the queries nrt*BatchMasked*: api_query.hip)
// ---------------------------------------------------------------------------
// One 32-bit word per face of the context's triangle mesh, in face order, from host memory or (`device`: copied on `s`) from HBM.
// Every refusal comes before anything changes; the tree stays as it is — the words are no part of it — and the leaf-order copy the
// walk reads is derived by the next masked query (leaf_masks_stale).  `masks` == NULL removes the masks.
static nrt_status set_prim_masks(nrt_ctx *c, const uint32_t *masks, uint64_t count, bool device, hipStream_t s) {
  const char *fn = device ? "nrtSetPrimMasksDevice" : "nrtSetPrimMasks";
  if (!c) return NRT_ERR_INVALID;
  if (c->prec != 0 && c->prim_kind != kPrimTriangles)
    return fail(c, NRT_ERR_INVALID, "%s: visibility masks: triangle contexts only (this context holds %s)", fn, kPrimKinds[c->prim_kind].name);
  if (c->prec == 0 || !c->d_verts || c->num_faces == 0)
    return fail(c, NRT_ERR_INVALID, "%s: set a triangle mesh first (nrtSetMesh): the masks are one word per face of it", fn);
  if (masks && count != (uint64_t)c->num_faces)
    return fail(c, NRT_ERR_INVALID, "%s: count %llu differs from the mesh's %u faces", fn, (unsigned long long)count, c->num_faces);
  if (device && ((uintptr_t)masks & 3u) != 0u) return fail(c, NRT_ERR_INVALID, "%s: the device array is not 4-byte aligned", fn);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, wait_for_launches(c)); // (masked launches in flight read the leaf-order words the next masked query rewrites)
  c->d_prim_masks = nullptr;
  c->leaf_masks_stale = true;
  if (!masks) return NRT_OK;
  const size_t bytes = (size_t)count * sizeof(uint32_t);
  if (nrt_status st = ensure(c, c->b_prim_masks, bytes)) return st;
  if (device) {
    HIPCHK(c, hipMemcpyAsync(c->b_prim_masks.p, masks, bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s)); // the context owns its copy: the caller's buffer is free again
  } else {
    HIPCHK(c, hipMemcpy(c->b_prim_masks.p, masks, bytes, hipMemcpyHostToDevice));
  }
  c->d_prim_masks = (uint32_t *)c->b_prim_masks.p;
  return NRT_OK;
}

extern "C" {

nrt_status nrtSetMesh_f32(nrt_ctx *c, const float *v, size_t stride, const uint32_t *f, uint32_t nf) {
  return set_mesh<float>(c, v, stride, f, nf);
}
nrt_status nrtSetMesh_f64(nrt_ctx *c, const double *v, size_t stride, const uint32_t *f, uint32_t nf) {
  return set_mesh<double>(c, v, stride, f, nf);
}

nrt_status nrtSetSpheres_f32(nrt_ctx *c, const float *centers, const float *radii, uint32_t n) {
  return set_radius_prims(c, "nrtSetSpheres", kPrimSpheres, 4, centers, radii, n, false, nullptr);
}

nrt_status nrtSetCylinders_f32(nrt_ctx *c, const float *endpoints, const float *radii, uint32_t n, int test_cap) {
  return set_cylinders(c, endpoints, radii, n, test_cap);
}

nrt_status nrtSetCurves_f32(nrt_ctx *c, const float *cps, const float *radii, uint32_t n, uint32_t subdiv) {
  return set_curves(c, cps, radii, n, subdiv, false, nullptr);
}
nrt_status nrtSetCurvesDevice_f32(nrt_ctx *c, const float *cps, const float *radii, uint32_t n, uint32_t subdiv, void *s) {
  return set_curves(c, cps, radii, n, subdiv, true, (hipStream_t)s);
}

nrt_status nrtSetMeshDevice_f32(nrt_ctx *c, const float *v, uint32_t nv, size_t stride, const uint32_t *f, uint32_t nf, void *s) {
  return set_mesh_device<float>(c, v, nv, stride, f, nf, (hipStream_t)s);
}
nrt_status nrtSetMeshDevice_f64(nrt_ctx *c, const double *v, uint32_t nv, size_t stride, const uint32_t *f, uint32_t nf, void *s) {
  return set_mesh_device<double>(c, v, nv, stride, f, nf, (hipStream_t)s);
}
nrt_status nrtSetSpheresDevice_f32(nrt_ctx *c, const float *centers, const float *radii, uint32_t n, void *s) {
  return set_radius_prims(c, "nrtSetSpheresDevice", kPrimSpheres, 4, centers, radii, n, true, (hipStream_t)s);
}

nrt_status nrtSetMeshMotion_f32(nrt_ctx *c, const float *v, size_t stride) { return set_mesh_motion<float>(c, v, 0, stride, false, nullptr); }
nrt_status nrtSetMeshMotion_f64(nrt_ctx *c, const double *v, size_t stride) { return set_mesh_motion<double>(c, v, 0, stride, false, nullptr); }
nrt_status nrtSetMeshMotionDevice_f32(nrt_ctx *c, const float *v, uint32_t nv, size_t stride, void *s) {
  return set_mesh_motion<float>(c, v, nv, stride, true, (hipStream_t)s);
}
nrt_status nrtSetMeshMotionDevice_f64(nrt_ctx *c, const double *v, uint32_t nv, size_t stride, void *s) {
  return set_mesh_motion<double>(c, v, nv, stride, true, (hipStream_t)s);
}

nrt_status nrtSetPrimMasks(nrt_ctx *c, const uint32_t *masks, uint64_t count) { return set_prim_masks(c, masks, count, false, nullptr); }
nrt_status nrtSetPrimMasksDevice(nrt_ctx *c, const uint32_t *masks, uint64_t count, void *s) {
  return set_prim_masks(c, masks, count, true, (hipStream_t)s);
}

} // extern "C"

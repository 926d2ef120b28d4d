// nanort_amd/csrc/prims.hip — everything the library does per primitive KIND (prim_kinds.h) outside the walk: the kernels
// that bring primitives in, lay them out for the walk and finish its records.  The kinds' intersectors are the walk's
// (traverse_dev.h), their box-and-centre rules the builder's (build.hip, k_prim_records).
//
//   k_max_index, k_gather_vertices   geometry that is already in HBM (nrtSetMeshDevice*, include/nanort_hip.h): what nrtSetMesh
//                                    does on the host, on the device.  The mesh's vertex count is the largest face index + 1, and
//                                    the caller's num_vertices is checked against it before any vertex is read; strided rows ->
//                                    the context's tight xyz (also the vertex pass of a refit, refit.hip).  max over u32 is exact
//                                    and order-free: the word never depends on scheduling.
//   k_permute_masks                  the triangles' visibility words (nrtSetPrimMasks*) in leaf order, for the masked walks
//   k_cylinder_segments              long cylinders cut into segments for the builder (nrtSetCylinders)
//   k_gather_leaf_*                  leaf-ordered primitive records from the index array of a tree (launch_gather_leaf)
//   k_sphere_uv, k_cylinder_post,    the pass behind a walk over spheres, cylinders, curves (launch_post_pass): it finishes the
//   k_curve_post                     hit records and closes the launch's completion record in the walk's place
#include <algorithm>

#include "kernels.h"
#include "traverse_dev.h" // cyl_normalize, cyl_dot, done_end_blocks

namespace nrt {

// ---- geometry taken from device memory ------------------------------------------------------------------------------------
constexpr unsigned kMeshBlock = 256;
constexpr unsigned kMeshMaxGrid = 2048; // 256 CUs x 8 blocks: the rest of the array by grid stride

// The array as a scalar head (up to the first 16-byte boundary), a middle of `n_vec` 128-bit loads and a scalar tail (both
// under four words): `faces` is only 4-byte aligned when it is a view into a larger allocation.
__global__ void __launch_bounds__(kMeshBlock) k_max_index(const uint32_t *__restrict__ faces, uint32_t head, uint64_t n_vec, uint32_t tail,
                                                          uint32_t *__restrict__ out) {
  const uint64_t gid = (uint64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  const uint4 *mid = reinterpret_cast<const uint4 *>(faces + head);
  uint32_t m = 0;
  for (uint64_t i = gid; i < n_vec; i += (uint64_t)gridDim.x * kMeshBlock) {
    const uint4 v = mid[i];
    m = max(max(m, max(v.x, v.y)), max(v.z, v.w));
  }
  if (gid < head) m = max(m, faces[gid]);
  if (gid < tail) m = max(m, faces[head + 4 * n_vec + gid]);
  // the wave's maximum by cross-lane exchange, the block's through LDS, then one atomic per block
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
  __shared__ uint32_t wave_max[kMeshBlock / 64];
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (unsigned w = 1; w < kMeshBlock / 64; w++) m = max(m, wave_max[w]);
    if (m) atomicMax(out, m); // (`out` starts at 0)
  }
}

hipError_t launch_max_index(const uint32_t *faces, uint64_t n_indices, uint32_t *out, hipStream_t s) {
  hipError_t e = hipMemsetAsync(out, 0, sizeof(uint32_t), s);
  if (e != hipSuccess || n_indices == 0) return e;
  const uint64_t to_boundary = ((16u - (uint32_t)((uintptr_t)faces & 15u)) & 15u) / 4u;
  const uint32_t head = (uint32_t)std::min<uint64_t>(to_boundary, n_indices);
  const uint64_t n_vec = (n_indices - head) / 4;
  const uint32_t tail = (uint32_t)(n_indices - head - 4 * n_vec);
  const uint64_t blocks = (n_vec + kMeshBlock - 1) / kMeshBlock;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, kMeshMaxGrid));
  hipLaunchKernelGGL(k_max_index, dim3(grid), dim3(kMeshBlock), 0, s, faces, head, n_vec, tail, out);
  return hipGetLastError();
}

// Aligned: the row stride and the base are multiples of sizeof(T) (typed loads); else byte loads.
template <typename T, bool Aligned>
__global__ void __launch_bounds__(kMeshBlock) k_gather_vertices(const unsigned char *__restrict__ src, size_t stride, uint32_t nv,
                                                                T *__restrict__ dst) {
  const uint32_t i = blockIdx.x * kMeshBlock + threadIdx.x;
  if (i >= nv) return;
  const unsigned char *row = src + (size_t)i * stride;
  T p[3];
  if (Aligned) {
    const T *r = reinterpret_cast<const T *>(row);
    p[0] = r[0];
    p[1] = r[1];
    p[2] = r[2];
  } else {
    __builtin_memcpy(p, row, sizeof(p));
  }
  dst[3 * (size_t)i + 0] = p[0];
  dst[3 * (size_t)i + 1] = p[1];
  dst[3 * (size_t)i + 2] = p[2];
}

// `nv` rows of `src`, row i at byte offset i * stride with xyz first, to tight xyz.  `src` is device memory.
template <typename T>
hipError_t launch_gather_vertices(const void *src, size_t stride, uint32_t nv, T *tight, hipStream_t s) {
  if (nv == 0) return hipSuccess;
  const bool aligned = stride % sizeof(T) == 0 && (uintptr_t)src % sizeof(T) == 0;
  const dim3 grid((nv + kMeshBlock - 1) / kMeshBlock);
  if (aligned)
    hipLaunchKernelGGL((k_gather_vertices<T, true>), grid, dim3(kMeshBlock), 0, s, (const unsigned char *)src, stride, nv, tight);
  else
    hipLaunchKernelGGL((k_gather_vertices<T, false>), grid, dim3(kMeshBlock), 0, s, (const unsigned char *)src, stride, nv, tight);
  return hipGetLastError();
}

// leaf_masks[k] = masks[tris[k].prim_id]: one thread per leaf record, the grid covers them all.  (tris[k].prim_id < num_faces by
// construction: the builder emits a permutation of the face ids, nrtSetTree checks every index; read with a guard all the same.)
// Derived whenever either side of that permutation changed (api_query.hip, refresh_leaf_masks).
template <typename T>
__global__ __launch_bounds__(256) void k_permute_masks(const LeafTri<T> *__restrict__ tris, const uint32_t *__restrict__ masks, uint32_t num_faces,
                                                       uint32_t *__restrict__ leaf_masks, uint32_t n) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint32_t p = tris[k].prim_id;
  leaf_masks[k] = p < num_faces ? masks[p] : 0u;
}

template <typename T>
hipError_t launch_permute_masks(const void *tris, const uint32_t *masks, uint32_t num_faces, uint32_t *leaf_masks, uint32_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_permute_masks<T>), dim3((n + 255u) / 256u), dim3(256), 0, s, (const LeafTri<T> *)tris, masks, num_faces, leaf_masks, n);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Long cylinders, cut into SEGMENTS for the builder (round 5).  The cylinder example's scene is box-spanning needles (random
// end points in the scene box, examples/cylinder_primitive/main.cc:428-462): a tree over their whole boxes prunes nothing —
// every box covers a fair part of the scene (4 200 L1 look-ups per ray, 44 Mrays/s in round 4).  So the builder is handed
// one primitive per SEGMENT of a cylinder's axis, each with the tight box of its piece of the tube — the box of the two
// end points of the piece, each grown by the radius the intersector uses for the whole tube, max(r0, r1)
// (main.cc:256), plus a few ulps for the rounding of the interior end points — and the CYLINDER's id: the index array then
// names a cylinder once per segment, a leaf tests the whole cylinder (CylinderIntersector::Intersect is a pure function of
// (ray, cylinder, current t): testing a cylinder twice returns the same record or rejects it), and the closest hit of a
// cylinder lies in the box of the segment it falls on.  The segment count is fixed on the host (nrtSetCylinders: length over
// `cyl_seg_radii` tube radii, at most `cyl_split`); a cylinder of one segment keeps the reference's own box
// (CylinderGeometry::BoundingBox, main.cc:132-165: p0 -/+ r0, p1 -/+ r1).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cylinder_segments(const float *__restrict__ verts, const float *__restrict__ radii,
                                                           const uint32_t *__restrict__ seg_off, uint32_t n,
                                                           float *__restrict__ seg_verts, float *__restrict__ seg_radii,
                                                           uint32_t *__restrict__ seg_prim) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t first = seg_off[i], K = seg_off[i + 1] - first;
  float p0[3], p1[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    p0[k] = verts[6 * (size_t)i + k];
    p1[k] = verts[6 * (size_t)i + 3 + k];
  }
  const float r0 = radii[2 * (size_t)i], r1 = radii[2 * (size_t)i + 1];
  if (K <= 1u) { // unsplit: the reference's own box
#pragma unroll
    for (int k = 0; k < 3; k++) {
      seg_verts[6 * (size_t)first + k] = p0[k];
      seg_verts[6 * (size_t)first + 3 + k] = p1[k];
    }
    seg_radii[2 * (size_t)first] = r0;
    seg_radii[2 * (size_t)first + 1] = r1;
    seg_prim[first] = i;
    return;
  }
  const float rr = r0 > r1 ? r0 : r1; // std::max<float>(r0, r1), main.cc:256
  const float invK = 1.0f / (float)K;
  float a[3] = {p0[0], p0[1], p0[2]};
  // The interior end points p0 + (p1 - p0) * s are rounded: p1 - p0 alone carries an error of the order of an ulp of the
  // CYLINDER's end points, whatever the size of the interior point itself (a long cylinder spanning the origin has interior
  // points near 0 whose error is that of its far ends).  So the slack the radius carries is sized once, from the end points.
  const float mag = fmaxf(fmaxf(fabsf(p0[0]), fabsf(p0[1])), fabsf(p0[2])) + fmaxf(fmaxf(fabsf(p1[0]), fabsf(p1[1])), fabsf(p1[2])) + rr;
  const float rs = rr + 1.0e-6f * mag;
  for (uint32_t j = 0; j < K; j++) {
    float b[3];
#pragma unroll
    for (int k = 0; k < 3; k++) b[k] = (j + 1u == K) ? p1[k] : p0[k] + (p1[k] - p0[k]) * ((float)(j + 1u) * invK);
    const size_t o = (size_t)first + j;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      seg_verts[6 * o + k] = a[k];
      seg_verts[6 * o + 3 + k] = b[k];
      a[k] = b[k];
    }
    seg_radii[2 * o] = rs;
    seg_radii[2 * o + 1] = rs;
    seg_prim[o] = i;
  }
}

hipError_t launch_cylinder_segments(const float *verts, const float *radii, const uint32_t *seg_off, uint32_t n, float *seg_verts,
                                    float *seg_radii, uint32_t *seg_prim, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_cylinder_segments, dim3((n + 255u) / 256u), dim3(256), 0, s, verts, radii, seg_off, n, seg_verts, seg_radii, seg_prim);
  return hipGetLastError();
}

// ---- leaf-ordered records ---------------------------------------------------------------------------------------------------
// Leaf-ordered triangle records from (indices, faces, tight vertices).
template <typename T>
__global__ __launch_bounds__(256) void k_gather_leaf_tris(const uint32_t *__restrict__ indices,
                                                          const uint32_t *__restrict__ faces,
                                                          const T *__restrict__ verts,
                                                          LeafTri<T> *__restrict__ out, uint32_t n) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n) return;
  const uint32_t prim = indices[s];
  const uint32_t f0 = faces[3 * (size_t)prim + 0], f1 = faces[3 * (size_t)prim + 1],
                 f2 = faces[3 * (size_t)prim + 2];
  LeafTri<T> t;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    t.p0[k] = verts[3 * (size_t)f0 + k];
    t.p1[k] = verts[3 * (size_t)f1 + k];
    t.p2[k] = verts[3 * (size_t)f2 + k];
  }
  t.prim_id = prim;
  out[s] = t;
}

// Leaf-ordered sphere records from (indices, centers, radii).
template <typename T>
__global__ __launch_bounds__(256) void k_gather_leaf_spheres(const uint32_t *__restrict__ indices,
                                                             const T *__restrict__ centers, const T *__restrict__ radii,
                                                             LeafSphere<T> *__restrict__ out, uint32_t n) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n) return;
  const uint32_t prim = indices[s];
  LeafSphere<T> r;
#pragma unroll
  for (int k = 0; k < 3; k++) r.c[k] = centers[3 * (size_t)prim + k];
  r.r = radii[prim];
  r.prim_id = prim;
  out[s] = r;
}

// Leaf-ordered cylinder records from (indices, end points, radii).
template <typename T>
__global__ __launch_bounds__(256) void k_gather_leaf_cylinders(const uint32_t *__restrict__ indices,
                                                               const T *__restrict__ verts, const T *__restrict__ radii,
                                                               LeafCylinder<T> *__restrict__ out, uint32_t n) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n) return;
  const uint32_t prim = indices[s];
  LeafCylinder<T> r;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    r.p0[k] = verts[3 * (size_t)(2 * prim) + k];
    r.p1[k] = verts[3 * (size_t)(2 * prim + 1) + k];
  }
  r.r0 = radii[2 * (size_t)prim];
  r.r1 = radii[2 * (size_t)prim + 1];
  r.prim_id = prim;
  out[s] = r;
}

// Leaf-ordered curve records from (indices, control points, radii): of a curve's four radii the intersector reads the first
// and the last.  Every byte of the 64-byte record is written.
__global__ __launch_bounds__(256) void k_gather_leaf_curves(const uint32_t *__restrict__ indices, const float *__restrict__ cps,
                                                            const float *__restrict__ radii, LeafCurve *__restrict__ out, uint32_t n) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n) return;
  const uint32_t prim = indices[s];
  LeafCurve r;
#pragma unroll
  for (int k = 0; k < 12; k++) r.cp[k] = cps[12 * (size_t)prim + k];
  r.r0 = radii[4 * (size_t)prim];
  r.r3 = radii[4 * (size_t)prim + 3];
  r.prim_id = prim;
  r.pad = 0u;
  out[s] = r;
}

// ---- post passes -----------------------------------------------------------------------------------------------------------
// SphereIntersector::PostTraversal (examples/particle_primitive/main.cc:262-277) as a pass over the finished
// hit records (the double-precision atan2/acos would otherwise cost the traversal kernel half its occupancy):
// u, v = spherical coordinates of the unit normal at the hit point; atan2/acos in double as there (device
// libm agrees with glibc to the last place or so of the double, i.e. to ~1 ulp of the float result).
template <typename T>
__global__ __launch_bounds__(256) void k_sphere_uv(const typename Wire<T>::Ray *__restrict__ rays,
                                                   typename Wire<T>::Hit *__restrict__ hits,
                                                   const T *__restrict__ centers, uint32_t n, DoneRec *done_rec,
                                                   DoneCount *done_count, uint32_t done_seq) {
  // (grid-stride: a bounded number of blocks, so that the completion hand-off at the end — one returning atomic per block —
  // is paid a couple of thousand times, not once per 256 rays)
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
  typename Wire<T>::Hit h = hits[i];
  if (h.prim_id == kInvalid) continue;
  const typename Wire<T>::Ray r = rays[i];
  const double kPi = 3.14159265358979323846;
  const T h0 = r.org[0] + h.t * r.dir[0], h1 = r.org[1] + h.t * r.dir[1], h2 = r.org[2] + h.t * r.dir[2];
  T n0 = h0 - centers[3 * (size_t)h.prim_id + 0], n1 = h1 - centers[3 * (size_t)h.prim_id + 1],
    n2 = h2 - centers[3 * (size_t)h.prim_id + 2];
  const T len = Const<T>::sqrt((n0 * n0 + n1 * n1) + n2 * n2); // vnormalize (nanort.h:383-398)
  if (Const<T>::abs(len) > Const<T>::eps()) {
    const T inv_len = T(1.0) / len;
    n0 *= inv_len;
    n1 *= inv_len;
    n2 *= inv_len;
  }
  h.u = T(float(atan2(double(n0), double(n2)) + kPi) * 0.5f * float(1.0 / kPi));
  h.v = T(float(acos(double(n1)) / kPi));
  hits[i] = h;
  }
  done_end_blocks(done_rec, done_count, done_seq);
}

// CylinderIntersector::PostTraversal (examples/cylinder_primitive/main.cc:367-418) as a pass over the finished compact
// records {u_param, v_param, t, prim} + mask {bit 0 hit, bit 1 hit_cap_}: the surface normal, into the caller's
// 28-byte records {u, v, normal[3], t, prim_id} (t is the intersector's t; the example never writes isect->t) and
// 0/1 mask.  `verts` holds the two end points of every cylinder (2 x xyz).  A miss writes {0, 0, 0, max_t, ~0}.
struct CylHit32 {
  float u, v, normal[3], t;
  uint32_t prim_id;
};
static_assert(sizeof(CylHit32) == kPrimKinds[kPrimCylinders].hit_bytes, "nrt_cyl_hit_f32");

__global__ __launch_bounds__(256) void k_cylinder_post(const Wire<float>::Ray *__restrict__ rays,
                                                       const Wire<float>::Hit *__restrict__ compact,
                                                       const uint8_t *__restrict__ bits, const float *__restrict__ verts,
                                                       uint32_t n, CylHit32 *__restrict__ out, uint8_t *__restrict__ mask,
                                                       DoneRec *done_rec, DoneCount *done_count, uint32_t done_seq) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) { // (grid-stride: see k_sphere_uv)
  const Wire<float>::Hit h = compact[i];
  const uint8_t b = bits[i];
  CylHit32 o;
  if (b & 1u) {
    const Wire<float>::Ray r = rays[i];
    const float *p0 = verts + 3 * (size_t)(2 * h.prim_id), *p1 = p0 + 3;
    float d01[3], pos[3], nrm[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      d01[k] = p1[k] - p0[k];
      pos[k] = r.org[k] + r.dir[k] * h.t;
    }
    if (b & 2u) { // a cap: +-axis, whichever faces the hit point from the cylinder's middle
      float pc[3];
      cyl_normalize<float>(d01, nrm);
#pragma unroll
      for (int k = 0; k < 3; k++) pc[k] = pos[k] - (d01[k] * 0.5f + p0[k]);
      if (!(cyl_dot<float>(pc, nrm) > 0.0f)) {
        nrm[0] = -nrm[0];
        nrm[1] = -nrm[1];
        nrm[2] = -nrm[2];
      }
    } else { // the side: away from the axis point at parameter v
      float pc[3];
#pragma unroll
      for (int k = 0; k < 3; k++) pc[k] = pos[k] - (p0[k] + h.v * d01[k]);
      cyl_normalize<float>(pc, nrm);
    }
    o.u = h.u;
    o.v = h.v;
    o.normal[0] = nrm[0];
    o.normal[1] = nrm[1];
    o.normal[2] = nrm[2];
    o.t = h.t;
    o.prim_id = h.prim_id;
  } else {
    o.u = o.v = 0.0f;
    o.normal[0] = o.normal[1] = o.normal[2] = 0.0f;
    o.t = h.t; // the kernel's miss record carries max_t
    o.prim_id = kInvalid;
  }
  out[i] = o;
  if (mask) mask[i] = b & 1u;
  }
  done_end_blocks(done_rec, done_count, done_seq);
}

// CurveIntersector::PostTraversal (examples/curves_primitive/main.cc:789-823) as a pass over the finished compact records
// {u_param, v_param, t, prim} + 0/1 mask: the curve's tangent at u (EvaluateBezierTangent :456-462, the power-basis
// coefficients in the example's association) and the normal vnormalize(cross(cross(dir, tangent), tangent)), into the caller's
// 40-byte records {t, prim_id, u, v, tangent[3], normal[3]}.  `cps` holds the four control points of every curve (4 x xyz).
// vnormalize (nanort.h:388-398) leaves a vector shorter than epsilon as it is.  A miss writes {max_t, ~0, 0, 0, 0, 0}.
struct CurveHit32 {
  float t;
  uint32_t prim_id;
  float u, v, tangent[3], normal[3];
};
static_assert(sizeof(CurveHit32) == kPrimKinds[kPrimCurves].hit_bytes, "nrt_curve_hit_f32");

__global__ __launch_bounds__(256) void k_curve_post(const Wire<float>::Ray *__restrict__ rays,
                                                    const Wire<float>::Hit *__restrict__ compact,
                                                    const uint8_t *__restrict__ bits, const float *__restrict__ cps, uint32_t n,
                                                    CurveHit32 *__restrict__ out, uint8_t *__restrict__ mask, DoneRec *done_rec,
                                                    DoneCount *done_count, uint32_t done_seq) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) { // (grid-stride: see k_sphere_uv)
  const Wire<float>::Hit h = compact[i];
  const uint8_t b = bits[i];
  CurveHit32 o;
  if (b & 1u) {
    const Wire<float>::Ray r = rays[i];
    const float *v = cps + 12 * (size_t)h.prim_id;
    float dv[3], tan[3], c1[3], c2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float v0 = v[k], v1 = v[3 + k], v2 = v[6 + k], v3 = v[9 + k];
      const float C1 = ((v3 - v2 * 3.0f) + v1 * 3.0f) - v0;
      const float C2 = (v2 * 3.0f - v1 * 6.0f) + v0 * 3.0f;
      const float C3 = v1 * 3.0f - v0 * 3.0f;
      dv[k] = (((C1 * 3.0f) * h.u) * h.u + (C2 * 2.0f) * h.u) + C3;
    }
    cyl_normalize<float>(dv, tan);
    const float dir[3] = {r.dir[0], r.dir[1], r.dir[2]};
    c1[0] = dir[1] * tan[2] - dir[2] * tan[1]; // vcross (nanort.h:400-407)
    c1[1] = dir[2] * tan[0] - dir[0] * tan[2];
    c1[2] = dir[0] * tan[1] - dir[1] * tan[0];
    c2[0] = c1[1] * tan[2] - c1[2] * tan[1];
    c2[1] = c1[2] * tan[0] - c1[0] * tan[2];
    c2[2] = c1[0] * tan[1] - c1[1] * tan[0];
    cyl_normalize<float>(c2, o.normal);
    o.tangent[0] = tan[0];
    o.tangent[1] = tan[1];
    o.tangent[2] = tan[2];
    o.t = h.t;
    o.prim_id = h.prim_id;
    o.u = h.u;
    o.v = h.v;
  } else {
    o.t = h.t; // the kernel's miss record carries max_t
    o.prim_id = kInvalid;
    o.u = o.v = 0.0f;
    o.tangent[0] = o.tangent[1] = o.tangent[2] = 0.0f;
    o.normal[0] = o.normal[1] = o.normal[2] = 0.0f;
  }
  out[i] = o;
  if (mask) mask[i] = b & 1u;
  }
  done_end_blocks(done_rec, done_count, done_seq);
}

// ---- host-side launchers (kernels.h) ----------------------------------------

template <typename T>
size_t leaf_record_bytes(int kind) {
  return kind == kPrimSpheres ? sizeof(LeafSphere<T>) : kind == kPrimCylinders ? sizeof(LeafCylinder<T>) : kind == kPrimCurves ? sizeof(LeafCurve) : sizeof(LeafTri<T>);
}

template <typename T>
hipError_t launch_gather_leaf(int kind, const uint32_t *indices, const uint32_t *faces, const T *verts, const T *radii, void *out, uint32_t n,
                              hipStream_t s) {
  if (!kPrimKinds[kind].fp64 && sizeof(T) != 4) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const dim3 grid((n + 255u) / 256u), block(256);
  if (kind == kPrimSpheres)
    hipLaunchKernelGGL((k_gather_leaf_spheres<T>), grid, block, 0, s, indices, verts, radii, (LeafSphere<T> *)out, n);
  else if (kind == kPrimCylinders)
    hipLaunchKernelGGL((k_gather_leaf_cylinders<T>), grid, block, 0, s, indices, verts, radii, (LeafCylinder<T> *)out, n);
  else if (kind == kPrimCurves)
    hipLaunchKernelGGL(k_gather_leaf_curves, grid, block, 0, s, indices, (const float *)verts, (const float *)radii, (LeafCurve *)out, n);
  else
    hipLaunchKernelGGL((k_gather_leaf_tris<T>), grid, block, 0, s, indices, faces, verts, (LeafTri<T> *)out, n);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_post_pass(int kind, const typename Wire<T>::Ray *rays, typename Wire<T>::Hit *hits, const uint8_t *bits, const T *verts, uint32_t n,
                            void *out, uint8_t *mask, DoneRec *done_rec, DoneCount *done_count, uint32_t done_seq, hipStream_t s) {
  if (!kPrimKinds[kind].post_pass || (!kPrimKinds[kind].fp64 && sizeof(T) != 4)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const dim3 grid(std::min((n + 255u) / 256u, 2048u)), block(256);
  if (kind == kPrimSpheres)
    hipLaunchKernelGGL((k_sphere_uv<T>), grid, block, 0, s, rays, hits, verts, n, done_rec, done_count, done_seq);
  else if (kind == kPrimCylinders)
    hipLaunchKernelGGL(k_cylinder_post, grid, block, 0, s, (const nrt_ray_f32 *)rays, (const nrt_hit_f32 *)hits, bits, (const float *)verts, n,
                       (CylHit32 *)out, mask, done_rec, done_count, done_seq);
  else
    hipLaunchKernelGGL(k_curve_post, grid, block, 0, s, (const nrt_ray_f32 *)rays, (const nrt_hit_f32 *)hits, bits, (const float *)verts, n,
                       (CurveHit32 *)out, mask, done_rec, done_count, done_seq);
  return hipGetLastError();
}

NRT_INSTANTIATE_F32_F64(launch_gather_vertices)
NRT_INSTANTIATE_F32_F64(launch_permute_masks)
NRT_INSTANTIATE_F32_F64(leaf_record_bytes)
NRT_INSTANTIATE_F32_F64(launch_gather_leaf)
NRT_INSTANTIATE_F32_F64(launch_post_pass)

} // namespace nrt

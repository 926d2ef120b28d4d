// nanort_amd/csrc/sdf.hip — the angle-weighted pseudonormals of the context's triangle mesh, for the signed distance query
// (include/nanort_hip.h, "signed distance queries").  include/nanort_sdf.h states the rule: per face its unit normal
// and, for each of its edges ab, ac, bc, the sum of the unit normals of every face that holds both of the edge's vertex indices;
// per vertex the sum over its corners of angle * unit normal.  Computed from d_verts / d_faces where they lie (a mesh set from the
// device or moved by a refit is never downloaded).
//
// The sums have to come out the same on every run, so nothing is accumulated with floating-point atomics.  The 3 * num_faces
// corner records (key: vertex index, value: corner id 3 * face + k) are sorted by key with the builder's stable radix sort
// (build.hip, launch_sort_pairs): a vertex's corners then stand together in ascending corner id, hence in ascending face id.
//   k_sdf_faces     a thread per face: the unit normal, the three corner angles, the three corner records
//   k_sdf_vertices  a thread per sorted record; the one at the head of a vertex's run walks the run and accumulates in list order
//                   (a fan's centre is one thread's loop, however long), and notes where the run starts and how long it is
//   k_sdf_edges     a thread per (face, edge): scans the SHORTER of the two end points' runs (ties: the smaller index) for faces that
//                   also hold the other end point — each face once: a face that names a vertex twice has its corners side by side —
//                   so the centre of a fan does not cost valence^2 reads.  Which run is scanned does not change the sum: both hold
//                   the faces with both indices in ascending face id.
// Plain loads and stores, no inline assembly.
#include "kernels.h"
#include "../../include/nanort_sdf.h"

namespace nrt {

namespace {

// The carve-up of the workspace: u32 words first, the angles behind them at an 8-byte boundary.
struct SdfPlan {
  size_t n, nb, off_keys0, off_keys1, off_vals0, off_vals1, off_hist, off_vstart, off_vlen, off_angles, total;
  SdfPlan(uint32_t num_faces, uint32_t num_verts, size_t real_bytes) {
    n = 3 * (size_t)num_faces;
    nb = sort_pairs_blocks((uint32_t)n);
    size_t o = 0;
    auto take = [&](size_t words) {
      const size_t at = o;
      o += words * sizeof(uint32_t);
      return at;
    };
    off_keys0 = take(n), off_keys1 = take(n), off_vals0 = take(n), off_vals1 = take(n);
    off_hist = take(256 * nb);
    off_vstart = take(num_verts), off_vlen = take(num_verts);
    o = (o + 7) & ~(size_t)7;
    off_angles = o;
    total = o + n * real_bytes;
  }
};

template <typename T>
__global__ __launch_bounds__(256) void k_sdf_faces(const T *__restrict__ verts, const uint32_t *__restrict__ faces, uint32_t nf, uint32_t nv,
                                                   T *__restrict__ fnormals, T *__restrict__ angles, uint32_t *__restrict__ keys,
                                                   uint32_t *__restrict__ vals) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  if (f >= nf) return;
  const uint32_t i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
  T n[3] = {T(0), T(0), T(0)}, ang[3] = {T(0), T(0), T(0)};
  if (i0 < nv && i1 < nv && i2 < nv) { // (the setters have checked it; a face that names no vertex has no normal)
    const T a[3] = {verts[3 * (size_t)i0], verts[3 * (size_t)i0 + 1], verts[3 * (size_t)i0 + 2]};
    const T b[3] = {verts[3 * (size_t)i1], verts[3 * (size_t)i1 + 1], verts[3 * (size_t)i1 + 2]};
    const T c[3] = {verts[3 * (size_t)i2], verts[3 * (size_t)i2 + 1], verts[3 * (size_t)i2 + 2]};
    nanort_sdf::UnitNormal<T>(a, b, c, n);
    nanort_sdf::CornerAngles<T>(a, b, c, ang);
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    fnormals[12 * (size_t)f + k] = n[k];
    angles[3 * (size_t)f + k] = ang[k];
    vals[3 * (size_t)f + k] = 3u * f + (uint32_t)k;
  }
  keys[3 * (size_t)f] = i0, keys[3 * (size_t)f + 1] = i1, keys[3 * (size_t)f + 2] = i2;
}

template <typename T>
__global__ __launch_bounds__(256) void k_sdf_vertices(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t n, uint32_t nv,
                                                      const T *__restrict__ fnormals, const T *__restrict__ angles, T *__restrict__ vnormals,
                                                      uint32_t *__restrict__ vstart, uint32_t *__restrict__ vlen) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t v = keys[i];
  if ((i != 0u && keys[i - 1u] == v) || v >= nv) return; // not the head of a run
  T acc[3] = {T(0), T(0), T(0)};
  uint32_t j = i;
  for (; j < n && keys[j] == v; j++) {
    const uint32_t corner = vals[j];
    const T w = angles[corner];
    const T *fn = fnormals + 12 * (size_t)(corner / 3u);
    acc[0] = acc[0] + w * fn[0];
    acc[1] = acc[1] + w * fn[1];
    acc[2] = acc[2] + w * fn[2];
  }
  vnormals[3 * (size_t)v] = acc[0], vnormals[3 * (size_t)v + 1] = acc[1], vnormals[3 * (size_t)v + 2] = acc[2];
  vstart[v] = i;
  vlen[v] = j - i;
}

template <typename T>
__global__ __launch_bounds__(256) void k_sdf_edges(const uint32_t *__restrict__ faces, uint32_t nf, uint32_t nv, const uint32_t *__restrict__ vals,
                                                   uint32_t n, const uint32_t *__restrict__ vstart, const uint32_t *__restrict__ vlen,
                                                   T *fnormals) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const uint32_t f = t / 3u, e = t % 3u + 1u;
  unsigned s0, s1;
  nanort_sdf::EdgeSlots(e, &s0, &s1);
  const uint32_t i = faces[3 * (size_t)f + s0], j = faces[3 * (size_t)f + s1];
  T acc[3] = {T(0), T(0), T(0)};
  if (i < nv && j < nv) {
    const uint32_t li = vlen[i], lj = vlen[j];
    const bool second = lj < li || (lj == li && j < i);
    const uint32_t scan = second ? j : i, other = second ? i : j;
    const uint32_t first = vstart[scan], len = second ? lj : li;
    uint32_t last = kInvalid;
    for (uint32_t r = first; r < first + len && r < n; r++) {
      const uint32_t g = vals[r] / 3u;
      if (g == last || g >= nf) continue;
      last = g;
      if (faces[3 * (size_t)g] != other && faces[3 * (size_t)g + 1] != other && faces[3 * (size_t)g + 2] != other) continue;
      const T *gn = fnormals + 12 * (size_t)g; // (slot 0: written by k_sdf_faces; this kernel writes slots 1..3 only)
      acc[0] = acc[0] + gn[0];
      acc[1] = acc[1] + gn[1];
      acc[2] = acc[2] + gn[2];
    }
  }
  T *out = fnormals + 12 * (size_t)f + 3u * e;
  out[0] = acc[0], out[1] = acc[1], out[2] = acc[2];
}

} // namespace

template <typename T>
size_t feature_normals_workspace_bytes(uint32_t num_faces, uint32_t num_verts) {
  return SdfPlan(num_faces, num_verts, sizeof(T)).total;
}

template <typename T>
hipError_t launch_feature_normals(const T *verts, const uint32_t *faces, uint32_t num_faces, uint32_t num_verts, void *workspace, T *face_normals,
                                  T *vertex_normals, hipStream_t s) {
  if ((uint64_t)num_faces * 3u > 0xFFFFFFFFull) return hipErrorInvalidValue;
  hipError_t e;
  if (num_verts && (e = hipMemsetAsync(vertex_normals, 0, 3 * (size_t)num_verts * sizeof(T), s)) != hipSuccess) return e; // (an unreferenced vertex: zero)
  if (num_faces == 0) return hipSuccess;
  const SdfPlan plan(num_faces, num_verts, sizeof(T));
  unsigned char *base = (unsigned char *)workspace;
  uint32_t *keys[2] = {(uint32_t *)(base + plan.off_keys0), (uint32_t *)(base + plan.off_keys1)};
  uint32_t *vals[2] = {(uint32_t *)(base + plan.off_vals0), (uint32_t *)(base + plan.off_vals1)};
  uint32_t *hist = (uint32_t *)(base + plan.off_hist), *vstart = (uint32_t *)(base + plan.off_vstart), *vlen = (uint32_t *)(base + plan.off_vlen);
  T *angles = (T *)(base + plan.off_angles);
  const uint32_t n = (uint32_t)plan.n;
  const unsigned face_blocks = (num_faces + 255u) / 256u, corner_blocks = (unsigned)((plan.n + 255u) / 256u);
  if ((e = hipMemsetAsync(vstart, 0, 2 * (size_t)num_verts * sizeof(uint32_t), s)) != hipSuccess) return e; // (vstart and vlen lie together)
  hipLaunchKernelGGL((k_sdf_faces<T>), dim3(face_blocks), dim3(256), 0, s, verts, faces, num_faces, num_verts, face_normals, angles, keys[0], vals[0]);
  if ((e = launch_sort_pairs(keys, vals, hist, n, s)) != hipSuccess) return e;
  hipLaunchKernelGGL((k_sdf_vertices<T>), dim3(corner_blocks), dim3(256), 0, s, keys[0], vals[0], n, num_verts, face_normals, angles, vertex_normals,
                     vstart, vlen);
  hipLaunchKernelGGL((k_sdf_edges<T>), dim3(corner_blocks), dim3(256), 0, s, faces, num_faces, num_verts, vals[0], n, vstart, vlen, face_normals);
  return hipGetLastError();
}

NRT_INSTANTIATE_F32_F64(feature_normals_workspace_bytes)
NRT_INSTANTIATE_F32_F64(launch_feature_normals)

} // namespace nrt

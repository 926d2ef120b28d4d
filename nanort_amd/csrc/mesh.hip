// nanort_amd/csrc/mesh.hip — geometry that is already in HBM (nrtSetMeshDevice* / nrtSetSpheresDevice*, include/nanort_hip.h):
// what nrtSetMesh does on the host, on the device.
//
//   k_max_index        the largest of 3 * num_faces u32 -> one word: the mesh's vertex count is that + 1, and the caller's
//                      num_vertices is checked against it before any vertex is read
//   k_gather_vertices  strided rows -> the context's tight xyz (also the vertex pass of a refit, refit.hip)
//
// max over u32 is exact and order-free: the word never depends on scheduling.
#include <algorithm>

#include "kernels.h"

namespace nrt {

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

NRT_INSTANTIATE_F32_F64(launch_gather_vertices)

} // namespace nrt

// tests/cpp/query_backend_check.cc — include/nanort.h's combined query WITH the HIP backend (tests/test_gpu_query.py): Build() over
// (MotionTriangleMesh, MotionTriangleSAHPred) runs on the GPU; after SetPrimMasks(), TraverseBatchQuery(q) — for each of the
// combinations of MOTION, MASKED and per-ray skip ids, closest hit and occlusion — must equal the header's own host form,
// TraverseBatchQuery(q, QueryTriangleIntersector), over the read-back tree, byte for byte.  A MASKED query on an accel without masks
// refuses.
//
//   query_backend_check <f32|f64> mesh.bin rays.bin range0 range1 skip cull
//   mesh.bin: u32 nv, u32 nf, T v0[nv][3], T v1[nv][3], u32 faces[nf][3], u32 prim_masks[nf]
//   rays.bin: u64 n, Ray<T> rays[n], T times[n], u32 ray_masks[n], u32 skip_prim_ids[n]
// Prints one line "ok <hits> <rays>" and returns 0, or says what differs and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nanort.h"

template <typename T>
static bool read_exact(FILE *fp, T *dst, size_t count) {
  return count == 0 || fread(dst, sizeof(T), count, fp) == count;
}

template <typename T>
static bool same_record(const nanort::TriangleIntersection<T> &a, const nanort::TriangleIntersection<T> &b) {
  return memcmp(&a.u, &b.u, sizeof(T)) == 0 && memcmp(&a.v, &b.v, sizeof(T)) == 0 && memcmp(&a.t, &b.t, sizeof(T)) == 0 && a.prim_id == b.prim_id;
}

template <typename T>
static int run(char **argv) {
  FILE *fp = fopen(argv[2], "rb");
  if (!fp) return 2;
  uint32_t nv = 0, nf = 0;
  if (!read_exact(fp, &nv, 1) || !read_exact(fp, &nf, 1)) return 2;
  std::vector<T> v0(3 * (size_t)nv), v1(3 * (size_t)nv);
  std::vector<unsigned int> faces(3 * (size_t)nf), prim_masks((size_t)nf);
  if (!read_exact(fp, v0.data(), v0.size()) || !read_exact(fp, v1.data(), v1.size()) || !read_exact(fp, faces.data(), faces.size()) ||
      !read_exact(fp, prim_masks.data(), prim_masks.size()))
    return 2;
  fclose(fp);
  fp = fopen(argv[3], "rb");
  if (!fp) return 2;
  uint64_t n64 = 0;
  if (!read_exact(fp, &n64, 1)) return 2;
  const size_t n = (size_t)n64;
  std::vector<nanort::Ray<T> > rays(n);
  std::vector<T> times(n);
  std::vector<unsigned int> ray_masks(n), skip_ids(n);
  if (!read_exact(fp, rays.data(), n) || !read_exact(fp, times.data(), n) || !read_exact(fp, ray_masks.data(), n) || !read_exact(fp, skip_ids.data(), n)) return 2;
  fclose(fp);

  nanort::BVHTraceOptions opt;
  opt.prim_ids_range[0] = (unsigned int)strtoul(argv[4], NULL, 10);
  opt.prim_ids_range[1] = (unsigned int)strtoul(argv[5], NULL, 10);
  opt.skip_prim_id = (unsigned int)strtoul(argv[6], NULL, 10);
  opt.cull_back_face = atoi(argv[7]) != 0;

  const size_t stride = 3 * sizeof(T);
  nanort::MotionTriangleMesh<T> mesh(v0.data(), v1.data(), faces.data(), stride);
  nanort::MotionTriangleSAHPred<T> pred(v0.data(), v1.data(), faces.data(), stride);
  nanort::BVHAccel<T> accel;
  if (!accel.Build(nf, mesh, pred)) {
    fprintf(stderr, "Build failed: %s\n", accel.LastBackendError().c_str());
    return 1;
  }

  std::vector<nanort::TriangleIntersection<T> > gpu(n), host(n);
  std::vector<unsigned char> gpu_flags(n), gpu_occ(n), host_flags(n);
  nanort::BatchQuery<T> q;
  q.rays = rays.data();
  q.num_rays = n;
  q.times = times.data();
  q.ray_masks = ray_masks.data();
  q.options = opt;

  // no masks yet: a MASKED query is refused with a reason
  q.masked = true;
  q.isects = gpu.data();
  if (accel.TraverseBatchQuery(q) || accel.LastBackendError().empty()) {
    fprintf(stderr, "a MASKED query on an accel without masks did not refuse\n");
    return 1;
  }
  if (!accel.SetPrimMasks(prim_masks.data(), nf)) {
    fprintf(stderr, "SetPrimMasks failed: %s\n", accel.LastBackendError().c_str());
    return 1;
  }

  long hits = 0;
  for (unsigned features = 0; features < 8; features++) {  // bit 0 MOTION, bit 1 MASKED, bit 2 per-ray skip ids
    q.motion = (features & 1u) != 0u;
    q.masked = (features & 2u) != 0u;
    q.skip_prim_ids = (features & 4u) ? skip_ids.data() : NULL;
    memset(gpu.data(), 0xAB, gpu.size() * sizeof(gpu[0]));
    memset(host.data(), 0xAB, host.size() * sizeof(host[0]));
    std::fill(gpu_flags.begin(), gpu_flags.end(), 9);
    std::fill(gpu_occ.begin(), gpu_occ.end(), 9);
    q.occlusion = false;
    q.isects = gpu.data();
    q.hit_out = gpu_flags.data();
    if (!accel.TraverseBatchQuery(q)) {
      fprintf(stderr, "features %u: TraverseBatchQuery failed: %s\n", features, accel.LastBackendError().c_str());
      return 1;
    }
    q.occlusion = true;
    q.isects = NULL;
    q.hit_out = gpu_occ.data();
    if (!accel.TraverseBatchQuery(q)) {
      fprintf(stderr, "features %u: the occlusion query failed: %s\n", features, accel.LastBackendError().c_str());
      return 1;
    }
    const nanort::QueryTriangleIntersector<T> isector(v0.data(), faces.data(), stride, q.motion ? v1.data() : NULL, q.masked ? prim_masks.data() : NULL);
    q.occlusion = false;
    q.isects = host.data();
    q.hit_out = host_flags.data();
    if (!accel.TraverseBatchQuery(q, isector)) return 1;
    for (size_t i = 0; i < n; i++) {
      hits += host_flags[i];
      if (gpu_flags[i] != host_flags[i] || gpu_occ[i] != host_flags[i] || !same_record(host[i], gpu[i])) {
        fprintf(stderr, "features %u, ray %zu: host hit %d t %.9g prim %u, GPU flag %d occluded %d t %.9g prim %u\n", features, i, host_flags[i],
                (double)host[i].t, host[i].prim_id, gpu_flags[i], gpu_occ[i], (double)gpu[i].t, gpu[i].prim_id);
        return 1;
      }
    }
  }
  printf("ok %ld %zu\n", hits, n);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 8) {
    fprintf(stderr, "usage: %s <f32|f64> mesh.bin rays.bin range0 range1 skip cull\n", argv[0]);
    return 1;
  }
  return std::string(argv[1]) == "f64" ? run<double>(argv) : run<float>(argv);
}

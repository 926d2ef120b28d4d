// tests/cpp/motion_check.cc — include/nanort.h's motion blur WITH the HIP backend (tests/test_gpu_motion.py): Build() over
// (MotionTriangleMesh, MotionTriangleSAHPred) runs on the GPU; TraverseBatchMotion() / OccludedBatchMotion() must equal the header's
// own per-ray Traverse() with a MotionTriangleIntersector set to each ray's time, over the read-back tree, byte for byte; the
// triangle batch call answers for keyframe 0; Refit() refuses.
//
//   motion_check <f32|f64> mesh.bin rays.bin range0 range1 skip cull
//   mesh.bin: u32 nv, u32 nf, T v0[nv][3], T v1[nv][3], u32 faces[nf][3]
//   rays.bin: u64 n, Ray<T> rays[n], T times[n]
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
  std::vector<unsigned int> faces(3 * (size_t)nf);
  if (!read_exact(fp, v0.data(), v0.size()) || !read_exact(fp, v1.data(), v1.size()) || !read_exact(fp, faces.data(), faces.size())) return 2;
  fclose(fp);
  fp = fopen(argv[3], "rb");
  if (!fp) return 2;
  uint64_t n64 = 0;
  if (!read_exact(fp, &n64, 1)) return 2;
  const size_t n = (size_t)n64;
  std::vector<nanort::Ray<T> > rays(n);
  std::vector<T> times(n);
  if (!read_exact(fp, rays.data(), rays.size()) || !read_exact(fp, times.data(), times.size())) return 2;
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

  // the batch calls first: the tree has not been read back yet
  std::vector<nanort::TriangleIntersection<T> > batch(n);
  std::vector<unsigned char> flags(n, 9), occ(n, 9);
  memset(batch.data(), 0xAB, batch.size() * sizeof(batch[0]));
  if (!accel.TraverseBatchMotion(rays.data(), times.data(), n, batch.data(), flags.data(), opt) ||
      !accel.OccludedBatchMotion(rays.data(), times.data(), n, occ.data(), opt)) {
    fprintf(stderr, "motion batch call failed: %s\n", accel.LastBackendError().c_str());
    return 1;
  }

  // the header's own per-ray walk over the read-back tree
  nanort::MotionTriangleIntersector<T> isector(mesh);
  size_t hits = 0;
  for (size_t i = 0; i < n; i++) {
    nanort::TriangleIntersection<T> h;
    h.u = h.v = T(0);
    h.t = rays[i].max_t;
    h.prim_id = 0xFFFFFFFFu;
    isector.SetTime(times[i]);
    const unsigned char hit = accel.Traverse(rays[i], isector, &h, opt) ? 1 : 0;
    hits += hit;
    if (flags[i] != hit || occ[i] != hit || !same_record(h, batch[i])) {
      fprintf(stderr, "ray %zu (time %g): host hit %d t %.9g prim %u, batch flag %d occluded %d t %.9g prim %u\n", i, (double)times[i], hit,
              (double)h.t, h.prim_id, flags[i], occ[i], (double)batch[i].t, batch[i].prim_id);
      return 1;
    }
  }

  // the triangle batch call on the same accel answers for keyframe 0
  {
    nanort::TriangleIntersector<T> k0(v0.data(), faces.data(), stride);
    std::vector<nanort::TriangleIntersection<T> > tb(n);
    std::vector<unsigned char> tf(n, 9);
    if (!accel.TraverseBatch(rays.data(), n, tb.data(), tf.data(), opt)) {
      fprintf(stderr, "TraverseBatch failed: %s\n", accel.LastBackendError().c_str());
      return 1;
    }
    for (size_t i = 0; i < n; i++) {
      nanort::TriangleIntersection<T> h;
      const bool hit = accel.Traverse(rays[i], k0, &h, opt);
      if (tf[i] != (hit ? 1 : 0) || (hit && !same_record(h, tb[i]))) {
        fprintf(stderr, "keyframe 0, ray %zu: host hit %d, batch flag %d\n", i, (int)hit, tf[i]);
        return 1;
      }
    }
  }

  // Refit() refuses, with a reason, and the accel still answers
  nanort::TriangleMesh<T> plain(v1.data(), faces.data(), stride);
  if (accel.Refit(plain) || accel.LastBackendError().empty()) {
    fprintf(stderr, "Refit() on a motion accel did not refuse\n");
    return 1;
  }
  std::vector<unsigned char> occ2(n, 9);
  if (!accel.OccludedBatchMotion(rays.data(), times.data(), n, occ2.data(), opt) || memcmp(occ2.data(), occ.data(), n) != 0) {
    fprintf(stderr, "the accel answers differently after the refused Refit()\n");
    return 1;
  }
  // a motion query on an accel built over a plain mesh is refused
  nanort::TriangleSAHPred<T> ppred(v0.data(), faces.data(), stride);
  nanort::TriangleMesh<T> pmesh(v0.data(), faces.data(), stride);
  nanort::BVHAccel<T> paccel;
  if (!paccel.Build(nf, pmesh, ppred) || paccel.OccludedBatchMotion(rays.data(), times.data(), n, occ2.data(), opt) || paccel.LastBackendError().empty()) {
    fprintf(stderr, "a motion query on a plain accel did not refuse\n");
    return 1;
  }
  printf("ok %zu %zu\n", hits, n);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 8) {
    fprintf(stderr, "usage: %s <f32|f64> mesh.bin rays.bin range0 range1 skip cull\n", argv[0]);
    return 1;
  }
  return std::string(argv[1]) == "f64" ? run<double>(argv) : run<float>(argv);
}

// tests/cpp/multihit_query_check.cc — include/nanort.h's MultiHitBatchQuery and BVHAccel::MultiHitTraverseBatchQuery().
//
// Compiled WITHOUT NANORT_USE_HIP_BACKEND (tests/test_multihit_query_model.py): a tree Load()ed from the file the test wrote, the host
// form MultiHitTraverseBatchQuery(q, QueryTriangleIntersector) over all the rays; counts and rows go to out.bin, where the test
// compares them with its expectation over the same tree.  One MultiHitTraverse() per ray with SetRay() must equal it (exit 4), and
// a query without rows, with K = 0 or K = 65 is refused (exit 5).
//
//   multihit_query_check <f32|f64> mesh.bin tree.bin rays.bin out.bin K features
//   features: 2 MOTION | 4 MASKED (NRT_QUERY_*) | 8 per-ray skip ids
//   mesh.bin: u32 nv, u32 nf, T v0[nv][3], T v1[nv][3], u32 faces[nf][3], u32 prim_masks[nf]
//   tree.bin: the format of BVHAccel::Dump / Load (size_t count, nodes, size_t count, indices)
//   rays.bin: u64 n, Ray<T> rays[n], T times[n], u32 ray_masks[n], u32 skip_prim_ids[n]
//   out.bin:  u32 counts[n], TriangleIntersection<T> rows[n][K]
//
// Compiled WITH the backend (tests/test_gpu_multihit_query.py; tree.bin, out.bin and features are not read): Build() over
// (MotionTriangleMesh, MotionTriangleSAHPred) runs on the GPU; after SetPrimMasks(), MultiHitTraverseBatchQuery(q) — for each of the
// eight combinations of MOTION, MASKED and per-ray skip ids — must equal the header's own host form over the read-back tree, byte for
// byte.  Prints one line "ok <held hits> <rays>" and returns 0, or says what differs and returns 1.
#define NANORT_ENABLE_SERIALIZATION
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
  fp = fopen(argv[4], "rb");
  if (!fp) return 2;
  uint64_t n64 = 0;
  if (!read_exact(fp, &n64, 1)) return 2;
  const size_t n = (size_t)n64;
  std::vector<nanort::Ray<T> > rays(n);
  std::vector<T> times(n);
  std::vector<unsigned int> ray_masks(n), skip_ids(n);
  if (!read_exact(fp, rays.data(), n) || !read_exact(fp, times.data(), n) || !read_exact(fp, ray_masks.data(), n) || !read_exact(fp, skip_ids.data(), n)) return 2;
  fclose(fp);
  const unsigned int K = (unsigned int)strtoul(argv[6], NULL, 10);
  const size_t stride = 3 * sizeof(T);

  nanort::MultiHitBatchQuery<T> q;
  q.rays = rays.data();
  q.num_rays = n;
  q.times = times.data();  // (all three arrays are always given: the flags say which are read)
  q.ray_masks = ray_masks.data();
  q.max_hits = K;
  std::vector<nanort::TriangleIntersection<T> > rows(n * (size_t)K);
  std::vector<unsigned int> counts(n, 0xA5A5A5A5u);
  memset(rows.data(), 0, rows.size() * sizeof(rows[0]));  // (fp64 records: the padding too)

#ifndef NANORT_USE_HIP_BACKEND
  const unsigned features = (unsigned)strtoul(argv[7], NULL, 10);
  const bool motion = (features & 2u) != 0u, masked = (features & 4u) != 0u, ids = (features & 8u) != 0u;
  nanort::BVHAccel<T> accel;
  if (!accel.Load(argv[3])) return 3;
  const nanort::QueryTriangleIntersector<T> isector(v0.data(), faces.data(), stride, motion ? v1.data() : NULL, masked ? prim_masks.data() : NULL);
  q.skip_prim_ids = ids ? skip_ids.data() : NULL;
  q.motion = motion;
  q.masked = masked;
  q.isects = rows.data();
  q.counts_out = counts.data();
  if (!accel.MultiHitTraverseBatchQuery(q, isector)) return 3;

  // one MultiHitTraverse() per ray
  for (size_t i = 0; i < n; i++) {
    nanort::StackVector<nanort::TriangleIntersection<T>, 128> held;
    isector.SetRay(motion ? times[i] : T(0), masked ? ray_masks[i] : 0xFFFFFFFFu, ids ? skip_ids[i] : q.options.skip_prim_id);
    accel.MultiHitTraverse(rays[i], (int)K, isector, &held, q.options);
    bool same = held->size() == counts[i];
    for (size_t j = 0; same && j < K; j++) {
      nanort::TriangleIntersection<T> want;
      want.u = want.v = T(0);
      want.t = rays[i].max_t;
      want.prim_id = 0xFFFFFFFFu;
      if (j < held->size()) want = held[j];
      same = same_record(want, rows[i * K + j]);
    }
    if (!same) {
      fprintf(stderr, "ray %zu: MultiHitTraverseBatchQuery differs from MultiHitTraverse with QueryTriangleIntersector\n", i);
      return 4;
    }
  }

  // refusals: nothing written
  nanort::MultiHitBatchQuery<T> bad = q;
  bad.isects = NULL;
  if (accel.MultiHitTraverseBatchQuery(bad, isector)) return 5;
  bad = q;
  bad.max_hits = 0;
  if (accel.MultiHitTraverseBatchQuery(bad, isector)) return 5;
  bad.max_hits = 65;
  if (accel.MultiHitTraverseBatchQuery(bad, isector)) return 5;
  q.counts_out = NULL;  // ... and the counts are optional
  if (!accel.MultiHitTraverseBatchQuery(q, isector)) return 5;

  fp = fopen(argv[5], "wb");
  if (!fp) return 2;
  fwrite(counts.data(), sizeof(counts[0]), counts.size(), fp);
  fwrite(rows.data(), sizeof(rows[0]), rows.size(), fp);
  fclose(fp);
  return 0;
#else
  nanort::MotionTriangleMesh<T> mesh(v0.data(), v1.data(), faces.data(), stride);
  nanort::MotionTriangleSAHPred<T> pred(v0.data(), v1.data(), faces.data(), stride);
  nanort::BVHAccel<T> accel;
  if (!accel.Build(nf, mesh, pred)) {
    fprintf(stderr, "Build failed: %s\n", accel.LastBackendError().c_str());
    return 1;
  }
  // no masks yet: a MASKED query is refused with a reason
  q.masked = true;
  q.isects = rows.data();
  if (accel.MultiHitTraverseBatchQuery(q) || accel.LastBackendError().empty()) {
    fprintf(stderr, "a MASKED query on an accel without masks did not refuse\n");
    return 1;
  }
  if (!accel.SetPrimMasks(prim_masks.data(), nf)) {
    fprintf(stderr, "SetPrimMasks failed: %s\n", accel.LastBackendError().c_str());
    return 1;
  }
  std::vector<nanort::TriangleIntersection<T> > host(rows.size());
  std::vector<unsigned int> host_counts(n);
  long held = 0;
  for (unsigned features = 0; features < 8; features++) {  // bit 0 MOTION, bit 1 MASKED, bit 2 per-ray skip ids
    q.motion = (features & 1u) != 0u;
    q.masked = (features & 2u) != 0u;
    q.skip_prim_ids = (features & 4u) ? skip_ids.data() : NULL;
    memset(rows.data(), 0xAB, rows.size() * sizeof(rows[0]));
    memset(host.data(), 0xAB, host.size() * sizeof(host[0]));
    std::fill(counts.begin(), counts.end(), 0xA5A5A5A5u);
    q.isects = rows.data();
    q.counts_out = counts.data();
    if (!accel.MultiHitTraverseBatchQuery(q)) {
      fprintf(stderr, "features %u: MultiHitTraverseBatchQuery failed: %s\n", features, accel.LastBackendError().c_str());
      return 1;
    }
    const nanort::QueryTriangleIntersector<T> isector(v0.data(), faces.data(), stride, q.motion ? v1.data() : NULL, q.masked ? prim_masks.data() : NULL);
    q.isects = host.data();
    q.counts_out = host_counts.data();
    if (!accel.MultiHitTraverseBatchQuery(q, isector)) return 1;
    for (size_t i = 0; i < n; i++) {
      held += host_counts[i];
      bool same = counts[i] == host_counts[i];
      for (size_t j = 0; same && j < K; j++) same = same_record(host[i * K + j], rows[i * K + j]);
      if (!same) {
        fprintf(stderr, "features %u, ray %zu: host count %u first t %.9g prim %u, GPU count %u first t %.9g prim %u\n", features, i, host_counts[i],
                (double)host[i * K].t, host[i * K].prim_id, counts[i], (double)rows[i * K].t, rows[i * K].prim_id);
        return 1;
      }
    }
  }
  printf("ok %ld %zu\n", held, n);
  return 0;
#endif
}

int main(int argc, char **argv) {
  if (argc < 8) {
    fprintf(stderr, "usage: %s <f32|f64> mesh.bin tree.bin rays.bin out.bin K features\n", argv[0]);
    return 1;
  }
  return std::string(argv[1]) == "f64" ? run<double>(argv) : run<float>(argv);
}

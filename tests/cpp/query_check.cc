// tests/cpp/query_check.cc — include/nanort.h's QueryTriangleIntersector, BatchQuery and the host TraverseBatchQuery(), compiled
// without NANORT_USE_HIP_BACKEND (tests/test_query_model.py): a tree Load()ed from the file the test wrote (the oracle's), then
//   1. TraverseBatchQuery(q, intersector) over all the rays: its records go to out.bin, where the test compares them with its
//      expectation over the same tree;
//   2. one Traverse() per ray with a QueryTriangleIntersector on which SetRay() was called: must equal 1 in every field (exit 4);
//   3. when the query has MOTION alone: MotionTriangleIntersector with SetTime() must equal 1 (exit 5);
//      when it has MASKED alone: MaskedTriangleIntersector with SetRayMask() must equal 1 (exit 6);
//   4. the occlusion form's flags must equal 1's flags (exit 7).
//
//   query_check <f32|f64> mesh.bin tree.bin rays.bin out.bin range0 range1 skip cull features
//   features: 2 MOTION | 4 MASKED (NRT_QUERY_*) | 8 per-ray skip ids
//   mesh.bin: u32 nv, u32 nf, T v0[nv][3], T v1[nv][3], u32 faces[nf][3], u32 prim_masks[nf]
//   tree.bin: the format of BVHAccel::Dump / Load (size_t count, nodes, size_t count, indices)
//   rays.bin: u64 n, Ray<T> rays[n], T times[n], u32 ray_masks[n], u32 skip_prim_ids[n]
//   out.bin:  TriangleIntersection<T> hits[n], u8 mask[n]
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
static void miss_record(nanort::TriangleIntersection<T> *h, const nanort::Ray<T> &ray) {
  h->u = h->v = T(0);
  h->t = ray.max_t;
  h->prim_id = 0xFFFFFFFFu;
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

  nanort::BVHTraceOptions opt;
  opt.prim_ids_range[0] = (unsigned int)strtoul(argv[6], NULL, 10);
  opt.prim_ids_range[1] = (unsigned int)strtoul(argv[7], NULL, 10);
  opt.skip_prim_id = (unsigned int)strtoul(argv[8], NULL, 10);
  opt.cull_back_face = atoi(argv[9]) != 0;
  const unsigned features = (unsigned)strtoul(argv[10], NULL, 10);
  const bool motion = (features & 2u) != 0u, masked = (features & 4u) != 0u, ids = (features & 8u) != 0u;

  nanort::BVHAccel<T> accel;
  if (!accel.Load(argv[3])) return 3;

  const size_t stride = 3 * sizeof(T);
  const nanort::QueryTriangleIntersector<T> isector(v0.data(), faces.data(), stride, motion ? v1.data() : NULL, masked ? prim_masks.data() : NULL);

  // 1. the batch form
  std::vector<nanort::TriangleIntersection<T> > hits(n);
  std::vector<unsigned char> mask(n, 0xA5);
  memset(hits.data(), 0, hits.size() * sizeof(hits[0]));  // (fp64 records: the padding too)
  nanort::BatchQuery<T> q;
  q.rays = rays.data();
  q.num_rays = n;
  q.times = times.data();  // (all three arrays are always given: the flags say which are read)
  q.ray_masks = ray_masks.data();
  q.skip_prim_ids = ids ? skip_ids.data() : NULL;
  q.motion = motion;
  q.masked = masked;
  q.options = opt;
  q.isects = hits.data();
  q.hit_out = mask.data();
  if (!accel.TraverseBatchQuery(q, isector)) return 3;

  // 2. the per-ray form
  for (size_t i = 0; i < n; i++) {
    nanort::TriangleIntersection<T> h;
    miss_record(&h, rays[i]);
    isector.SetRay(motion ? times[i] : T(0), masked ? ray_masks[i] : 0xFFFFFFFFu, ids ? skip_ids[i] : opt.skip_prim_id);
    const unsigned char f = accel.Traverse(rays[i], isector, &h, opt) ? 1 : 0;
    if (f != mask[i] || !same_record(h, hits[i])) {
      fprintf(stderr, "ray %zu: TraverseBatchQuery differs from Traverse with QueryTriangleIntersector\n", i);
      return 4;
    }
  }

  // 3. one feature alone: the existing intersectors
  if (motion && !masked && !ids) {
    const nanort::MotionTriangleIntersector<T> mi(v0.data(), v1.data(), faces.data(), stride);
    for (size_t i = 0; i < n; i++) {
      nanort::TriangleIntersection<T> h;
      miss_record(&h, rays[i]);
      mi.SetTime(times[i]);
      const unsigned char f = accel.Traverse(rays[i], mi, &h, opt) ? 1 : 0;
      if (f != mask[i] || !same_record(h, hits[i])) {
        fprintf(stderr, "ray %zu: differs from MotionTriangleIntersector\n", i);
        return 5;
      }
    }
  }
  if (masked && !motion && !ids) {
    const nanort::MaskedTriangleIntersector<T> ki(v0.data(), faces.data(), stride, prim_masks.data());
    for (size_t i = 0; i < n; i++) {
      nanort::TriangleIntersection<T> h;
      miss_record(&h, rays[i]);
      ki.SetRayMask(ray_masks[i]);
      const unsigned char f = accel.Traverse(rays[i], ki, &h, opt) ? 1 : 0;
      if (f != mask[i] || !same_record(h, hits[i])) {
        fprintf(stderr, "ray %zu: differs from MaskedTriangleIntersector\n", i);
        return 6;
      }
    }
  }

  // 4. the occlusion form: the same flags, no records
  std::vector<unsigned char> occ(n, 0xA5);
  q.occlusion = true;
  q.isects = NULL;
  q.hit_out = occ.data();
  if (!accel.TraverseBatchQuery(q, isector)) return 3;
  if (memcmp(occ.data(), mask.data(), n) != 0) {
    fprintf(stderr, "the occlusion flags differ from the closest-hit flags\n");
    return 7;
  }
  q.hit_out = NULL;  // ... and a query with rays and without its output is refused
  if (accel.TraverseBatchQuery(q, isector)) return 7;

  fp = fopen(argv[5], "wb");
  if (!fp) return 2;
  fwrite(hits.data(), sizeof(hits[0]), hits.size(), fp);
  fwrite(mask.data(), 1, mask.size(), fp);
  fclose(fp);
  return 0;
}

#ifdef NANORT_USE_HIP_BACKEND
// The backend's forms, instantiated for both precisions (the test compiles this file with the backend to an object, -Werror).
template <typename T>
bool backend_forms(const nanort::BVHAccel<T> &accel, const nanort::BatchQuery<T> &q, void *hip_stream) {
  return accel.TraverseBatchQuery(q) && accel.TraverseBatchQueryDevice(q, hip_stream);
}
template bool backend_forms<float>(const nanort::BVHAccel<float> &, const nanort::BatchQuery<float> &, void *);
template bool backend_forms<double>(const nanort::BVHAccel<double> &, const nanort::BatchQuery<double> &, void *);
#endif

int main(int argc, char **argv) {
  if (argc < 11) {
    fprintf(stderr, "usage: %s <f32|f64> mesh.bin tree.bin rays.bin out.bin range0 range1 skip cull features\n", argv[0]);
    return 1;
  }
  return std::string(argv[1]) == "f64" ? run<double>(argv) : run<float>(argv);
}

// tests/cpp/skip_ids_check.cc — per-ray skip ids through include/nanort.h (tests/test_skip_ids_cpu.py, tests/test_gpu_skip_ids.py).
//
// Two sheets of triangles one behind the other, rays through both.  Wave 1 is traced per ray; wave 2 traces the same rays, each
// skipping the triangle it hit in wave 1 (some rays carry the sentinel, an id beyond the mesh or a triangle they do not hit).
//  * without NANORT_USE_HIP_BACKEND: the header's host TraverseBatch(rays, n, intersector, ..., skip_prim_ids)
//  * with it:                        BVHAccel::TraverseBatch / OccludedBatch(..., skip_prim_ids) on the GPU
// against the accel's own per-ray Traverse() with that ray's options, every field bit for bit.
#include <cstdio>
#include <cstring>
#include <vector>

#include "nanort.h"

typedef float real;

static unsigned int lcg(unsigned int *s) {
  *s = *s * 1664525u + 1013904223u;
  return *s >> 8;
}

int main() {
  const int N = 12;  // 2 sheets x N x N x 2 = 576 triangles
  std::vector<real> verts;
  std::vector<unsigned int> faces;
  for (int sheet = 0; sheet < 2; sheet++) {
    const unsigned int base = static_cast<unsigned int>(verts.size() / 3);
    for (int y = 0; y <= N; y++)
      for (int x = 0; x <= N; x++) {
        verts.push_back(static_cast<real>(x) / N * 2 - 1);
        verts.push_back(static_cast<real>(y) / N * 2 - 1);
        verts.push_back(static_cast<real>(sheet) + static_cast<real>(0.05) * static_cast<real>((x * 7 + y * 3) % 5));
      }
    for (int y = 0; y < N; y++)
      for (int x = 0; x < N; x++) {
        const unsigned int a = base + y * (N + 1) + x, b = a + 1, c = a + (N + 1), d = c + 1;
        const unsigned int q[6] = {a, b, c, b, d, c};
        faces.insert(faces.end(), q, q + 6);
      }
  }
  const unsigned int nfaces = static_cast<unsigned int>(faces.size() / 3);
  nanort::TriangleMesh<real> mesh(&verts[0], &faces[0], sizeof(real) * 3);
  nanort::TriangleSAHPred<real> pred(&verts[0], &faces[0], sizeof(real) * 3);
  nanort::BVHAccel<real> accel;
  if (!accel.Build(nfaces, mesh, pred)) {
    std::printf("build failed\n");
    return 1;
  }
  nanort::TriangleIntersector<real> isector(&verts[0], &faces[0], sizeof(real) * 3);

  const size_t n = 1500;
  std::vector<nanort::Ray<real> > rays(n);
  unsigned int seed = 12345u;
  for (size_t i = 0; i < n; i++) {
    nanort::Ray<real> &r = rays[i];
    r.org[0] = static_cast<real>(lcg(&seed) % 2000) / 1000 - 1;
    r.org[1] = static_cast<real>(lcg(&seed) % 2000) / 1000 - 1;
    r.org[2] = -2;
    r.dir[0] = (static_cast<real>(lcg(&seed) % 200) - 100) / 1000;
    r.dir[1] = (static_cast<real>(lcg(&seed) % 200) - 100) / 1000;
    r.dir[2] = 1;
    r.min_t = 0;
    r.max_t = static_cast<real>(1.0e30);
  }
  // wave 1, per ray; its prim_id column is wave 2's ids
  std::vector<unsigned int> ids(n, 0xFFFFFFFFu);
  size_t hit1 = 0;
  for (size_t i = 0; i < n; i++) {
    nanort::TriangleIntersection<real> isect;
    if (accel.Traverse(rays[i], isector, &isect)) {
      ids[i] = isect.prim_id;
      hit1++;
    }
    if (i % 3 == 2) ids[i] = 0xFFFFFFFFu;             // the sentinel
    if (i % 5 == 4) ids[i] = nfaces + static_cast<unsigned int>(i);  // beyond the mesh
    if (i % 7 == 6) ids[i] = (ids[i] + nfaces / 2) % nfaces;         // some other triangle
  }
  // the expected records: per-ray Traverse() with per-ray options
  nanort::BVHTraceOptions base;
  std::vector<nanort::TriangleIntersection<real> > want(n), got(n);
  std::vector<unsigned char> want_hit(n), got_hit(n, 7), got_occ(n, 7);
  std::memset(static_cast<void *>(&want[0]), 0xAB, n * sizeof(want[0]));
  std::memset(static_cast<void *>(&got[0]), 0xAB, n * sizeof(got[0]));
  size_t hit2 = 0, unpeeled = 0;
  for (size_t i = 0; i < n; i++) {
    nanort::BVHTraceOptions o = base;
    o.skip_prim_id = ids[i];
    nanort::TriangleIntersection<real> isect;
    const bool hit = accel.Traverse(rays[i], isector, &isect, o);
    want_hit[i] = hit ? 1 : 0;
    if (hit) {
      want[i] = isect;
      hit2++;
      if (isect.prim_id == ids[i]) unpeeled++;  // (never: the skipped triangle cannot be reported)
    }
  }
#ifdef NANORT_USE_HIP_BACKEND
  if (!accel.TraverseBatch(&rays[0], n, &got[0], &got_hit[0], base, &ids[0])) {
    std::printf("TraverseBatch failed: %s\n", accel.LastBackendError().c_str());
    return 1;
  }
  if (!accel.OccludedBatch(&rays[0], n, &got_occ[0], base, &ids[0])) {
    std::printf("OccludedBatch failed: %s\n", accel.LastBackendError().c_str());
    return 1;
  }
  // ... and the call without the array is the call as it always was
  std::vector<nanort::TriangleIntersection<real> > plain(n), plain_null(n);
  std::vector<unsigned char> plain_hit(n), plain_null_hit(n);
  std::memset(static_cast<void *>(&plain[0]), 0xAB, n * sizeof(plain[0]));
  std::memset(static_cast<void *>(&plain_null[0]), 0xAB, n * sizeof(plain_null[0]));
  if (!accel.TraverseBatch(&rays[0], n, &plain[0], &plain_hit[0]) || !accel.TraverseBatch(&rays[0], n, &plain_null[0], &plain_null_hit[0], base, NULL)) {
    std::printf("TraverseBatch failed: %s\n", accel.LastBackendError().c_str());
    return 1;
  }
  const bool null_same = std::memcmp(&plain[0], &plain_null[0], n * sizeof(plain[0])) == 0 && plain_hit == plain_null_hit;
  std::printf("null_array_same %d\n", null_same ? 1 : 0);
#else
  if (!accel.TraverseBatch(&rays[0], n, isector, &got[0], &got_hit[0], base, &ids[0])) {
    std::printf("TraverseBatch (host) failed\n");
    return 1;
  }
  got_occ = want_hit;
#endif
  size_t bad = 0, bad_occ = 0;
  for (size_t i = 0; i < n; i++) {
    if (got_hit[i] != want_hit[i] || std::memcmp(&got[i], &want[i], sizeof(got[i])) != 0) bad++;  // (a miss leaves the 0xAB pattern on both sides)
    if (got_occ[i] != want_hit[i]) bad_occ++;
  }
  std::printf("rays %zu faces %u wave1_hits %zu wave2_hits %zu\n", n, nfaces, hit1, hit2);
  std::printf("batch_vs_per_ray_mismatches %zu\n", bad);
  std::printf("occluded_vs_per_ray_mismatches %zu\n", bad_occ);
  std::printf("skipped_triangle_reported %zu\n", unpeeled);
  return (bad || bad_occ || unpeeled) ? 2 : 0;
}

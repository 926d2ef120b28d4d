// tests/cpp/masks_check.cc — include/nanort.h's visibility masks WITH the HIP backend (tests/test_gpu_masks.py): Build() over
// (TriangleMesh, TriangleSAHPred) runs on the GPU; after SetPrimMasks(), TraverseBatchMasked() / OccludedBatchMasked() must equal the
// header's own per-ray Traverse() with a MaskedTriangleIntersector set to each ray's mask, over the read-back tree, byte for byte.
// Then the masks change with no Build(): the same again.  A copy made before that change keeps the first masks (copy-on-write);
// an accel without masks refuses; removed masks refuse.
//
//   masks_check <f32|f64> mesh.bin rays.bin range0 range1 skip cull
//   mesh.bin: u32 nv, u32 nf, T v[nv][3], u32 faces[nf][3], u32 masks_a[nf], u32 masks_b[nf]
//   rays.bin: u64 n, Ray<T> rays[n], u32 ray_masks[n]
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

// The batch calls of `accel` against its own per-ray walk with the filter over `prim_masks`; the hits, or -1.
template <typename T>
static long check(const char *what, const nanort::BVHAccel<T> &accel, const nanort::TriangleMesh<T> &mesh, const unsigned int *prim_masks,
                  const std::vector<nanort::Ray<T> > &rays, const std::vector<unsigned int> &ray_masks, const nanort::BVHTraceOptions &opt) {
  const size_t n = rays.size();
  std::vector<nanort::TriangleIntersection<T> > batch(n);
  std::vector<unsigned char> flags(n, 9), occ(n, 9);
  memset(batch.data(), 0xAB, batch.size() * sizeof(batch[0]));
  if (!accel.TraverseBatchMasked(rays.data(), ray_masks.data(), n, batch.data(), flags.data(), opt) ||
      !accel.OccludedBatchMasked(rays.data(), ray_masks.data(), n, occ.data(), opt)) {
    fprintf(stderr, "%s: masked batch call failed: %s\n", what, accel.LastBackendError().c_str());
    return -1;
  }
  nanort::MaskedTriangleIntersector<T> isector(mesh, prim_masks);
  long hits = 0;
  for (size_t i = 0; i < n; i++) {
    nanort::TriangleIntersection<T> h;
    h.u = h.v = T(0);
    h.t = rays[i].max_t;
    h.prim_id = 0xFFFFFFFFu;
    isector.SetRayMask(ray_masks[i]);
    const unsigned char hit = accel.Traverse(rays[i], isector, &h, opt) ? 1 : 0;
    hits += hit;
    if (flags[i] != hit || occ[i] != hit || !same_record(h, batch[i])) {
      fprintf(stderr, "%s: ray %zu (mask %08x): host hit %d t %.9g prim %u, batch flag %d occluded %d t %.9g prim %u\n", what, i, ray_masks[i], hit,
              (double)h.t, h.prim_id, flags[i], occ[i], (double)batch[i].t, batch[i].prim_id);
      return -1;
    }
  }
  return hits;
}

template <typename T>
static int run(char **argv) {
  FILE *fp = fopen(argv[2], "rb");
  if (!fp) return 2;
  uint32_t nv = 0, nf = 0;
  if (!read_exact(fp, &nv, 1) || !read_exact(fp, &nf, 1)) return 2;
  std::vector<T> v(3 * (size_t)nv);
  std::vector<unsigned int> faces(3 * (size_t)nf), masks_a((size_t)nf), masks_b((size_t)nf);
  if (!read_exact(fp, v.data(), v.size()) || !read_exact(fp, faces.data(), faces.size()) || !read_exact(fp, masks_a.data(), masks_a.size()) ||
      !read_exact(fp, masks_b.data(), masks_b.size()))
    return 2;
  fclose(fp);
  fp = fopen(argv[3], "rb");
  if (!fp) return 2;
  uint64_t n64 = 0;
  if (!read_exact(fp, &n64, 1)) return 2;
  const size_t n = (size_t)n64;
  std::vector<nanort::Ray<T> > rays(n);
  std::vector<unsigned int> ray_masks(n);
  if (!read_exact(fp, rays.data(), rays.size()) || !read_exact(fp, ray_masks.data(), ray_masks.size())) return 2;
  fclose(fp);

  nanort::BVHTraceOptions opt;
  opt.prim_ids_range[0] = (unsigned int)strtoul(argv[4], NULL, 10);
  opt.prim_ids_range[1] = (unsigned int)strtoul(argv[5], NULL, 10);
  opt.skip_prim_id = (unsigned int)strtoul(argv[6], NULL, 10);
  opt.cull_back_face = atoi(argv[7]) != 0;

  const size_t stride = 3 * sizeof(T);
  nanort::TriangleMesh<T> mesh(v.data(), faces.data(), stride);
  nanort::TriangleSAHPred<T> pred(v.data(), faces.data(), stride);
  nanort::BVHAccel<T> accel;
  if (!accel.Build(nf, mesh, pred)) {
    fprintf(stderr, "Build failed: %s\n", accel.LastBackendError().c_str());
    return 1;
  }
  std::vector<unsigned char> occ(n, 9);
  // no masks yet: refused with a reason
  if (accel.OccludedBatchMasked(rays.data(), ray_masks.data(), n, occ.data(), opt) || accel.LastBackendError().empty()) {
    fprintf(stderr, "a masked query on an accel without masks did not refuse\n");
    return 1;
  }
  // a wrong count is refused
  if (accel.SetPrimMasks(masks_a.data(), nf + 1) || accel.LastBackendError().empty()) {
    fprintf(stderr, "SetPrimMasks with a wrong count did not refuse\n");
    return 1;
  }
  if (!accel.SetPrimMasks(masks_a.data(), nf)) {
    fprintf(stderr, "SetPrimMasks failed: %s\n", accel.LastBackendError().c_str());
    return 1;
  }
  const long hits_a = check<T>("masks a", accel, mesh, masks_a.data(), rays, ray_masks, opt);
  if (hits_a < 0) return 1;

  // a copy shares the context; the original then changes its masks with no Build(): the copy keeps the first ones
  nanort::BVHAccel<T> copy(accel);
  if (!accel.SetPrimMasks(masks_b.data(), nf)) {
    fprintf(stderr, "SetPrimMasks (second) failed: %s\n", accel.LastBackendError().c_str());
    return 1;
  }
  const long hits_b = check<T>("masks b", accel, mesh, masks_b.data(), rays, ray_masks, opt);
  if (hits_b < 0) return 1;
  if (check<T>("the copy, masks a", copy, mesh, masks_a.data(), rays, ray_masks, opt) != hits_a) return 1;

  // the plain batch call on the same accel ignores the masks
  {
    nanort::TriangleIntersector<T> plain(v.data(), faces.data(), stride);
    std::vector<nanort::TriangleIntersection<T> > tb(n);
    std::vector<unsigned char> tf(n, 9);
    if (!accel.TraverseBatch(rays.data(), n, tb.data(), tf.data(), opt)) {
      fprintf(stderr, "TraverseBatch failed: %s\n", accel.LastBackendError().c_str());
      return 1;
    }
    for (size_t i = 0; i < n; i++) {
      nanort::TriangleIntersection<T> h;
      const bool hit = accel.Traverse(rays[i], plain, &h, opt);
      if (tf[i] != (hit ? 1 : 0) || (hit && !same_record(h, tb[i]))) {
        fprintf(stderr, "plain query, ray %zu: host hit %d, batch flag %d\n", i, (int)hit, tf[i]);
        return 1;
      }
    }
  }

  // removed: refused again
  if (!accel.SetPrimMasks(NULL, 0) || accel.OccludedBatchMasked(rays.data(), ray_masks.data(), n, occ.data(), opt) || accel.LastBackendError().empty()) {
    fprintf(stderr, "a masked query after SetPrimMasks(NULL) did not refuse\n");
    return 1;
  }
  printf("ok %ld %zu\n", hits_a + hits_b, n);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 8) {
    fprintf(stderr, "usage: %s <f32|f64> mesh.bin rays.bin range0 range1 skip cull\n", argv[0]);
    return 1;
  }
  return std::string(argv[1]) == "f64" ? run<double>(argv) : run<float>(argv);
}

// tests/cpp/masks_host_check.cc — include/nanort.h's MaskedTriangleIntersector on the HOST, compiled without NANORT_USE_HIP_BACKEND
// (tests/test_masks_model.py): a tree Load()ed from the file the test wrote (the oracle's), then one Traverse() per ray with the
// intersector set to that ray's mask.  Writes the records, which the test compares with its expectation over the same tree.
//
//   masks_host_check <f32|f64> mesh.bin tree.bin rays.bin out.bin range0 range1 skip cull
//   mesh.bin: u32 nv, u32 nf, T v[nv][3], u32 faces[nf][3], u32 prim_masks[nf]
//   tree.bin: the format of BVHAccel::Dump / Load (size_t count, nodes, size_t count, indices)
//   rays.bin: u64 n, Ray<T> rays[n], u32 ray_masks[n]
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
static int run(char **argv) {
  FILE *fp = fopen(argv[2], "rb");
  if (!fp) return 2;
  uint32_t nv = 0, nf = 0;
  if (!read_exact(fp, &nv, 1) || !read_exact(fp, &nf, 1)) return 2;
  std::vector<T> v(3 * (size_t)nv);
  std::vector<unsigned int> faces(3 * (size_t)nf), prim_masks((size_t)nf);
  if (!read_exact(fp, v.data(), v.size()) || !read_exact(fp, faces.data(), faces.size()) || !read_exact(fp, prim_masks.data(), prim_masks.size())) return 2;
  fclose(fp);
  fp = fopen(argv[4], "rb");
  if (!fp) return 2;
  uint64_t n = 0;
  if (!read_exact(fp, &n, 1)) return 2;
  std::vector<nanort::Ray<T> > rays((size_t)n);
  std::vector<unsigned int> ray_masks((size_t)n);
  if (!read_exact(fp, rays.data(), rays.size()) || !read_exact(fp, ray_masks.data(), ray_masks.size())) return 2;
  fclose(fp);

  nanort::BVHTraceOptions opt;
  opt.prim_ids_range[0] = (unsigned int)strtoul(argv[6], NULL, 10);
  opt.prim_ids_range[1] = (unsigned int)strtoul(argv[7], NULL, 10);
  opt.skip_prim_id = (unsigned int)strtoul(argv[8], NULL, 10);
  opt.cull_back_face = atoi(argv[9]) != 0;

  nanort::BVHAccel<T> accel;
  if (!accel.Load(argv[3])) return 3;

  const size_t stride = 3 * sizeof(T);
  nanort::TriangleMesh<T> mesh(v.data(), faces.data(), stride);
  nanort::MaskedTriangleIntersector<T> isector(mesh, prim_masks.data());
  std::vector<nanort::TriangleIntersection<T> > hits((size_t)n);
  std::vector<unsigned char> mask((size_t)n);
  memset(hits.data(), 0, hits.size() * sizeof(hits[0]));  // (fp64 records: the padding too)
  for (size_t i = 0; i < (size_t)n; i++) {
    nanort::TriangleIntersection<T> &h = hits[i];
    h.u = h.v = T(0);  // the miss record of the batch calls: {0, 0, max_t, 0xFFFFFFFF}
    h.t = rays[i].max_t;
    h.prim_id = 0xFFFFFFFFu;
    isector.SetRayMask(ray_masks[i]);
    mask[i] = accel.Traverse(rays[i], isector, &h, opt) ? 1 : 0;
  }

  fp = fopen(argv[5], "wb");
  if (!fp) return 2;
  fwrite(hits.data(), sizeof(hits[0]), hits.size(), fp);
  fwrite(mask.data(), 1, mask.size(), fp);
  fclose(fp);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 10) {
    fprintf(stderr, "usage: %s <f32|f64> mesh.bin tree.bin rays.bin out.bin range0 range1 skip cull\n", argv[0]);
    return 1;
  }
  return std::string(argv[1]) == "f64" ? run<double>(argv) : run<float>(argv);
}

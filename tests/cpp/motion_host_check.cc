// tests/cpp/motion_host_check.cc — include/nanort.h's motion-blur classes on the HOST, compiled without NANORT_USE_HIP_BACKEND
// (tests/test_motion_model.py): Build() over (MotionTriangleMesh, MotionTriangleSAHPred), then one Traverse() per ray with the
// MotionTriangleIntersector set to that ray's time.  Writes the header's own tree and the records, which the test compares with
// oracle.traverse over the same tree and numpy-interpolated vertices.
//
//   motion_host_check <f32|f64> mesh.bin rays.bin out.bin range0 range1 skip cull [min_leaf]
//   mesh.bin: u32 nv, u32 nf, T v0[nv][3], T v1[nv][3], u32 faces[nf][3]
//   rays.bin: u64 n, Ray<T> rays[n], T times[n]
//   out.bin:  u64 num_nodes, u64 num_indices, BVHNode<T> nodes[], u32 indices[], TriangleIntersection<T> hits[n], u8 mask[n]
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
static int run(int argc, char **argv) {
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
  uint64_t n = 0;
  if (!read_exact(fp, &n, 1)) return 2;
  std::vector<nanort::Ray<T> > rays((size_t)n);
  std::vector<T> times((size_t)n);
  if (!read_exact(fp, rays.data(), rays.size()) || !read_exact(fp, times.data(), times.size())) return 2;
  fclose(fp);

  nanort::BVHTraceOptions opt;
  opt.prim_ids_range[0] = (unsigned int)strtoul(argv[5], NULL, 10);
  opt.prim_ids_range[1] = (unsigned int)strtoul(argv[6], NULL, 10);
  opt.skip_prim_id = (unsigned int)strtoul(argv[7], NULL, 10);
  opt.cull_back_face = atoi(argv[8]) != 0;
  nanort::BVHBuildOptions<T> bo;
  if (argc > 9) bo.min_leaf_primitives = (unsigned int)atoi(argv[9]);

  const size_t stride = 3 * sizeof(T);
  nanort::MotionTriangleMesh<T> mesh(v0.data(), v1.data(), faces.data(), stride);
  nanort::MotionTriangleSAHPred<T> pred(v0.data(), v1.data(), faces.data(), stride);
  nanort::BVHAccel<T> accel;
  if (!accel.Build(nf, mesh, pred, bo)) return 3;

  nanort::MotionTriangleIntersector<T> isector(mesh);
  std::vector<nanort::TriangleIntersection<T> > hits((size_t)n);
  std::vector<unsigned char> mask((size_t)n);
  memset(hits.data(), 0, hits.size() * sizeof(hits[0]));  // (fp64 records: the padding too)
  for (size_t i = 0; i < (size_t)n; i++) {
    nanort::TriangleIntersection<T> &h = hits[i];
    h.u = h.v = T(0);  // the miss record of the batch calls: {0, 0, max_t, 0xFFFFFFFF}
    h.t = rays[i].max_t;
    h.prim_id = 0xFFFFFFFFu;
    isector.SetTime(times[i]);
    mask[i] = accel.Traverse(rays[i], isector, &h, opt) ? 1 : 0;
  }

  const std::vector<nanort::BVHNode<T> > &nodes = accel.GetNodes();
  const std::vector<unsigned int> &idx = accel.GetIndices();
  fp = fopen(argv[4], "wb");
  if (!fp) return 2;
  const uint64_t nn = nodes.size(), ni = idx.size();
  fwrite(&nn, 8, 1, fp);
  fwrite(&ni, 8, 1, fp);
  fwrite(nodes.data(), sizeof(nodes[0]), nodes.size(), fp);
  fwrite(idx.data(), 4, idx.size(), fp);
  fwrite(hits.data(), sizeof(hits[0]), hits.size(), fp);
  fwrite(mask.data(), 1, mask.size(), fp);
  fclose(fp);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 9) {
    fprintf(stderr, "usage: %s <f32|f64> mesh.bin rays.bin out.bin range0 range1 skip cull [min_leaf]\n", argv[0]);
    return 1;
  }
  return std::string(argv[1]) == "f64" ? run<double>(argc, argv) : run<float>(argc, argv);
}

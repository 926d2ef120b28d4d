// tests/cpp/curves_check.cc — the built-in curve primitive of include/nanort.h (BezierCurvePred / BezierCurveGeometry /
// BezierCurveIntersection / BezierCurveIntersector), on the host and, compiled with -DNANORT_USE_HIP_BACKEND, on the GPU.
//
//   curves_check layout
//       prints sizeof and the member offsets of BezierCurveIntersection and of nrt_curve_hit_f32, one line each
//   curves_check run <curves.bin> <rays.bin> <num_subdivisions> <out.bin>
//       curves.bin: u32 n, n * 12 floats, n * 4 floats; rays.bin: u64 m, m rays.  Build() over the pair, then per ray the host
//       Traverse() with the built-in intersector; out.bin: u64 num_nodes, u64 num_indices, nodes, indices, m records (40 B),
//       m flags.  With the backend macro Build() runs on the GPU, the tree is the one read back from it, and the program
//       first checks that TraverseBatch(BezierCurveIntersection*) gives the bytes of the per-ray loop, that a second call with
//       another subdivision count and back gives them again, and that Refit() refuses.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nanort.h"
#include "nanort_hip.h"

typedef nanort::BezierCurveIntersection Hit;

static bool read_all(const char *path, std::vector<char> *buf) {
  FILE *fp = fopen(path, "rb");
  if (!fp) return false;
  fseek(fp, 0, SEEK_END);
  const long n = ftell(fp);
  fseek(fp, 0, SEEK_SET);
  buf->resize(static_cast<size_t>(n));
  const bool ok = n == 0 || fread(&(*buf)[0], 1, static_cast<size_t>(n), fp) == static_cast<size_t>(n);
  fclose(fp);
  return ok;
}

static void host_loop(const nanort::BVHAccel<float> &accel, const float *cps, const float *radii, int subdiv, const nanort::Ray<float> *rays,
                      size_t m, std::vector<Hit> *hits, std::vector<unsigned char> *mask) {
  hits->assign(m, Hit());
  mask->assign(m, 0);
  for (size_t i = 0; i < m; i++) {
    nanort::BezierCurveIntersector<> isector(cps, radii, subdiv);
    (*mask)[i] = accel.Traverse(rays[i], isector, &(*hits)[i]) ? 1 : 0;
  }
}

int main(int argc, char **argv) {
  if (argc >= 2 && std::strcmp(argv[1], "layout") == 0) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(Hit), offsetof(Hit, t), offsetof(Hit, prim_id), offsetof(Hit, u), offsetof(Hit, v),
           offsetof(Hit, tangent), offsetof(Hit, normal));
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(nrt_curve_hit_f32), offsetof(nrt_curve_hit_f32, t), offsetof(nrt_curve_hit_f32, prim_id),
           offsetof(nrt_curve_hit_f32, u), offsetof(nrt_curve_hit_f32, v), offsetof(nrt_curve_hit_f32, tangent), offsetof(nrt_curve_hit_f32, normal));
    return 0;
  }
  if (argc != 6 || std::strcmp(argv[1], "run") != 0) {
    fprintf(stderr, "usage: curves_check layout | run <curves.bin> <rays.bin> <num_subdivisions> <out.bin>\n");
    return 2;
  }
  std::vector<char> cb, rb;
  if (!read_all(argv[2], &cb) || !read_all(argv[3], &rb) || cb.size() < 4 || rb.size() < 8) {
    fprintf(stderr, "cannot read the inputs\n");
    return 2;
  }
  unsigned int n = 0;
  unsigned long long m64 = 0;
  std::memcpy(&n, &cb[0], 4);
  std::memcpy(&m64, &rb[0], 8);
  const size_t m = static_cast<size_t>(m64);
  if (cb.size() != 4 + static_cast<size_t>(n) * 64 || rb.size() != 8 + m * sizeof(nanort::Ray<float>)) {
    fprintf(stderr, "input sizes do not match their counts\n");
    return 2;
  }
  std::vector<float> cps(12 * static_cast<size_t>(n)), radii(4 * static_cast<size_t>(n));
  std::memcpy(cps.data(), &cb[4], cps.size() * sizeof(float));
  std::memcpy(radii.data(), &cb[4 + cps.size() * sizeof(float)], radii.size() * sizeof(float));
  std::vector<nanort::Ray<float> > rays(m);
  if (m) std::memcpy(static_cast<void *>(&rays[0]), &rb[8], m * sizeof(nanort::Ray<float>));
  const int subdiv = atoi(argv[4]);

  nanort::BezierCurveGeometry geom(cps.data(), radii.data());
  nanort::BezierCurvePred pred(cps.data());
  nanort::BVHAccel<float> accel;
  nanort::BVHBuildOptions<float> options;
  options.cache_bbox = false;
  if (!accel.Build(n, geom, pred, options)) {
    fprintf(stderr, "Build() failed\n");
    return 1;
  }
  std::vector<Hit> hits;
  std::vector<unsigned char> mask;
  host_loop(accel, cps.data(), radii.data(), subdiv, m ? &rays[0] : NULL, m, &hits, &mask);

#ifdef NANORT_USE_HIP_BACKEND
  if (accel.NumHipDevices() == 0) {
    fprintf(stderr, "Build() did not go to the GPU: %s\n", accel.LastBackendError().c_str());
    return 1;
  }
  const int other = subdiv == 4 ? 7 : 4;
  const int order[3] = {subdiv, other, subdiv};
  for (int pass = 0; pass < 3; pass++) {
    std::vector<Hit> bh(m);
    std::vector<unsigned char> bm(m, 2);
    if (!accel.TraverseBatch(m ? &rays[0] : NULL, m, m ? &bh[0] : NULL, m ? &bm[0] : NULL, nanort::BVHTraceOptions(), order[pass])) {
      fprintf(stderr, "TraverseBatch failed: %s\n", accel.LastBackendError().c_str());
      return 1;
    }
    std::vector<Hit> hh;
    std::vector<unsigned char> hm;
    host_loop(accel, cps.data(), radii.data(), order[pass], m ? &rays[0] : NULL, m, &hh, &hm);
    if (m && (std::memcmp(&bm[0], &hm[0], m) != 0 || std::memcmp(static_cast<const void *>(&bh[0]), static_cast<const void *>(&hh[0]), m * sizeof(Hit)) != 0)) {
      fprintf(stderr, "pass %d (num_subdivisions %d): the batch differs from the per-ray host loop\n", pass, order[pass]);
      return 1;
    }
  }
  if (accel.Refit(geom) || accel.LastBackendError().find("curve") == std::string::npos) {
    fprintf(stderr, "Refit() over curves did not refuse with its message\n");
    return 1;
  }
#endif

  FILE *fp = fopen(argv[5], "wb");
  if (!fp) return 2;
  const unsigned long long nn = accel.GetNodes().size(), ni = accel.GetIndices().size();
  fwrite(&nn, 8, 1, fp);
  fwrite(&ni, 8, 1, fp);
  fwrite(&accel.GetNodes()[0], sizeof(nanort::BVHNode<float>), nn, fp);
  fwrite(&accel.GetIndices()[0], 4, ni, fp);
  if (m) {
    fwrite(static_cast<const void *>(&hits[0]), sizeof(Hit), m, fp);
    fwrite(&mask[0], 1, m, fp);
  }
  fclose(fp);
  return 0;
}

// tests/cpp/multihit_check.cc — include/nanort.h's multi-hit traversal from a C++ program (tests/test_multihit_model.py,
// tests/test_gpu_multihit.py).
//
//   multihit_check mesh.bin rays.bin K out.bin [batch]
// mesh.bin: u32 nv, u32 nf, float xyz[nv], u32 faces[nf][3]; rays.bin: u64 n, Ray<float>[n].
// Builds the BVH (on the GPU when compiled with -DNANORT_USE_HIP_BACKEND), runs MultiHitTraverse per ray and writes
//   u32 counts[n], TriangleIntersection<float> rows[n][K] (miss records {0, 0, max_t, 0xFFFFFFFF} after the held hits),
//   u64 num_nodes, BVHNode<float> nodes[], u32 indices[nf];
// with `batch` (backend builds only), MultiHitTraverseBatch's counts and rows follow.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nanort.h"

template <class V>
static bool read_exact(FILE *f, V *p, size_t n) {
  return fread(p, sizeof(V), n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: multihit_check mesh.bin rays.bin K out.bin [batch]\n");
    return 2;
  }
  FILE *fm = fopen(argv[1], "rb");
  FILE *fr = fopen(argv[2], "rb");
  if (!fm || !fr) return 2;
  uint32_t nv = 0, nf = 0;
  uint64_t n = 0;
  if (!read_exact(fm, &nv, 1) || !read_exact(fm, &nf, 1)) return 2;
  std::vector<float> verts(3 * (size_t)nv);
  std::vector<unsigned int> faces(3 * (size_t)nf);
  if (!read_exact(fm, verts.data(), verts.size()) || !read_exact(fm, faces.data(), faces.size())) return 2;
  if (!read_exact(fr, &n, 1)) return 2;
  std::vector<nanort::Ray<float> > rays((size_t)n);
  if (!read_exact(fr, rays.data(), rays.size())) return 2;
  fclose(fm);
  fclose(fr);
  const unsigned int K = (unsigned int)atoi(argv[3]);

  nanort::TriangleMesh<float> mesh(verts.data(), faces.data(), sizeof(float) * 3);
  nanort::TriangleSAHPred<float> pred(verts.data(), faces.data(), sizeof(float) * 3);
  nanort::BVHAccel<float> accel;
  if (!accel.Build(nf, mesh, pred, nanort::BVHBuildOptions<float>())) return 3;

  nanort::TriangleIntersector<float, nanort::TriangleIntersection<float> > isector(verts.data(), faces.data(), sizeof(float) * 3);
  std::vector<uint32_t> counts((size_t)n);
  std::vector<nanort::TriangleIntersection<float> > rows((size_t)n * K);
  for (size_t i = 0; i < (size_t)n; i++) {
    nanort::StackVector<nanort::TriangleIntersection<float>, 128> held;
    accel.MultiHitTraverse(rays[i], (int)K, isector, &held);
    counts[i] = (uint32_t)held->size();
    for (unsigned int j = 0; j < K; j++) {
      nanort::TriangleIntersection<float> &h = rows[i * K + j];
      if (j < held->size()) {
        h = held[j];
      } else {
        h.u = 0.0f;
        h.v = 0.0f;
        h.t = rays[i].max_t;
        h.prim_id = 0xFFFFFFFFu;
      }
    }
  }
  FILE *fo = fopen(argv[4], "wb");
  if (!fo) return 2;
  fwrite(counts.data(), sizeof(uint32_t), counts.size(), fo);
  fwrite(rows.data(), sizeof(rows[0]), rows.size(), fo);
  const std::vector<nanort::BVHNode<float> > &nodes = accel.GetNodes();
  const uint64_t nn = nodes.size();
  fwrite(&nn, sizeof(nn), 1, fo);
  fwrite(nodes.data(), sizeof(nodes[0]), nodes.size(), fo);
  fwrite(accel.GetIndices().data(), sizeof(unsigned int), accel.GetIndices().size(), fo);
#ifdef NANORT_USE_HIP_BACKEND
  if (argc > 5) {
    std::vector<unsigned int> bcounts((size_t)n);
    std::vector<nanort::TriangleIntersection<float> > brows((size_t)n * K);
    if (!accel.MultiHitTraverseBatch(rays.data(), (size_t)n, K, brows.data(), bcounts.data())) {
      fprintf(stderr, "MultiHitTraverseBatch: %s\n", accel.LastBackendError().c_str());
      return 4;
    }
    fwrite(bcounts.data(), sizeof(unsigned int), bcounts.size(), fo);
    fwrite(brows.data(), sizeof(brows[0]), brows.size(), fo);
  }
#endif
  fclose(fo);
  return 0;
}

// tests/cpp/refit_host_check.cc — BVHAccel::Refit of include/nanort.h on the host (no backend; tests/test_host_refit.py).
//
//   refit_host_check f32|f64 mesh0.bin mesh1.bin rays.bin out.bin
// mesh*.bin: u32 nv, u32 nf, float xyz[nv], u32 faces[nf][3] (the same faces in both); rays.bin: u64 n, Ray<float>[n].
// f64 widens vertices and rays.  Builds on mesh0, refits to mesh1's vertices, runs Traverse per ray on the refit tree and
// writes u64 num_nodes, BVHNode<T> before[num_nodes], BVHNode<T> after[num_nodes], u32 indices[nf],
// TriangleIntersection<T> hits[n] (a miss keeps {0, 0, 0, 0}), u8 mask[n].
//   refit_host_check malformed mesh0.bin
// (needs -DNANORT_ENABLE_SERIALIZATION) Builds on mesh0, Dump()s the tree, points the last branch's high child back at the
// root (a record reached twice), Load()s it: Refit must return false and leave every node byte as it was.  Prints `ok`.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "nanort.h"

namespace {

bool read_mesh(const char *path, std::vector<float> *v, std::vector<unsigned int> *f) {
  FILE *fp = fopen(path, "rb");
  if (!fp) return false;
  uint32_t nv = 0, nf = 0;
  bool ok = fread(&nv, 4, 1, fp) == 1 && fread(&nf, 4, 1, fp) == 1;
  v->resize(3 * (size_t)nv);
  f->resize(3 * (size_t)nf);
  ok = ok && fread(v->data(), 4, v->size(), fp) == v->size() && fread(f->data(), 4, f->size(), fp) == f->size();
  fclose(fp);
  return ok;
}

template <typename T>
int run(const char **argv) {
  std::vector<float> v0f, v1f;
  std::vector<unsigned int> f0, f1;
  if (!read_mesh(argv[2], &v0f, &f0) || !read_mesh(argv[3], &v1f, &f1) || f0 != f1 || v0f.size() != v1f.size()) return 2;
  std::vector<T> v0(v0f.begin(), v0f.end()), v1(v1f.begin(), v1f.end());
  FILE *fr = fopen(argv[4], "rb");
  if (!fr) return 2;
  uint64_t n = 0;
  if (fread(&n, 8, 1, fr) != 1) return 2;
  std::vector<nanort::Ray<float> > rf((size_t)n);
  if (fread(rf.data(), sizeof(nanort::Ray<float>), rf.size(), fr) != rf.size()) return 2;
  fclose(fr);
  std::vector<nanort::Ray<T> > rays((size_t)n);
  for (size_t i = 0; i < rays.size(); i++) {
    for (int k = 0; k < 3; k++) {
      rays[i].org[k] = rf[i].org[k];
      rays[i].dir[k] = rf[i].dir[k];
    }
    rays[i].min_t = rf[i].min_t;
    rays[i].max_t = rf[i].max_t;
    rays[i].type = rf[i].type;
  }
  const unsigned int nf = static_cast<unsigned int>(f0.size() / 3);
  nanort::BVHAccel<T> accel;
  nanort::TriangleMesh<T> m0(v0.data(), f0.data(), 3 * sizeof(T)), m1(v1.data(), f0.data(), 3 * sizeof(T));
  nanort::TriangleSAHPred<T> pred(v0.data(), f0.data(), 3 * sizeof(T));
  if (!accel.Build(nf, m0, pred)) return 3;
  const std::vector<nanort::BVHNode<T> > before = accel.GetNodes();
  if (!accel.Refit(m1)) return 4;
  const std::vector<nanort::BVHNode<T> > &after = accel.GetNodes();
  const std::vector<unsigned int> &idx = accel.GetIndices();
  nanort::TriangleIntersector<T> isect(v1.data(), f0.data(), 3 * sizeof(T));
  std::vector<nanort::TriangleIntersection<T> > hits((size_t)n);
  std::vector<unsigned char> mask((size_t)n);
  for (size_t i = 0; i < rays.size(); i++) {
    memset(static_cast<void *>(&hits[i]), 0, sizeof(hits[i]));
    mask[i] = accel.Traverse(rays[i], isect, &hits[i]) ? 1 : 0;
  }
  FILE *fo = fopen(argv[5], "wb");
  if (!fo) return 2;
  const uint64_t nn = before.size();
  fwrite(&nn, 8, 1, fo);
  fwrite(before.data(), sizeof(nanort::BVHNode<T>), nn, fo);
  fwrite(after.data(), sizeof(nanort::BVHNode<T>), after.size(), fo);
  fwrite(idx.data(), 4, idx.size(), fo);
  fwrite(hits.data(), sizeof(nanort::TriangleIntersection<T>), hits.size(), fo);
  fwrite(mask.data(), 1, mask.size(), fo);
  fclose(fo);
  return after.size() == nn ? 0 : 5;
}

#if defined(NANORT_ENABLE_SERIALIZATION)
int malformed(const char *mesh) {
  std::vector<float> v;
  std::vector<unsigned int> f;
  if (!read_mesh(mesh, &v, &f)) return 2;
  nanort::BVHAccel<float> accel;
  nanort::TriangleMesh<float> m(v.data(), f.data(), 12);
  if (!accel.Build(static_cast<unsigned int>(f.size() / 3), m, nanort::TriangleSAHPred<float>(v.data(), f.data(), 12))) return 3;
  std::vector<nanort::BVHNode<float> > nodes = accel.GetNodes();
  const std::vector<unsigned int> idx = accel.GetIndices();
  size_t last = nodes.size();
  for (size_t i = 0; i < nodes.size(); i++)
    if (nodes[i].flag == 0) last = i;
  if (last == nodes.size()) return 3;
  nodes[last].data[1] = 0;  // the root again: reached twice
  FILE *fp = tmpfile();
  if (!fp) return 2;
  const size_t nn = nodes.size(), ni = idx.size();
  fwrite(&nn, sizeof(size_t), 1, fp);
  fwrite(nodes.data(), sizeof(nodes[0]), nn, fp);
  fwrite(&ni, sizeof(size_t), 1, fp);
  fwrite(idx.data(), 4, ni, fp);
  rewind(fp);
  nanort::BVHAccel<float> bad;
  const bool loaded = bad.Load(fp);
  fclose(fp);
  if (!loaded) return 4;
  const std::vector<nanort::BVHNode<float> > before = bad.GetNodes();
  if (bad.Refit(m)) return 5;
  const std::vector<nanort::BVHNode<float> > &after = bad.GetNodes();
  if (after.size() != before.size() || memcmp(after.data(), before.data(), before.size() * sizeof(before[0])) != 0) return 6;
  printf("ok\n");
  return 0;
}
#endif

}  // namespace

int main(int argc, char **argv) {
#if defined(NANORT_ENABLE_SERIALIZATION)
  if (argc == 3 && std::string(argv[1]) == "malformed") return malformed(argv[2]);
#endif
  if (argc != 6) {
    fprintf(stderr, "usage: refit_host_check f32|f64 mesh0.bin mesh1.bin rays.bin out.bin\n");
    return 2;
  }
  const char **a = const_cast<const char **>(argv);
  return std::string(argv[1]) == "f64" ? run<double>(a) : run<float>(a);
}

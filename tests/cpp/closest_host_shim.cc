// tests/cpp/closest_host_shim.cc — include/nanort.h's closest-point query on the HOST, compiled without NANORT_USE_HIP_BACKEND as a
// shared library (tests/closest_fixture.py): Build() over (TriangleMesh, TriangleSAHPred), the header's own tree, and
// BVHAccel<T>::ClosestPointBatch() — which, without the backend, is the loop over the header's host walk ClosestPoint().
#include <cstdint>
#include <cstring>
#include <vector>

#include "nanort.h"

namespace {

template <typename T>
struct Handle {
  std::vector<T> verts;
  std::vector<unsigned int> faces;
  nanort::BVHAccel<T> accel;
};

template <typename T>
void *create(const T *verts, uint32_t nv, const uint32_t *faces, uint32_t nf) {
  Handle<T> *h = new Handle<T>;
  h->verts.assign(verts, verts + 3 * (size_t)nv);
  h->faces.assign(faces, faces + 3 * (size_t)nf);
  nanort::TriangleMesh<T> mesh(h->verts.data(), h->faces.data(), 3 * sizeof(T));
  nanort::TriangleSAHPred<T> pred(h->verts.data(), h->faces.data(), 3 * sizeof(T));
  if (!h->accel.Build(nf, mesh, pred, nanort::BVHBuildOptions<T>())) {
    delete h;
    return nullptr;
  }
  return h;
}

template <typename T>
void sizes(void *hv, uint64_t *out2) {
  Handle<T> *h = (Handle<T> *)hv;
  out2[0] = h->accel.GetNodes().size();
  out2[1] = h->accel.GetIndices().size();
}

template <typename T>
void tree(void *hv, void *nodes, uint32_t *indices) {
  Handle<T> *h = (Handle<T> *)hv;
  static_assert(sizeof(nanort::BVHNode<T>) == (sizeof(T) == 4 ? 40 : 64), "BVHNode layout");
  memcpy(nodes, h->accel.GetNodes().data(), h->accel.GetNodes().size() * sizeof(nanort::BVHNode<T>));
  memcpy(indices, h->accel.GetIndices().data(), h->accel.GetIndices().size() * sizeof(uint32_t));
}

// points: {T p[3], max_dist} per point; out: ClosestPointResult<T> records (the library's layout)
template <typename T>
int closest(void *hv, const T *points4, uint64_t n, const uint32_t *opt3, void *out, uint8_t *found) {
  Handle<T> *h = (Handle<T> *)hv;
  static_assert(sizeof(nanort::ClosestPointResult<T>) == (sizeof(T) == 4 ? 32 : 56), "ClosestPointResult layout");
  std::vector<T> xyz(3 * (size_t)n), md((size_t)n);
  for (uint64_t i = 0; i < n; i++) {
    for (int k = 0; k < 3; k++) xyz[3 * i + k] = points4[4 * i + k];
    md[i] = points4[4 * i + 3];
  }
  nanort::BVHTraceOptions opt;
  opt.prim_ids_range[0] = opt3[0];
  opt.prim_ids_range[1] = opt3[1];
  opt.skip_prim_id = opt3[2];
  nanort::TriangleMesh<T> mesh(h->verts.data(), h->faces.data(), 3 * sizeof(T));
  return h->accel.ClosestPointBatch(xyz.data(), md.data(), (size_t)n, mesh, (nanort::ClosestPointResult<T> *)out, found, opt) ? 0 : 1;
}

} // namespace

#define CHS_EXPORTS(T, S)                                                                                                   \
  void *chs_create_##S(const T *verts, uint32_t nv, const uint32_t *faces, uint32_t nf) { return create<T>(verts, nv, faces, nf); } \
  void chs_sizes_##S(void *h, uint64_t *out2) { sizes<T>(h, out2); }                                                        \
  void chs_tree_##S(void *h, void *nodes, uint32_t *indices) { tree<T>(h, nodes, indices); }                                \
  int chs_closest_##S(void *h, const T *points4, uint64_t n, const uint32_t *opt3, void *out, uint8_t *found) {            \
    return closest<T>(h, points4, n, opt3, out, found);                                                                     \
  }                                                                                                                         \
  void chs_destroy_##S(void *h) { delete (Handle<T> *)h; }

extern "C" {
CHS_EXPORTS(float, f32)
CHS_EXPORTS(double, f64)
}

// tests/cpp/nearest_host_shim.cc — include/nanort.h's nearest-faces query on the HOST, compiled without NANORT_USE_HIP_BACKEND as a
// shared library (tests/nearest_fixture.py): Build() over (TriangleMesh, TriangleSAHPred), the header's own tree, and
// BVHAccel<T>::NearestFacesBatch() — which, without the backend, is the loop over the header's host walk NearestFaces().
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

// points: {T p[3], max_dist} per point; out: n * k ClosestPointResult<T> records (the library's layout); counts: n words
template <typename T>
int nearest(void *hv, const T *points4, uint64_t n, uint32_t k, const uint32_t *opt3, void *out, uint32_t *counts) {
  Handle<T> *h = (Handle<T> *)hv;
  static_assert(sizeof(nanort::ClosestPointResult<T>) == (sizeof(T) == 4 ? 32 : 56) && sizeof(unsigned int) == sizeof(uint32_t), "record layout");
  std::vector<T> xyz(3 * (size_t)n), md((size_t)n);
  for (uint64_t i = 0; i < n; i++) {
    for (int j = 0; j < 3; j++) xyz[3 * i + j] = points4[4 * i + j];
    md[i] = points4[4 * i + 3];
  }
  nanort::BVHTraceOptions opt;
  opt.prim_ids_range[0] = opt3[0];
  opt.prim_ids_range[1] = opt3[1];
  opt.skip_prim_id = opt3[2];
  nanort::TriangleMesh<T> mesh(h->verts.data(), h->faces.data(), 3 * sizeof(T));
  return h->accel.NearestFacesBatch(xyz.data(), md.data(), (size_t)n, k, mesh, (nanort::ClosestPointResult<T> *)out, counts, opt) ? 0 : 1;
}

} // namespace

#define NHS_EXPORTS(T, S)                                                                                                           \
  void *nhs_create_##S(const T *verts, uint32_t nv, const uint32_t *faces, uint32_t nf) { return create<T>(verts, nv, faces, nf); } \
  int nhs_nearest_##S(void *h, const T *points4, uint64_t n, uint32_t k, const uint32_t *opt3, void *out, uint32_t *counts) {       \
    return nearest<T>(h, points4, n, k, opt3, out, counts);                                                                         \
  }                                                                                                                                 \
  void nhs_destroy_##S(void *h) { delete (Handle<T> *)h; }

extern "C" {
NHS_EXPORTS(float, f32)
NHS_EXPORTS(double, f64)
}

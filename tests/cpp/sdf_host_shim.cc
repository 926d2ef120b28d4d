// tests/cpp/sdf_host_shim.cc — include/nanort.h's signed distance query on the HOST, compiled without NANORT_USE_HIP_BACKEND as a
// shared library (tests/sdf_fixture.py): Build() over (TriangleMesh, TriangleSAHPred), FeatureNormals<T> of the mesh, and
// BVHAccel<T>::SignedDistanceBatch() — which, without the backend, is the loop over the header's host walk SignedDistance().
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
  nanort::FeatureNormals<T> normals;
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
  h->normals.Build(mesh, nf);
  return h;
}

// sizes2: {num_faces, num_vertices} of the normals; the arrays may be NULL
template <typename T>
void normals(void *hv, uint64_t *sizes2, T *fnormals, T *vnormals) {
  Handle<T> *h = (Handle<T> *)hv;
  sizes2[0] = h->normals.num_faces, sizes2[1] = h->normals.num_vertices;
  if (fnormals) memcpy(fnormals, h->normals.face_normals.data(), h->normals.face_normals.size() * sizeof(T));
  if (vnormals) memcpy(vnormals, h->normals.vertex_normals.data(), h->normals.vertex_normals.size() * sizeof(T));
}

// points: {T p[3], max_dist} per point; out: SignedDistanceResult<T> records (the library's layout)
template <typename T>
int signed_distance(void *hv, const T *points4, uint64_t n, const uint32_t *opt3, void *out, uint8_t *found) {
  Handle<T> *h = (Handle<T> *)hv;
  static_assert(sizeof(nanort::SignedDistanceResult<T>) == (sizeof(T) == 4 ? 32 : 56), "SignedDistanceResult layout");
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
  return h->accel.SignedDistanceBatch(xyz.data(), md.data(), (size_t)n, mesh, h->normals, (nanort::SignedDistanceResult<T> *)out, found, opt) ? 0 : 1;
}

} // namespace

#define SHS_EXPORTS(T, S)                                                                                                   \
  void *shs_create_##S(const T *verts, uint32_t nv, const uint32_t *faces, uint32_t nf) { return create<T>(verts, nv, faces, nf); } \
  void shs_normals_##S(void *h, uint64_t *sizes2, T *fnormals, T *vnormals) { normals<T>(h, sizes2, fnormals, vnormals); }  \
  int shs_signed_##S(void *h, const T *points4, uint64_t n, const uint32_t *opt3, void *out, uint8_t *found) {             \
    return signed_distance<T>(h, points4, n, opt3, out, found);                                                             \
  }                                                                                                                         \
  void shs_destroy_##S(void *h) { delete (Handle<T> *)h; }

extern "C" {
SHS_EXPORTS(float, f32)
SHS_EXPORTS(double, f64)
}

// tests/cpp/refit_check.cc — BVHAccel::Refit of include/nanort.h with the HIP backend (tests/test_gpu_header_refit.py).
//
//   refit_check f32|f64 DIR
// DIR holds mesh0.bin, mesh1.bin, mesh2.bin ({u32 nv, u32 nf, float xyz[nv], u32 faces[nf][3]}, the same faces) and
// rays.bin ({u64 n, Ray<float>[n]}); f64 widens them.  Scenarios:
//   refit    Build on mesh0, copy, Refit to mesh1: the refit object answers on mesh1, the copy still on mesh0's tree;
//   move     a moved-into object refits to mesh2;
//   kinds    sphere and cylinder accels refuse Refit with a reason.
// After every step, every batch method (TraverseBatch, TraverseBatches, OccludedBatch, TraverseBatchDevice,
// MultiHitTraverseBatch at K = 1, 4, 16) must equal the same object's per-ray host walk over the vertices it was last given.
// Prints `devices D checks N mismatches M`; exits 1 on a mismatch.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "nanort.h"
#include <hip/hip_runtime_api.h>

using nanort::BVHAccel;
using nanort::Ray;

namespace {

unsigned long long g_checks = 0, g_bad = 0;

void expect(const char *where, const char *what, bool cond) {
  g_checks++;
  if (!cond) {
    g_bad++;
    fprintf(stderr, "MISMATCH %s: %s\n", where, what);
  }
}

template <typename T>
struct Mesh {
  std::vector<T> v;
  std::vector<unsigned int> f;
  unsigned int nf = 0;
  nanort::TriangleMesh<T> tm() const { return nanort::TriangleMesh<T>(v.data(), f.data(), sizeof(T) * 3); }
  nanort::TriangleSAHPred<T> pred() const { return nanort::TriangleSAHPred<T>(v.data(), f.data(), sizeof(T) * 3); }
};

template <typename T>
bool read_mesh(const std::string &path, Mesh<T> *m) {
  FILE *fp = fopen(path.c_str(), "rb");
  if (!fp) return false;
  uint32_t nv = 0, nf = 0;
  bool ok = fread(&nv, 4, 1, fp) == 1 && fread(&nf, 4, 1, fp) == 1;
  std::vector<float> v(3 * (size_t)nv);
  m->f.resize(3 * (size_t)nf);
  ok = ok && fread(v.data(), 4, v.size(), fp) == v.size() && fread(m->f.data(), 4, m->f.size(), fp) == m->f.size();
  fclose(fp);
  m->v.assign(v.begin(), v.end());
  m->nf = nf;
  return ok;
}

template <typename T>
bool read_rays(const std::string &path, std::vector<Ray<T> > *out) {
  FILE *fp = fopen(path.c_str(), "rb");
  if (!fp) return false;
  uint64_t n = 0;
  bool ok = fread(&n, 8, 1, fp) == 1;
  std::vector<Ray<float> > r((size_t)n);
  ok = ok && fread(r.data(), sizeof(Ray<float>), r.size(), fp) == r.size();
  fclose(fp);
  out->resize(r.size());
  for (size_t i = 0; i < r.size(); i++) {
    for (int k = 0; k < 3; k++) {
      (*out)[i].org[k] = r[i].org[k];
      (*out)[i].dir[k] = r[i].dir[k];
    }
    (*out)[i].min_t = r[i].min_t;
    (*out)[i].max_t = r[i].max_t;
    (*out)[i].type = r[i].type;
  }
  return ok;
}

template <typename T>
void check_tri(const char *where, const BVHAccel<T> &a, const Mesh<T> &m, const std::vector<Ray<T> > &rays) {
  typedef nanort::TriangleIntersection<T> H;
  const size_t n = rays.size();
  std::vector<H> bh(n), wh(n), dh(n);
  std::vector<unsigned char> bm(n, 7), wm(n, 7), wo(n, 7), ob(n, 7), dm(n, 7);
  expect(where, "TraverseBatch", a.TraverseBatch(rays.data(), n, bh.data(), bm.data()));
  const Ray<T> *wr[2] = {rays.data(), rays.data()};
  const size_t wn[2] = {n, n};
  H *wi[2] = {wh.data(), NULL};
  unsigned char *wmk[2] = {wm.data(), wo.data()};
  const unsigned char occ[2] = {0, 1};
  expect(where, "TraverseBatches", a.TraverseBatches(2, wr, wn, wi, wmk, occ));
  expect(where, "OccludedBatch", a.OccludedBatch(rays.data(), n, ob.data()));
  const unsigned int Ks[3] = {1, 4, 16};
  std::vector<H> mh[3];
  std::vector<unsigned int> mc[3];
  for (int k = 0; k < 3; k++) {
    mh[k].resize(n * Ks[k]);
    mc[k].resize(n);
    expect(where, "MultiHitTraverseBatch", a.MultiHitTraverseBatch(rays.data(), n, Ks[k], mh[k].data(), mc[k].data()));
  }
  void *d_rays = NULL, *d_hits = NULL, *d_mask = NULL;
  hipStream_t s;
  if (hipStreamCreate(&s) != hipSuccess || hipMalloc(&d_rays, n * sizeof(Ray<T>)) != hipSuccess || hipMalloc(&d_hits, n * sizeof(H)) != hipSuccess ||
      hipMalloc(&d_mask, n) != hipSuccess)
    exit(3);
  hipMemcpyAsync(d_rays, rays.data(), n * sizeof(Ray<T>), hipMemcpyHostToDevice, s);
  expect(where, "TraverseBatchDevice", a.TraverseBatchDevice(static_cast<const Ray<T> *>(d_rays), n, static_cast<H *>(d_hits),
                                                            static_cast<unsigned char *>(d_mask), s));
  hipMemcpyAsync(dh.data(), d_hits, n * sizeof(H), hipMemcpyDeviceToHost, s);
  hipMemcpyAsync(dm.data(), d_mask, n, hipMemcpyDeviceToHost, s);
  if (hipStreamSynchronize(s) != hipSuccess) exit(3);
  hipFree(d_rays);
  hipFree(d_hits);
  hipFree(d_mask);
  hipStreamDestroy(s);
  // the host walk of the same object over the vertices it was last given
  nanort::TriangleIntersector<T> isect(m.v.data(), m.f.data(), sizeof(T) * 3);
  auto same = [](const H &x, const H &y) { return memcmp(&x.t, &y.t, sizeof(T)) == 0 && x.prim_id == y.prim_id && x.u == y.u && x.v == y.v; };
  unsigned long long bad_b = 0, bad_w = 0, bad_o = 0, bad_d = 0, bad_m = 0, hits = 0;
  for (size_t i = 0; i < n; i++) {
    H hh;
    const unsigned char hm = a.Traverse(rays[i], isect, &hh) ? 1 : 0;
    hits += hm;
    bad_b += bm[i] != hm || (hm && !same(bh[i], hh));
    bad_w += wm[i] != hm || wo[i] != hm || (hm && !same(wh[i], hh));
    bad_o += ob[i] != hm;
    bad_d += dm[i] != hm || (hm && !same(dh[i], hh));
    for (int k = 0; k < 3; k++) {
      nanort::StackVector<H, 128> held;
      a.MultiHitTraverse(rays[i], (int)Ks[k], isect, &held);
      bool good = mc[k][i] == held->size();
      for (unsigned int j = 0; good && j < held->size(); j++) good = same(mh[k][i * Ks[k] + j], held[j]);
      bad_m += !good;
    }
  }
  expect(where, "TraverseBatch == Traverse", bad_b == 0);
  expect(where, "TraverseBatches == Traverse", bad_w == 0);
  expect(where, "OccludedBatch == Traverse", bad_o == 0);
  expect(where, "TraverseBatchDevice == Traverse", bad_d == 0);
  expect(where, "MultiHitTraverseBatch == MultiHitTraverse", bad_m == 0);
  expect(where, "some rays hit", hits > 0);
  if (bad_b + bad_w + bad_o + bad_d + bad_m)
    fprintf(stderr, "%s: batch %llu batches %llu occluded %llu device %llu multihit %llu of %zu\n", where, bad_b, bad_w, bad_o, bad_d, bad_m, n);
}

template <typename T>
bool same_nodes(const std::vector<nanort::BVHNode<T> > &a, const std::vector<nanort::BVHNode<T> > &b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0;
}

template <typename T>
int run(const std::string &dir) {
  Mesh<T> m0, m1, m2;
  std::vector<Ray<T> > rays;
  if (!read_mesh(dir + "/mesh0.bin", &m0) || !read_mesh(dir + "/mesh1.bin", &m1) || !read_mesh(dir + "/mesh2.bin", &m2) ||
      !read_rays(dir + "/rays.bin", &rays))
    return 2;
  size_t devices = 0;
  {  // refit: the object answers on the new positions, a copy made before on the old tree and old positions
    BVHAccel<T> a;
    expect("refit", "Build", a.Build(m0.nf, m0.tm(), m0.pred()));
    devices = a.NumHipDevices();
    check_tri("refit: built", a, m0, rays);
    const std::vector<nanort::BVHNode<T> > nodes0 = a.GetNodes();
    BVHAccel<T> copy = a;
    expect("refit", "Refit", a.Refit(m1.tm()));
    expect("refit", "Refit (again, same positions)", a.Refit(m1.tm()));
    check_tri("refit: refit object", a, m1, rays);
    check_tri("refit: copy made before", copy, m0, rays);
    expect("refit", "the copy keeps the old tree", same_nodes(copy.GetNodes(), nodes0));
    expect("refit", "the refit tree differs", !same_nodes(a.GetNodes(), nodes0));
    expect("refit", "topology kept", a.GetNodes().size() == nodes0.size());
    // a faces array with other contents is refused
    std::vector<unsigned int> other = m1.f;
    std::swap(other[0], other[1]);
    nanort::TriangleMesh<T> bad(m1.v.data(), other.data(), sizeof(T) * 3);
    expect("refit", "other faces refused", !a.Refit(bad) && !a.LastBackendError().empty());
    check_tri("refit: after the refusal", a, m1, rays);
    // move: a moved-into object refits
    BVHAccel<T> moved(std::move(a));
    expect("move", "Refit", moved.Refit(m2.tm()));
    check_tri("move: refit", moved, m2, rays);
    // the copy refits on its own, the moved-into object keeps its positions
    expect("copy", "Refit", copy.Refit(m2.tm()));
    check_tri("copy: refit", copy, m2, rays);
    check_tri("move: untouched by the copy's refit", moved, m2, rays);
  }
  if (sizeof(T) == 4) {  // kinds: spheres and cylinders refuse
    std::vector<float> c(300), r(100, 0.05f), e(600), cr(200, 0.02f);
    for (size_t i = 0; i < c.size(); i++) c[i] = static_cast<float>((i * 7919) % 1000) / 500.0f - 1.0f;
    for (size_t i = 0; i < e.size(); i++) e[i] = static_cast<float>((i * 104729) % 1000) / 500.0f - 1.0f;
    BVHAccel<float> s;
    nanort::SphereGeometry sg(c.data(), r.data());
    expect("kinds", "sphere Build", s.Build(100, sg, nanort::SpherePred(c.data())));
    expect("kinds", "sphere Refit refused", !s.Refit(sg) && !s.LastBackendError().empty());
    BVHAccel<float> cy;
    nanort::CylinderGeometry cg(e.data(), cr.data());
    expect("kinds", "cylinder Build", cy.Build(100, cg, nanort::CylinderPred(e.data())));
    expect("kinds", "cylinder Refit refused", !cy.Refit(cg) && !cy.LastBackendError().empty());
  }
  printf("devices %zu checks %llu mismatches %llu\n", devices, g_checks, g_bad);
  return g_bad ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: refit_check f32|f64 DIR\n");
    return 2;
  }
  return std::string(argv[1]) == "f64" ? run<double>(argv[2]) : run<float>(argv[2]);
}

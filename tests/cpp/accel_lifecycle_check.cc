// tests/cpp/accel_lifecycle_check.cc — the HIP-backed BVHAccel of include/nanort.h across copies, moves, rebuilds, Load()
// and threads (tests/test_gpu_accel_lifecycle.py).
//
//   accel_lifecycle_check --list
//   accel_lifecycle_check --fixture DIR
//   accel_lifecycle_check SCENARIO f32|f64 DIR [OUT]
//
// DIR holds what the test writes: mesh_a.bin, mesh_b.bin ({u32 nv, u32 nf, float xyz[nv], u32 ijk[nf]}), rays.bin and
// prays.bin ({u64 n, Ray<float>[n]}: a camera over the meshes and the particle camera), spheres.bin ({u32 n, float
// xyz[n], float r[n]}), cylinders.bin ({u32 n, float ends[n][2][3], float radii[n][2]}), motion.bin ({u32 nv, u32 nf, float
// xyz0[nv], float xyz1[nv], u32 ijk[nf], u32 masks[nf], u32 other_masks[nf]}: a mesh with a second keyframe and two sets of
// visibility masks), mrays.bin (a camera over it), curves.bin ({u32 n, float cps[n][4][3], float radii[n][4]}) and crays.bin
// (the curve camera).  f64 widens meshes and rays.
//
// --fixture: no HIP call.  From the header's host classes alone, over host-built trees: the share of mrays.bin that answers
// differently at time 0.5 than at time 0, with the masks than without, with the other masks than with the first; the share of
// crays.bin that answers differently at 2 than at 4 subdivisions, and that hits at all.  The test holds them against its bounds.
//
// After every step, for every live accel, one invariant: each batch method returns exactly what the same object's per-ray
// host method returns on that object's own tree (TraverseBatch / TraverseBatches / the device variants against Traverse,
// OccludedBatch and the occlusion waves against Traverse's hit flag, MultiHitTraverseBatch at K = 1, 4, 16 against
// MultiHitTraverse), or it returns false with a non-empty LastBackendError() — a refusal, counted apart; the test knows
// how many each scenario must see.  Batches always run before the host reference, so they also run before the first
// host access of a freshly built tree.  Prints `scenario NAME checks N mismatches M refused R`; exits 1 on a mismatch.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "nanort.h"
#include <hip/hip_runtime_api.h>  // device buffers for the *Device entry points

using nanort::BVHAccel;
using nanort::Ray;

namespace {

template <typename T>
struct Mesh {
  std::vector<T> v;
  std::vector<unsigned int> f;
  unsigned int nf = 0;
  nanort::TriangleMesh<T> tm() const { return nanort::TriangleMesh<T>(v.data(), f.data(), sizeof(T) * 3); }
  nanort::TriangleSAHPred<T> pred() const { return nanort::TriangleSAHPred<T>(v.data(), f.data(), sizeof(T) * 3); }
};

// A predicate type other than TriangleSAHPred: Build() takes the generic host path (a host-built tree to Dump()).
template <typename T>
struct HostPred : nanort::TriangleSAHPred<T> {
  HostPred(const T *v, const unsigned int *f, size_t s) : nanort::TriangleSAHPred<T>(v, f, s) {}
};

struct Inputs {
  Mesh<float> a, b;
  std::vector<Ray<float> > rays, prays;
  std::vector<float> sc, sr, ce, cr;
  unsigned int ns = 0, nc = 0;
  Mesh<float> m0;          // motion.bin: keyframe 0 and the faces ...
  std::vector<float> m1;   // ... keyframe 1
  std::vector<unsigned int> masks, masks2;
  std::vector<Ray<float> > mrays, crays;
  std::vector<float> kc, kr;  // curves.bin
  unsigned int nk = 0;
};
Inputs g_in;
std::string g_dir;

struct Tally {
  unsigned long long checks = 0, mismatches = 0, refused = 0;
};
Tally g;

bool read_mesh(const std::string &path, Mesh<float> *m) {
  FILE *fp = fopen(path.c_str(), "rb");
  if (!fp) return false;
  uint32_t nv = 0, nf = 0;
  bool ok = fread(&nv, 4, 1, fp) == 1 && fread(&nf, 4, 1, fp) == 1;
  m->v.resize(3 * (size_t)nv);
  m->f.resize(3 * (size_t)nf);
  ok = ok && fread(m->v.data(), 4, m->v.size(), fp) == m->v.size() && fread(m->f.data(), 4, m->f.size(), fp) == m->f.size();
  m->nf = nf;
  fclose(fp);
  return ok;
}
bool read_rays(const std::string &path, std::vector<Ray<float> > *r) {
  FILE *fp = fopen(path.c_str(), "rb");
  if (!fp) return false;
  uint64_t n = 0;
  bool ok = fread(&n, 8, 1, fp) == 1;
  r->resize((size_t)n);
  ok = ok && fread(r->data(), sizeof(Ray<float>), (size_t)n, fp) == n;
  fclose(fp);
  return ok;
}
bool read_prims(const std::string &path, unsigned int per_a, unsigned int per_b, std::vector<float> *a, std::vector<float> *b, unsigned int *n) {
  FILE *fp = fopen(path.c_str(), "rb");
  if (!fp) return false;
  uint32_t k = 0;
  bool ok = fread(&k, 4, 1, fp) == 1;
  a->resize((size_t)per_a * k);
  b->resize((size_t)per_b * k);
  ok = ok && fread(a->data(), 4, a->size(), fp) == a->size() && fread(b->data(), 4, b->size(), fp) == b->size();
  *n = k;
  fclose(fp);
  return ok;
}
bool read_motion(const std::string &path) {
  FILE *fp = fopen(path.c_str(), "rb");
  if (!fp) return false;
  uint32_t nv = 0, nf = 0;
  bool ok = fread(&nv, 4, 1, fp) == 1 && fread(&nf, 4, 1, fp) == 1;
  g_in.m0.v.resize(3 * (size_t)nv);
  g_in.m1.resize(3 * (size_t)nv);
  g_in.m0.f.resize(3 * (size_t)nf);
  g_in.m0.nf = nf;
  g_in.masks.resize(nf);
  g_in.masks2.resize(nf);
  ok = ok && fread(g_in.m0.v.data(), 4, 3 * (size_t)nv, fp) == 3 * (size_t)nv && fread(g_in.m1.data(), 4, 3 * (size_t)nv, fp) == 3 * (size_t)nv &&
       fread(g_in.m0.f.data(), 4, 3 * (size_t)nf, fp) == 3 * (size_t)nf && fread(g_in.masks.data(), 4, nf, fp) == nf &&
       fread(g_in.masks2.data(), 4, nf, fp) == nf;
  fclose(fp);
  return ok;
}
bool read_inputs(const std::string &dir) {
  if (!(read_motion(dir + "/motion.bin") && read_rays(dir + "/mrays.bin", &g_in.mrays) && read_rays(dir + "/crays.bin", &g_in.crays) &&
        read_prims(dir + "/curves.bin", 12, 4, &g_in.kc, &g_in.kr, &g_in.nk)))
    return false;
  return read_mesh(dir + "/mesh_a.bin", &g_in.a) && read_mesh(dir + "/mesh_b.bin", &g_in.b) && read_rays(dir + "/rays.bin", &g_in.rays) &&
         read_rays(dir + "/prays.bin", &g_in.prays) && read_prims(dir + "/spheres.bin", 3, 1, &g_in.sc, &g_in.sr, &g_in.ns) &&
         read_prims(dir + "/cylinders.bin", 6, 2, &g_in.ce, &g_in.cr, &g_in.nc);
}

template <typename T>
Mesh<T> widen(const Mesh<float> &m, float shift = 0.0f) {
  Mesh<T> o;
  o.v.resize(m.v.size());
  for (size_t i = 0; i < m.v.size(); i++) o.v[i] = static_cast<T>(m.v[i] + (i % 3 == 0 ? shift : 0.0f));
  o.f = m.f;
  o.nf = m.nf;
  return o;
}
template <typename T>
std::vector<Ray<T> > widen(const std::vector<Ray<float> > &r) {
  std::vector<Ray<T> > o(r.size());
  for (size_t i = 0; i < r.size(); i++) {
    for (int k = 0; k < 3; k++) {
      o[i].org[k] = r[i].org[k];
      o[i].dir[k] = r[i].dir[k];
    }
    o[i].min_t = r[i].min_t;
    o[i].max_t = r[i].max_t;
    o[i].type = r[i].type;
  }
  return o;
}

template <typename X>
bool bits_eq(const X &a, const X &b) {
  return memcmp(&a, &b, sizeof(X)) == 0;
}

void tally(const char *where, const char *method, unsigned long long bad) {
  g.checks++;
  if (bad) {
    g.mismatches += bad;
    fprintf(stderr, "MISMATCH %s %s: %llu\n", where, method, bad);
  }
}
// a batch method returned false: a refusal when it says why, a failure when it does not
void refusal(const char *where, const char *method, const std::string &err) {
  if (err.empty()) {
    g.mismatches++;
    fprintf(stderr, "MISMATCH %s %s: returned false without a reason\n", where, method);
  } else {
    g.refused++;
    fprintf(stderr, "refused %s %s: %s\n", where, method, err.c_str());
  }
}
// where the contract documents a refusal: records handed out instead are a mismatch
void must_refuse(const char *where, const char *method, bool ok, const std::string &err) {
  if (ok) {
    g.mismatches++;
    fprintf(stderr, "MISMATCH %s %s: returned records where the contract refuses\n", where, method);
  } else {
    refusal(where, method, err);
  }
}
void expect(const char *where, const char *what, bool cond) {
  g.checks++;
  if (!cond) {
    g.mismatches++;
    fprintf(stderr, "MISMATCH %s: %s\n", where, what);
  }
}

struct DevBuf {
  void *p = NULL;
  explicit DevBuf(size_t bytes) {
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) {
      fprintf(stderr, "hipMalloc(%zu) failed\n", bytes);
      exit(3);
    }
  }
  ~DevBuf() { hipFree(p); }
  template <class X>
  X *as() const {
    return static_cast<X *>(p);
  }
};
template <class X>
void to_host(std::vector<X> *dst, const DevBuf &src, hipStream_t s) {
  hipMemcpyAsync(dst->data(), src.p, dst->size() * sizeof(X), hipMemcpyDeviceToHost, s);
}

const unsigned int kMultiK[3] = {1, 4, 16};
const unsigned int kDeviceK = 4;

// ---- the invariant for a triangle accel: every batch method, then the per-ray host walk over the object's own tree ----
template <typename T>
void check_tri(const char *where, const BVHAccel<T> &a, const Mesh<T> &m, const std::vector<Ray<T> > &rays, bool *pending_after_batches = NULL,
               const char *save = NULL) {
  typedef nanort::TriangleIntersection<T> H;
  const size_t n = rays.size();
  H sentinel;
  memset(static_cast<void *>(&sentinel), 0x5A, sizeof(H));
  sentinel.u = sentinel.v = sentinel.t = T(-7);
  sentinel.prim_id = 0xDEADBEEFu;
  // 1. the batch methods (host arrays untouched so far when the accel was just built)
  std::vector<H> bh(n, sentinel), wh(n, sentinel);
  std::vector<unsigned char> bm(n, 7), wm(n, 7), wo(n, 7), ob(n, 7);
  const bool ok_b = a.TraverseBatch(rays.data(), n, bh.data(), bm.data());
  const std::string err_b = a.LastBackendError();
  const Ray<T> *wr[2] = {rays.data(), rays.data()};
  const size_t wn[2] = {n, n};
  H *wi[2] = {wh.data(), NULL};
  unsigned char *wmk[2] = {wm.data(), wo.data()};
  const unsigned char occ[2] = {0, 1};
  const bool ok_w = a.TraverseBatches(2, wr, wn, wi, wmk, occ);
  const std::string err_w = a.LastBackendError();
  const bool ok_o = a.OccludedBatch(rays.data(), n, ob.data());
  const std::string err_o = a.LastBackendError();
  std::vector<H> mh[3];
  std::vector<unsigned int> mc[3];
  bool ok_m[3];
  std::string err_m[3];
  for (int k = 0; k < 3; k++) {
    mh[k].assign(n * kMultiK[k], sentinel);
    mc[k].assign(n, 0xFFFFu);
    ok_m[k] = a.MultiHitTraverseBatch(rays.data(), n, kMultiK[k], mh[k].data(), mc[k].data());
    err_m[k] = a.LastBackendError();
  }
  // device-resident variants, on one stream
  hipStream_t s;
  if (hipStreamCreate(&s) != hipSuccess) exit(3);
  DevBuf d_rays(n * sizeof(Ray<T>)), d_h(n * sizeof(H)), d_m(n), d_wh(n * sizeof(H)), d_wm(n), d_wo(n), d_o(n), d_mh(n * kDeviceK * sizeof(H)),
      d_mc(n * sizeof(unsigned int));
  hipMemcpyAsync(d_rays.p, rays.data(), n * sizeof(Ray<T>), hipMemcpyHostToDevice, s);
  const bool ok_db = a.TraverseBatchDevice(d_rays.as<Ray<T> >(), n, d_h.as<H>(), d_m.as<unsigned char>(), s);
  const std::string err_db = a.LastBackendError();
  const Ray<T> *dwr[2] = {d_rays.as<Ray<T> >(), d_rays.as<Ray<T> >()};
  H *dwi[2] = {d_wh.as<H>(), NULL};
  unsigned char *dwm[2] = {d_wm.as<unsigned char>(), d_wo.as<unsigned char>()};
  const bool ok_dw = a.TraverseBatchesDevice(2, dwr, wn, dwi, dwm, occ, s);
  const std::string err_dw = a.LastBackendError();
  const bool ok_do = a.OccludedBatchDevice(d_rays.as<Ray<T> >(), n, d_o.as<unsigned char>(), s);
  const std::string err_do = a.LastBackendError();
  const bool ok_dm = a.MultiHitTraverseBatchDevice(d_rays.as<Ray<T> >(), n, kDeviceK, d_mh.as<H>(), d_mc.as<unsigned int>(), s);
  const std::string err_dm = a.LastBackendError();
  std::vector<H> dh(n), dwh(n), dmh(n * kDeviceK);
  std::vector<unsigned char> dm(n), dwm_h(n), dwo(n), dob(n);
  std::vector<unsigned int> dmc(n);
  if (ok_db) to_host(&dh, d_h, s), to_host(&dm, d_m, s);
  if (ok_dw) to_host(&dwh, d_wh, s), to_host(&dwm_h, d_wm, s), to_host(&dwo, d_wo, s);
  if (ok_do) to_host(&dob, d_o, s);
  if (ok_dm) to_host(&dmh, d_mh, s), to_host(&dmc, d_mc, s);
  if (hipStreamSynchronize(s) != hipSuccess) {
    fprintf(stderr, "hipStreamSynchronize failed\n");
    exit(3);
  }
  hipStreamDestroy(s);
  if (pending_after_batches) *pending_after_batches = a.HostTreePending();

  // 2. the host reference on the same object
  nanort::TriangleIntersector<T> isect(m.v.data(), m.f.data(), sizeof(T) * 3);
  std::vector<H> hh(n, sentinel);
  std::vector<unsigned char> hm(n);
  for (size_t i = 0; i < n; i++) hm[i] = a.Traverse(rays[i], isect, &hh[i]) ? 1 : 0;
  auto same = [](const H &x, const H &y) { return bits_eq(x.t, y.t) && x.prim_id == y.prim_id && x.u == y.u && x.v == y.v; };
  auto untouched = [&](const H &x) { return bits_eq(x.t, sentinel.t) && x.prim_id == sentinel.prim_id && x.u == sentinel.u && x.v == sentinel.v; };
  auto miss_rec = [](const H &x, const Ray<T> &r) { return bits_eq(x.t, r.max_t) && x.prim_id == 0xFFFFFFFFu && x.u == T(0) && x.v == T(0); };
  std::string w = where;
  if (ok_b) {
    unsigned long long bad = 0;
    for (size_t i = 0; i < n; i++)
      if (bm[i] != hm[i] || !(hm[i] ? same(bh[i], hh[i]) : untouched(bh[i]))) bad++;
    tally(where, "TraverseBatch", bad);
  } else {
    refusal(where, "TraverseBatch", err_b);
  }
  if (ok_w) {
    unsigned long long bad = 0;
    for (size_t i = 0; i < n; i++)
      if (wm[i] != hm[i] || wo[i] != hm[i] || !(hm[i] ? same(wh[i], hh[i]) : untouched(wh[i]))) bad++;
    tally(where, "TraverseBatches", bad);
  } else {
    refusal(where, "TraverseBatches", err_w);
  }
  if (ok_o) {
    unsigned long long bad = 0;
    for (size_t i = 0; i < n; i++) bad += ob[i] != hm[i];
    tally(where, "OccludedBatch", bad);
  } else {
    refusal(where, "OccludedBatch", err_o);
  }
  if (ok_db) {
    unsigned long long bad = 0;
    for (size_t i = 0; i < n; i++)
      if (dm[i] != hm[i] || !(hm[i] ? same(dh[i], hh[i]) : miss_rec(dh[i], rays[i]))) bad++;
    tally(where, "TraverseBatchDevice", bad);
  } else {
    refusal(where, "TraverseBatchDevice", err_db);
  }
  if (ok_dw) {
    unsigned long long bad = 0;
    for (size_t i = 0; i < n; i++)
      if (dwm_h[i] != hm[i] || dwo[i] != hm[i] || !(hm[i] ? same(dwh[i], hh[i]) : miss_rec(dwh[i], rays[i]))) bad++;
    tally(where, "TraverseBatchesDevice", bad);
  } else {
    refusal(where, "TraverseBatchesDevice", err_dw);
  }
  if (ok_do) {
    unsigned long long bad = 0;
    for (size_t i = 0; i < n; i++) bad += dob[i] != hm[i];
    tally(where, "OccludedBatchDevice", bad);
  } else {
    refusal(where, "OccludedBatchDevice", err_do);
  }
  // multi-hit: the host walk's held hits, then miss records
  for (int k = 0; k < 4; k++) {
    const bool dev = k == 3;
    const unsigned int K = dev ? kDeviceK : kMultiK[k];
    const bool ok = dev ? ok_dm : ok_m[k];
    const char *name = dev ? "MultiHitTraverseBatchDevice" : "MultiHitTraverseBatch";
    if (!ok) {
      refusal(where, name, dev ? err_dm : err_m[k]);
      continue;
    }
    const std::vector<H> &rows = dev ? dmh : mh[k];
    const std::vector<unsigned int> &cnt = dev ? dmc : mc[k];
    unsigned long long bad = 0;
    for (size_t i = 0; i < n; i++) {
      nanort::StackVector<H, 128> held;
      a.MultiHitTraverse(rays[i], (int)K, isect, &held);
      bool good = cnt[i] == held->size() && (held->size() > 0) == (hm[i] != 0);
      for (unsigned int j = 0; good && j < K; j++)
        good = j < held->size() ? same(rows[i * K + j], held[j]) : miss_rec(rows[i * K + j], rays[i]);
      bad += !good;
    }
    char label[64];
    snprintf(label, sizeof(label), "%s(K=%u)", name, K);
    tally(where, label, bad);
  }
  if (save && ok_b) {  // the batch records and the tree they came from, for the oracle (tests/test_gpu_accel_lifecycle.py)
    FILE *fp = fopen(save, "wb");
    if (!fp) exit(2);
    fwrite(bh.data(), sizeof(H), n, fp);
    fwrite(bm.data(), 1, n, fp);
    const uint64_t nn = a.GetNodes().size(), ni = a.GetIndices().size();
    fwrite(&nn, 8, 1, fp);
    fwrite(a.GetNodes().data(), sizeof(nanort::BVHNode<T>), nn, fp);
    fwrite(&ni, 8, 1, fp);
    fwrite(a.GetIndices().data(), 4, ni, fp);
    fclose(fp);
  }
}

// ---- spheres / cylinders: TraverseBatch against Traverse (fp32 only) ----
void check_sph(const char *where, const BVHAccel<float> &a) {
  typedef nanort::SphereIntersection H;
  const std::vector<Ray<float> > &rays = g_in.prays;
  const size_t n = rays.size();
  H sentinel;
  sentinel.u = sentinel.v = sentinel.t = -7.0f;
  sentinel.prim_id = 0xDEADBEEFu;
  std::vector<H> bh(n, sentinel), hh(n, sentinel);
  std::vector<unsigned char> bm(n, 7), hm(n);
  const bool ok = a.TraverseBatch(rays.data(), n, bh.data(), bm.data());
  if (!ok) return refusal(where, "TraverseBatch(sphere)", a.LastBackendError());
  nanort::SphereIntersector<H> isect(g_in.sc.data(), g_in.sr.data());
  unsigned long long bad = 0;
  for (size_t i = 0; i < n; i++) {
    hm[i] = a.Traverse(rays[i], isect, &hh[i]) ? 1 : 0;
    const H &x = bh[i], &y = hh[i];
    const bool good = hm[i] ? (bits_eq(x.t, y.t) && x.prim_id == y.prim_id && std::fabs(x.u - y.u) <= 1e-6f && std::fabs(x.v - y.v) <= 1e-6f)
                            : memcmp(&x, &sentinel, sizeof(H)) == 0;
    bad += bm[i] != hm[i] || !good;
  }
  tally(where, "TraverseBatch(sphere)", bad);
}

// `default_call`: TraverseBatch(rays, n, isects, hit_out) — the cap flag the application never names
void check_cyl(const char *where, const BVHAccel<float> &a, bool cap, bool default_call = false) {
  typedef nanort::CylinderIntersection H;
  const std::vector<Ray<float> > &rays = g_in.prays;
  const size_t n = rays.size();
  H sentinel;
  memset(static_cast<void *>(&sentinel), 0x5A, sizeof(H));
  std::vector<H> bh(n, sentinel), hh(n, sentinel);
  std::vector<unsigned char> bm(n, 7), hm(n);
  const bool ok = default_call ? a.TraverseBatch(rays.data(), n, bh.data(), bm.data())
                               : a.TraverseBatch(rays.data(), n, bh.data(), bm.data(), nanort::BVHTraceOptions(), cap);
  const char *name = cap ? "TraverseBatch(cylinder, cap)" : "TraverseBatch(cylinder, no cap)";
  if (!ok) return refusal(where, name, a.LastBackendError());
  nanort::CylinderIntersector<H> isect(g_in.ce.data(), g_in.cr.data(), cap);
  unsigned long long bad = 0;
  for (size_t i = 0; i < n; i++) {
    hm[i] = a.Traverse(rays[i], isect, &hh[i]) ? 1 : 0;
    bad += bm[i] != hm[i] || memcmp(&bh[i], hm[i] ? &hh[i] : &sentinel, sizeof(H)) != 0;
  }
  tally(where, name, bad);
}

// the overloads and entry points of the other primitive kinds refuse (kind: 0 triangles, 1 spheres, 2 cylinders, -1 none)
template <typename T>
void check_tri_refused(const char *where, const BVHAccel<T> &a) {
  typedef nanort::TriangleIntersection<T> H;
  const std::vector<Ray<T> > rays = widen<T>(std::vector<Ray<float> >(g_in.rays.begin(), g_in.rays.begin() + 64));
  const size_t n = rays.size();
  std::vector<H> h(n * 4);
  std::vector<unsigned char> m(n), o(n);
  std::vector<unsigned int> c(n);
  must_refuse(where, "TraverseBatch", a.TraverseBatch(rays.data(), n, h.data(), m.data()), a.LastBackendError());
  const Ray<T> *wr[1] = {rays.data()};
  const size_t wn[1] = {n};
  H *wi[1] = {h.data()};
  unsigned char *wm[1] = {m.data()};
  must_refuse(where, "TraverseBatches", a.TraverseBatches(1, wr, wn, wi, wm, NULL), a.LastBackendError());
  must_refuse(where, "OccludedBatch", a.OccludedBatch(rays.data(), n, o.data()), a.LastBackendError());
  must_refuse(where, "MultiHitTraverseBatch", a.MultiHitTraverseBatch(rays.data(), n, 4, h.data(), c.data()), a.LastBackendError());
  DevBuf d_rays(n * sizeof(Ray<T>)), d_h(n * 4 * sizeof(H)), d_m(n), d_c(n * 4);
  hipMemcpy(d_rays.p, rays.data(), n * sizeof(Ray<T>), hipMemcpyHostToDevice);
  must_refuse(where, "TraverseBatchDevice", a.TraverseBatchDevice(d_rays.as<Ray<T> >(), n, d_h.as<H>(), d_m.as<unsigned char>(), NULL),
              a.LastBackendError());
  const Ray<T> *dwr[1] = {d_rays.as<Ray<T> >()};
  H *dwi[1] = {d_h.as<H>()};
  unsigned char *dwm[1] = {d_m.as<unsigned char>()};
  must_refuse(where, "TraverseBatchesDevice", a.TraverseBatchesDevice(1, dwr, wn, dwi, dwm, NULL, NULL), a.LastBackendError());
  must_refuse(where, "OccludedBatchDevice", a.OccludedBatchDevice(d_rays.as<Ray<T> >(), n, d_m.as<unsigned char>(), NULL), a.LastBackendError());
  must_refuse(where, "MultiHitTraverseBatchDevice",
              a.MultiHitTraverseBatchDevice(d_rays.as<Ray<T> >(), n, 4, d_h.as<H>(), d_c.as<unsigned int>(), NULL), a.LastBackendError());
  hipDeviceSynchronize();
}
void check_sph_refused(const char *where, const BVHAccel<float> &a) {
  std::vector<nanort::SphereIntersection> h(64);
  must_refuse(where, "TraverseBatch(sphere)", a.TraverseBatch(g_in.prays.data(), 64, h.data()), a.LastBackendError());
}
void check_cyl_refused(const char *where, const BVHAccel<float> &a) {
  std::vector<nanort::CylinderIntersection> h(64);
  must_refuse(where, "TraverseBatch(cylinder)", a.TraverseBatch(g_in.prays.data(), 64, h.data()), a.LastBackendError());
}
void check_prims_refused(const char *where, const BVHAccel<float> &a) {
  check_sph_refused(where, a);
  check_cyl_refused(where, a);
}
void check_prims_refused(const char *, const BVHAccel<double> &) {}

bool build_sph(BVHAccel<float> *a) {
  nanort::BVHBuildOptions<float> o;
  o.cache_bbox = false;
  return a->Build(g_in.ns, nanort::SphereGeometry(g_in.sc.data(), g_in.sr.data()), nanort::SpherePred(g_in.sc.data()), o);
}
bool build_cyl(BVHAccel<float> *a) {
  nanort::BVHBuildOptions<float> o;
  o.cache_bbox = false;
  return a->Build(g_in.nc, nanort::CylinderGeometry(g_in.ce.data(), g_in.cr.data()), nanort::CylinderPred(g_in.ce.data()), o);
}
template <typename T>
bool build_tri(BVHAccel<T> *a, const Mesh<T> &m) {
  return a->Build(m.nf, m.tm(), m.pred());
}
#define BUILD(call)                                                    \
  do {                                                                 \
    if (!(call)) {                                                     \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #call); \
      exit(3);                                                         \
    }                                                                  \
  } while (0)

// the spheres and cylinders of a f32 run (nothing for f64: those primitives are fp32)
void prims_batch_first(float) {
  BVHAccel<float> s, c;
  BUILD(build_sph(&s));
  check_sph("spheres", s);
  check_sph("spheres again", s);
  BUILD(build_cyl(&c));
  check_cyl("cylinders", c, true);
  check_cyl("cylinders again", c, true, true);
}
void prims_batch_first(double) {}

// ---- a triangle accel over a MotionTriangleMesh that holds visibility masks: the motion and the masked queries ----
template <typename T>
struct MotionFixture {
  Mesh<T> k0;        // keyframe 0 and the faces
  std::vector<T> v1;  // keyframe 1
  std::vector<Ray<T> > rays;
  std::vector<T> times;                 // every ray at time 0.5
  std::vector<unsigned int> ray_masks;  // 1, 2, 3, 1, ...: never all-ones
  MotionFixture() : k0(widen<T>(g_in.m0)), v1(g_in.m1.begin(), g_in.m1.end()), rays(widen<T>(g_in.mrays)), times(g_in.mrays.size(), T(0.5)) {
    for (size_t i = 0; i < rays.size(); i++) ray_masks.push_back(1u + static_cast<unsigned int>(i % 3));
  }
  nanort::MotionTriangleMesh<T> mesh() const { return nanort::MotionTriangleMesh<T>(k0.v.data(), v1.data(), k0.f.data(), sizeof(T) * 3); }
  nanort::MotionTriangleSAHPred<T> pred() const { return nanort::MotionTriangleSAHPred<T>(k0.v.data(), v1.data(), k0.f.data(), sizeof(T) * 3); }
  nanort::MotionTriangleIntersector<T> at_time() const { return nanort::MotionTriangleIntersector<T>(k0.v.data(), v1.data(), k0.f.data(), sizeof(T) * 3); }
  nanort::MaskedTriangleIntersector<T> masked(const unsigned int *masks) const {
    return nanort::MaskedTriangleIntersector<T>(k0.v.data(), k0.f.data(), sizeof(T) * 3, masks);
  }
};

// per ray, through the host walk: the record of `isect` after prepare(isect, i), the miss record where it misses
template <typename T, class I, class Prepare>
void host_records(const BVHAccel<T> &a, const std::vector<Ray<T> > &rays, const I &isect, Prepare prepare, std::vector<nanort::TriangleIntersection<T> > *h,
                  std::vector<unsigned char> *m) {
  h->resize(rays.size());
  m->resize(rays.size());
  for (size_t i = 0; i < rays.size(); i++) {
    nanort::TriangleIntersection<T> x;
    prepare(isect, i);
    (*m)[i] = a.Traverse(rays[i], isect, &x) ? 1 : 0;
    if (!(*m)[i]) {
      x.u = x.v = T(0);
      x.t = rays[i].max_t;
      x.prim_id = 0xFFFFFFFFu;
    }
    (*h)[i] = x;
  }
}
template <typename T>
unsigned long long records_differ(const std::vector<nanort::TriangleIntersection<T> > &x, const std::vector<unsigned char> &xm,
                                  const std::vector<nanort::TriangleIntersection<T> > &y, const std::vector<unsigned char> &ym) {
  unsigned long long bad = 0;
  for (size_t i = 0; i < x.size(); i++)
    bad += !(xm[i] == ym[i] && bits_eq(x[i].t, y[i].t) && x[i].prim_id == y[i].prim_id && bits_eq(x[i].u, y[i].u) && bits_eq(x[i].v, y[i].v));
  return bad;
}

// `masks`: the words the accel holds now (NULL: none — after a Build() — and the masked queries must refuse)
template <typename T>
void check_motion(const char *where, const BVHAccel<T> &a, const MotionFixture<T> &F, const unsigned int *masks) {
  typedef nanort::TriangleIntersection<T> H;
  const size_t n = F.rays.size();
  H sentinel;
  memset(static_cast<void *>(&sentinel), 0x5A, sizeof(H));
  std::vector<H> th(n, sentinel), kh(n, sentinel), hh;
  std::vector<unsigned char> tm(n, 7), to(n, 7), km(n, 7), ko(n, 7), hm;
  // the batch methods first (every record is written, a miss as the miss record), then the host walk of the same object
  const bool ok_t = a.TraverseBatchMotion(F.rays.data(), F.times.data(), n, th.data(), tm.data());
  const std::string err_t = a.LastBackendError();
  const bool ok_to = a.OccludedBatchMotion(F.rays.data(), F.times.data(), n, to.data());
  const std::string err_to = a.LastBackendError();
  const bool ok_k = a.TraverseBatchMasked(F.rays.data(), F.ray_masks.data(), n, kh.data(), km.data());
  const std::string err_k = a.LastBackendError();
  const bool ok_ko = a.OccludedBatchMasked(F.rays.data(), F.ray_masks.data(), n, ko.data());
  const std::string err_ko = a.LastBackendError();
  host_records(a, F.rays, F.at_time(), [&](const nanort::MotionTriangleIntersector<T> &x, size_t i) { x.SetTime(F.times[i]); }, &hh, &hm);
  if (ok_t)
    tally(where, "TraverseBatchMotion", records_differ(th, tm, hh, hm));
  else
    refusal(where, "TraverseBatchMotion", err_t);
  if (ok_to)
    tally(where, "OccludedBatchMotion", to != hm);
  else
    refusal(where, "OccludedBatchMotion", err_to);
  if (!masks) {
    must_refuse(where, "TraverseBatchMasked", ok_k, err_k);
    must_refuse(where, "OccludedBatchMasked", ok_ko, err_ko);
    return;
  }
  host_records(a, F.rays, F.masked(masks), [&](const nanort::MaskedTriangleIntersector<T> &x, size_t i) { x.SetRayMask(F.ray_masks[i]); }, &hh, &hm);
  if (ok_k)
    tally(where, "TraverseBatchMasked", records_differ(kh, km, hh, hm));
  else
    refusal(where, "TraverseBatchMasked", err_k);
  if (ok_ko)
    tally(where, "OccludedBatchMasked", ko != hm);
  else
    refusal(where, "OccludedBatchMasked", err_ko);
}
// an object with no tree (moved-from): the four queries refuse
template <typename T>
void check_motion_refused(const char *where, const BVHAccel<T> &a, const MotionFixture<T> &F) {
  const size_t n = 64;
  std::vector<nanort::TriangleIntersection<T> > h(n);
  std::vector<unsigned char> m(n);
  must_refuse(where, "TraverseBatchMotion", a.TraverseBatchMotion(F.rays.data(), F.times.data(), n, h.data(), m.data()), a.LastBackendError());
  must_refuse(where, "OccludedBatchMotion", a.OccludedBatchMotion(F.rays.data(), F.times.data(), n, m.data()), a.LastBackendError());
  must_refuse(where, "TraverseBatchMasked", a.TraverseBatchMasked(F.rays.data(), F.ray_masks.data(), n, h.data(), m.data()), a.LastBackendError());
  must_refuse(where, "OccludedBatchMasked", a.OccludedBatchMasked(F.rays.data(), F.ray_masks.data(), n, m.data()), a.LastBackendError());
}

// ---- curves: TraverseBatch(BezierCurveIntersection*) and OccludedBatchCurves against Traverse (fp32 only) ----
void host_curves(const BVHAccel<float> &a, int subdiv, std::vector<nanort::BezierCurveIntersection> *h, std::vector<unsigned char> *m) {
  const std::vector<Ray<float> > &rays = g_in.crays;
  h->assign(rays.size(), nanort::BezierCurveIntersection());
  m->assign(rays.size(), 0);
  for (size_t i = 0; i < rays.size(); i++) {
    nanort::BezierCurveIntersector<> isect(g_in.kc.data(), g_in.kr.data(), subdiv);
    (*m)[i] = a.Traverse(rays[i], isect, &(*h)[i]) ? 1 : 0;
  }
}
void check_crv(const char *where, const BVHAccel<float> &a, int subdiv) {
  typedef nanort::BezierCurveIntersection H;
  const std::vector<Ray<float> > &rays = g_in.crays;
  const size_t n = rays.size();
  std::vector<H> bh(n), hh;
  std::vector<unsigned char> bm(n, 7), bo(n, 7), hm;
  const bool ok = a.TraverseBatch(rays.data(), n, bh.data(), bm.data(), nanort::BVHTraceOptions(), subdiv);
  const std::string err = a.LastBackendError();
  const bool ok_o = a.OccludedBatchCurves(rays.data(), n, bo.data(), nanort::BVHTraceOptions(), subdiv);
  const std::string err_o = a.LastBackendError();
  host_curves(a, subdiv, &hh, &hm);
  char name[64];
  snprintf(name, sizeof(name), "TraverseBatch(curve, %d subdivisions)", subdiv);
  if (ok) {
    unsigned long long bad = 0;
    for (size_t i = 0; i < n; i++) bad += bm[i] != hm[i] || memcmp(static_cast<const void *>(&bh[i]), static_cast<const void *>(&hh[i]), sizeof(H)) != 0;
    tally(where, name, bad);
  } else {
    refusal(where, name, err);
  }
  if (ok_o)
    tally(where, "OccludedBatchCurves", bo != hm);
  else
    refusal(where, "OccludedBatchCurves", err_o);
}
void check_crv_refused(const char *where, const BVHAccel<float> &a) {
  std::vector<nanort::BezierCurveIntersection> h(64);
  std::vector<unsigned char> m(64);
  must_refuse(where, "TraverseBatch(curve)", a.TraverseBatch(g_in.crays.data(), 64, h.data()), a.LastBackendError());
  must_refuse(where, "OccludedBatchCurves", a.OccludedBatchCurves(g_in.crays.data(), 64, m.data()), a.LastBackendError());
}
bool build_crv(BVHAccel<float> *a) {
  nanort::BVHBuildOptions<float> o;
  o.cache_bbox = false;
  return a->Build(g_in.nk, nanort::BezierCurveGeometry(g_in.kc.data(), g_in.kr.data()), nanort::BezierCurvePred(g_in.kc.data()), o);
}

// ================================ scenarios ================================
template <typename T>
struct Fixture {
  Mesh<T> a, b;
  std::vector<Ray<T> > rays;
  Fixture() : a(widen<T>(g_in.a)), b(widen<T>(g_in.b)), rays(widen<T>(g_in.rays)) {}
};

template <typename T>
void batch_first() {
  Fixture<T> F;
  BVHAccel<T> a;
  BUILD(build_tri(&a, F.a));
  expect("batch_first", "HostTreePending() after Build()", a.HostTreePending());
  bool pending = false;
  check_tri("batch_first", a, F.a, F.rays, &pending);
  expect("batch_first", "the batch methods did not read the tree back", pending);
  check_tri("batch_first again", a, F.a, F.rays);
  prims_batch_first(T());
}

void cyl_cap_first() {
  BVHAccel<float> c;
  BUILD(build_cyl(&c));
  check_cyl("cyl_cap_first first call", c, false);
  check_cyl("cyl_cap_first", c, true);
  check_cyl("cyl_cap_first again", c, false);
  check_cyl("cyl_cap_first default", c, true, true);
  // the scene must tell the two flags apart, or none of this checks anything
  nanort::CylinderIntersector<nanort::CylinderIntersection> with(g_in.ce.data(), g_in.cr.data(), true), without(g_in.ce.data(), g_in.cr.data(), false);
  size_t differ = 0;
  for (size_t i = 0; i < g_in.prays.size(); i++) {
    nanort::CylinderIntersection x, y;
    memset(static_cast<void *>(&x), 0, sizeof(x));
    memset(static_cast<void *>(&y), 0, sizeof(y));
    c.Traverse(g_in.prays[i], with, &x);
    c.Traverse(g_in.prays[i], without, &y);
    differ += memcmp(&x, &y, sizeof(x)) != 0;
  }
  expect("cyl_cap_first", "the cap flag changes some records", differ > 0);
}

template <typename T>
void copy_then_rebuild_copy(const char *save) {
  Fixture<T> F;
  BVHAccel<T> a;
  BUILD(build_tri(&a, F.a));
  BVHAccel<T> b(a);
  BVHAccel<T> c;
  BUILD(build_tri(&c, F.b));  // (assigned over an accel that has a context of its own)
  c = a;
  check_tri("copy_then_rebuild_copy copy before", b, F.a, F.rays);
  expect("copy_then_rebuild_copy", "a copy shares the original's context until it changes it", b.HipContext() == a.HipContext());
  BUILD(build_tri(&b, F.b));
  BUILD(build_tri(&c, F.b));
  expect("copy_then_rebuild_copy", "HipContext() of a rebuilt copy is its own", b.HipContext() != a.HipContext() && c.HipContext() != a.HipContext() &&
                                                                               b.HipContext() != c.HipContext() && b.HipContext() != NULL);
  check_tri("copy_then_rebuild_copy original", a, F.a, F.rays, NULL, save);
  check_tri("copy_then_rebuild_copy copy", b, F.b, F.rays);
  check_tri("copy_then_rebuild_copy assigned", c, F.b, F.rays);
  check_tri("copy_then_rebuild_copy original again", a, F.a, F.rays);
}

template <typename T>
void copy_then_rebuild_original() {
  Fixture<T> F;
  BVHAccel<T> a;
  BUILD(build_tri(&a, F.a));
  BVHAccel<T> b(a);
  BVHAccel<T> c;
  c = a;
  BUILD(build_tri(&a, F.b));
  check_tri("copy_then_rebuild_original copy", b, F.a, F.rays);
  check_tri("copy_then_rebuild_original assigned", c, F.a, F.rays);
  check_tri("copy_then_rebuild_original original", a, F.b, F.rays);
  check_tri("copy_then_rebuild_original copy again", b, F.a, F.rays);
}

void copy_then_kind_change() {
  Fixture<float> F;
  BVHAccel<float> a;
  BUILD(build_tri(&a, F.a));
  BVHAccel<float> b(a);
  BUILD(build_sph(&b));
  check_tri("copy_then_kind_change original (copy is spheres)", a, F.a, F.rays);
  check_sph("copy_then_kind_change copy (spheres)", b);
  BUILD(build_cyl(&b));
  check_tri("copy_then_kind_change original (copy is cylinders)", a, F.a, F.rays);
  check_cyl("copy_then_kind_change copy (cylinders)", b, true, true);
  check_cyl("copy_then_kind_change copy (cylinders, no cap)", b, false);
  check_tri("copy_then_kind_change original again", a, F.a, F.rays);
}

// a host-built tree over the first half of mesh A's faces (a valid tree of the same mesh arrays, another topology), dumped
template <typename T>
std::string dump_half_tree(const Mesh<T> &m, const char *tag) {
  BVHAccel<T> h;
  BUILD(h.Build(m.nf / 2, m.tm(), HostPred<T>(m.v.data(), m.f.data(), sizeof(T) * 3)));
  const std::string path = g_dir + "/" + tag + (sizeof(T) == 8 ? "_f64" : "_f32") + ".bvh";
  BUILD(h.Dump(path.c_str()));
  return path;
}

template <typename T>
void copy_then_load() {
  Fixture<T> F;
  const std::string path = dump_half_tree(F.a, "copy_then_load");
  BVHAccel<T> a;
  BUILD(build_tri(&a, F.a));
  BVHAccel<T> b(a);
  BUILD(b.Load(path.c_str()));
  check_tri("copy_then_load copy (loaded)", b, F.a, F.rays);
  check_tri("copy_then_load original", a, F.a, F.rays);
  BVHAccel<T> c;  // the same through copy-assignment, original checked first
  c = a;
  BUILD(c.Load(path.c_str()));
  check_tri("copy_then_load assigned (loaded)", c, F.a, F.rays);
  check_tri("copy_then_load original again", a, F.a, F.rays);
}

void copy_cyl_cap_flip() {
  BVHAccel<float> a;
  BUILD(build_cyl(&a));
  check_cyl("copy_cyl_cap_flip original", a, true, true);
  BVHAccel<float> b(a);
  check_cyl("copy_cyl_cap_flip copy, no cap", b, false);
  check_cyl("copy_cyl_cap_flip original default", a, true, true);
  check_cyl("copy_cyl_cap_flip copy, no cap again", b, false);
  BVHAccel<float> c;
  c = a;
  check_cyl("copy_cyl_cap_flip assigned, no cap", c, false);
  check_cyl("copy_cyl_cap_flip original default again", a, true, true);
  check_cyl("copy_cyl_cap_flip copy default", b, true, true);
}

template <typename T>
void batch_records(const BVHAccel<T> &a, const std::vector<Ray<T> > &rays, std::vector<nanort::TriangleIntersection<T> > *h,
                   std::vector<unsigned char> *m, bool *ok) {
  h->assign(rays.size(), nanort::TriangleIntersection<T>());
  m->assign(rays.size(), 0);
  *ok = a.TraverseBatch(rays.data(), rays.size(), h->data(), m->data());
}
template <typename T>
bool same_records(const std::vector<nanort::TriangleIntersection<T> > &x, const std::vector<unsigned char> &xm,
                  const std::vector<nanort::TriangleIntersection<T> > &y, const std::vector<unsigned char> &ym) {
  if (xm != ym) return false;
  for (size_t i = 0; i < x.size(); i++)
    if (xm[i] && !(bits_eq(x[i].t, y[i].t) && x[i].prim_id == y[i].prim_id && x[i].u == y[i].u && x[i].v == y[i].v)) return false;
  return true;
}

template <typename T>
void move() {
  Fixture<T> F;
  std::vector<nanort::TriangleIntersection<T> > h0, h1;
  std::vector<unsigned char> m0, m1;
  bool ok0 = false, ok1 = false;
  BVHAccel<T> s;
  BUILD(build_tri(&s, F.a));
  batch_records(s, F.rays, &h0, &m0, &ok0);
  expect("move", "TraverseBatch before the move", ok0);
  BVHAccel<T> t(std::move(s));
  expect("move", "move-constructed target: HostTreePending() == 1 (no read-back)", t.HostTreePending());
  expect("move", "moved-from source: IsValid() == false", !s.IsValid());
  batch_records(t, F.rays, &h1, &m1, &ok1);
  expect("move", "move-constructed target: the source's records", ok1 && same_records(h0, m0, h1, m1));
  check_tri_refused("move moved-from", s);  // (empty: every batch method refuses)
  BUILD(build_tri(&s, F.b));                    // the moved-from object is rebuilt
  check_tri("move moved-from rebuilt", s, F.b, F.rays);
  BVHAccel<T> u;
  BUILD(build_tri(&u, F.b));  // (the target of the assignment has a context of its own)
  u = std::move(t);
  expect("move", "move-assigned target: HostTreePending() == 1 (no read-back)", u.HostTreePending());
  expect("move", "moved-from source: IsValid() == false", !t.IsValid());
  batch_records(u, F.rays, &h1, &m1, &ok1);
  expect("move", "move-assigned target: the source's records", ok1 && same_records(h0, m0, h1, m1));
  check_tri("move move-assigned", u, F.a, F.rays);
  { BVHAccel<T> dead(std::move(u)); }  // destroyed after a move: u's context went with it
  expect("move", "moved-from source: IsValid() == false", !u.IsValid());
  check_tri("move rebuilt source after target died", s, F.b, F.rays);
}

template <typename T>
void vector_growth() {
  Fixture<T> F;
  std::vector<Mesh<T> > meshes;
  for (int k = 0; k < 8; k++) meshes.push_back(widen<T>(k % 2 ? g_in.b : g_in.a, 0.01f * k));
  std::vector<BVHAccel<T> > v;  // no reserve(): push_back reallocates on the way
  for (int k = 0; k < 8; k++) {
    BVHAccel<T> a;
    BUILD(build_tri(&a, meshes[k]));
    v.push_back(std::move(a));
  }
  for (int k = 0; k < 8; k++) {
    char w[64];
    snprintf(w, sizeof(w), "vector_growth [%d]", k);
    expect(w, "HostTreePending() after the reallocations (moved, not copied)", v[k].HostTreePending());
    check_tri(w, v[k], meshes[k], F.rays);
  }
}

void kind_cycle() {
  Fixture<float> F;
  BVHAccel<float> a;
  BUILD(build_tri(&a, F.a));
  check_tri("kind_cycle triangles", a, F.a, F.rays);
  check_prims_refused("kind_cycle triangles", a);
  BUILD(build_sph(&a));
  check_sph("kind_cycle spheres", a);
  check_tri_refused("kind_cycle spheres", a);
  check_cyl_refused("kind_cycle spheres", a);
  BUILD(build_cyl(&a));
  check_cyl("kind_cycle cylinders", a, true, true);
  check_tri_refused("kind_cycle cylinders", a);
  check_sph_refused("kind_cycle cylinders", a);
  BUILD(build_tri(&a, F.b));
  check_tri("kind_cycle triangles again", a, F.b, F.rays);
  check_prims_refused("kind_cycle triangles again", a);
}

template <typename T>
void empty_rebuild() {
  Fixture<T> F;
  BVHAccel<T> a;
  BUILD(build_tri(&a, F.a));
  check_tri("empty_rebuild", a, F.a, F.rays);
  expect("empty_rebuild", "Build(0, ...) returns false", !a.Build(0, F.a.tm(), F.a.pred()));
  expect("empty_rebuild", "IsValid() false after Build(0, ...)", !a.IsValid());
  check_tri_refused("empty_rebuild empty", a);
  check_prims_refused("empty_rebuild empty", a);
  BUILD(build_tri(&a, F.b));
  check_tri("empty_rebuild rebuilt", a, F.b, F.rays);
}

template <typename T>
void load_refusals() {
  Fixture<T> F;
  const std::string path = dump_half_tree(F.a, "load_refusals");
  BVHAccel<T> a;
  BUILD(build_tri(&a, F.a));
  BUILD(a.Load(path.c_str()));
  expect("load_refusals", "HipContext() is NULL while the loaded tree is not on the device", a.HipContext() == NULL);
  // the device entries and OccludedBatch refuse until one TraverseBatch() has sent the loaded tree (documented)
  typedef nanort::TriangleIntersection<T> H;
  const size_t n = F.rays.size();
  std::vector<unsigned char> o(n);
  must_refuse("load_refusals", "OccludedBatch", a.OccludedBatch(F.rays.data(), n, o.data()), a.LastBackendError());
  DevBuf d_rays(n * sizeof(Ray<T>)), d_h(n * 4 * sizeof(H)), d_m(n), d_c(n * 4);
  hipMemcpy(d_rays.p, F.rays.data(), n * sizeof(Ray<T>), hipMemcpyHostToDevice);
  must_refuse("load_refusals", "TraverseBatchDevice", a.TraverseBatchDevice(d_rays.as<Ray<T> >(), n, d_h.as<H>(), d_m.as<unsigned char>(), NULL),
              a.LastBackendError());
  const Ray<T> *dwr[1] = {d_rays.as<Ray<T> >()};
  const size_t wn[1] = {n};
  H *dwi[1] = {d_h.as<H>()};
  unsigned char *dwm[1] = {d_m.as<unsigned char>()};
  must_refuse("load_refusals", "TraverseBatchesDevice", a.TraverseBatchesDevice(1, dwr, wn, dwi, dwm, NULL, NULL), a.LastBackendError());
  must_refuse("load_refusals", "OccludedBatchDevice", a.OccludedBatchDevice(d_rays.as<Ray<T> >(), n, d_m.as<unsigned char>(), NULL),
              a.LastBackendError());
  must_refuse("load_refusals", "MultiHitTraverseBatchDevice",
              a.MultiHitTraverseBatchDevice(d_rays.as<Ray<T> >(), n, 4, d_h.as<H>(), d_c.as<unsigned int>(), NULL), a.LastBackendError());
  hipDeviceSynchronize();
  check_tri("load_refusals after TraverseBatch", a, F.a, F.rays);  // (TraverseBatch runs first in the check)
  expect("load_refusals", "HipContext() once the loaded tree is on the device", a.HipContext() != NULL);
}

// four ray sets of one size: the camera rays four times over (a longer scatter: a wider window for the race this checks),
// rotated by a quarter each
template <typename T>
std::vector<std::vector<Ray<T> > > ray_sets(const std::vector<Ray<T> > &rays) {
  std::vector<std::vector<Ray<T> > > sets(4);
  for (size_t k = 0; k < 4; k++) {
    for (int r = 0; r < 4; r++) sets[k].insert(sets[k].end(), rays.begin(), rays.end());
    std::rotate(sets[k].begin(), sets[k].begin() + (k * sets[k].size()) / 4, sets[k].end());
    if (k & 1) std::reverse(sets[k].begin(), sets[k].end());
  }
  return sets;
}

// `objs[k]` traces set k from its own thread, `rounds` times; every result equals the serial one
template <typename T>
void threaded(const char *where, const std::vector<const BVHAccel<T> *> &objs, const std::vector<Ray<T> > &rays) {
  const std::vector<std::vector<Ray<T> > > sets = ray_sets(rays);
  std::vector<std::vector<nanort::TriangleIntersection<T> > > sh(4);
  std::vector<std::vector<unsigned char> > sm(4);
  for (int k = 0; k < 4; k++) {  // serial first: sizes every object's staging for this ray count
    bool ok = false;
    batch_records(*objs[k], sets[k], &sh[k], &sm[k], &ok);
    expect(where, "serial TraverseBatch", ok);
  }
  const int rounds = 24;
  std::vector<unsigned long long> bad(4, 0);
  std::vector<std::thread> pool;
  for (int k = 0; k < 4; k++)
    pool.push_back(std::thread([&, k]() {
      std::vector<nanort::TriangleIntersection<T> > h;
      std::vector<unsigned char> m;
      for (int r = 0; r < rounds; r++) {
        bool ok = false;
        batch_records(*objs[k], sets[k], &h, &m, &ok);
        bad[k] += !(ok && same_records(sh[k], sm[k], h, m));
      }
    }));
  for (size_t k = 0; k < pool.size(); k++) pool[k].join();
  for (int k = 0; k < 4; k++) tally(where, "concurrent TraverseBatch == serial", bad[k]);
}

template <typename T>
void threads_same_object() {
  Fixture<T> F;
  BVHAccel<T> a;
  BUILD(build_tri(&a, F.a));
  check_tri("threads_same_object", a, F.a, F.rays);
  threaded<T>("threads_same_object", std::vector<const BVHAccel<T> *>(4, &a), F.rays);
}

template <typename T>
void threads_copies() {
  Fixture<T> F;
  BVHAccel<T> a;
  BUILD(build_tri(&a, F.a));
  std::vector<BVHAccel<T> > copies(4, a);
  for (int k = 0; k < 4; k++) check_tri("threads_copies", copies[k], F.a, F.rays);
  threaded<T>("threads_copies", std::vector<const BVHAccel<T> *>{&copies[0], &copies[1], &copies[2], &copies[3]}, F.rays);
}

void replicas_prims(float) {
  copy_then_kind_change();
  copy_cyl_cap_flip();
}
void replicas_prims(double) {}

// every copy / move scenario again with one replica of each tree on a second context (NANORT_HIP_DEVICES=0,0): the peers
// are shared by copies too
template <typename T>
void replicas() {
  setenv("NANORT_HIP_DEVICES", "0,0", 1);
  {
    Fixture<T> F;
    BVHAccel<T> a;
    BUILD(build_tri(&a, F.a));
    expect("replicas", "two contexts (NumHipDevices() == 2)", a.NumHipDevices() == 2);
  }
  copy_then_rebuild_copy<T>(NULL);
  copy_then_rebuild_original<T>();
  copy_then_load<T>();
  move<T>();
  vector_growth<T>();
  threads_copies<T>();
  replicas_prims(T());
}

// Build, move-construct, move-assign, copy, then the copied object onto contexts of its own; after every step every live
// object: the moved-from ones refuse (4 queries each), the others equal their own host walk.
template <typename T>
void motion_masks() {
  MotionFixture<T> F;
  const unsigned int nf = F.k0.nf;
  const unsigned int *masks = g_in.masks.data(), *other = g_in.masks2.data();
  BVHAccel<T> a;
  BUILD(a.Build(nf, F.mesh(), F.pred()));
  BUILD(a.SetPrimMasks(masks, nf));
  check_motion("motion_masks built", a, F, masks);
  BVHAccel<T> b(std::move(a));
  expect("motion_masks", "moved-from source: IsValid() == false", !a.IsValid());
  check_motion_refused("motion_masks moved-from (constructed)", a, F);
  check_motion("motion_masks move-constructed", b, F, masks);
  BVHAccel<T> c;
  c = std::move(b);
  check_motion_refused("motion_masks moved-from (constructed), after the assignment", a, F);
  check_motion_refused("motion_masks moved-from (assigned)", b, F);
  check_motion("motion_masks move-assigned", c, F, masks);
  BVHAccel<T> d(c);
  expect("motion_masks", "a copy shares the original's context until one of them changes it", d.HipContext() == c.HipContext());
  check_motion("motion_masks copied-from", c, F, masks);
  check_motion("motion_masks copy", d, F, masks);
  BUILD(c.SetPrimMasks(other, nf));  // the copied-from object moves to contexts of its own: both keyframes and the new words go along
  expect("motion_masks", "SetPrimMasks() on a shared context detaches", d.HipContext() != c.HipContext() && c.HipContext() != NULL);
  check_motion("motion_masks copied-from, other masks", c, F, other);
  check_motion("motion_masks copy, its own masks", d, F, masks);
  check_motion_refused("motion_masks moved-from (constructed), after the detach", a, F);
  check_motion_refused("motion_masks moved-from (assigned), after the detach", b, F);
  BUILD(c.Build(nf, F.mesh(), F.pred()));  // a Build() drops the masks: the two masked queries refuse
  check_motion("motion_masks rebuilt", c, F, NULL);
  check_motion("motion_masks copy after the rebuild", d, F, masks);
  BVHAccel<T> e(d);
  BUILD(e.SetPrimMasks(other, nf));  // ... and the COPY is the one that detaches, from what it was given by the copy
  check_motion("motion_masks second copy, other masks", e, F, other);
  check_motion("motion_masks copy, still its own masks", d, F, masks);
}

// The same for a curve accel; the argument change is the subdivision count, 4 and then 2.
void curve_subdiv() {
  BVHAccel<float> a;
  BUILD(build_crv(&a));
  check_crv("curve_subdiv built", a, 4);
  BVHAccel<float> b(std::move(a));
  expect("curve_subdiv", "moved-from source: IsValid() == false", !a.IsValid());
  check_crv_refused("curve_subdiv moved-from (constructed)", a);
  check_crv("curve_subdiv move-constructed", b, 4);
  BVHAccel<float> c;
  c = std::move(b);
  check_crv_refused("curve_subdiv moved-from (constructed), after the assignment", a);
  check_crv_refused("curve_subdiv moved-from (assigned)", b);
  check_crv("curve_subdiv move-assigned", c, 4);
  BVHAccel<float> d(c);
  check_crv("curve_subdiv copied-from", c, 4);
  check_crv("curve_subdiv copy", d, 4);
  check_crv("curve_subdiv copied-from, 2 subdivisions", c, 2);  // moves to contexts of its own, the curves sent with the new count
  expect("curve_subdiv", "a new subdivision count on a shared context detaches", d.HipContext() != c.HipContext() && c.HipContext() != NULL);
  check_crv("curve_subdiv copy, still 4", d, 4);
  check_crv("curve_subdiv copied-from, 2 again", c, 2);
  check_crv_refused("curve_subdiv moved-from (constructed), after the detach", a);
  check_crv_refused("curve_subdiv moved-from (assigned), after the detach", b);
  check_crv("curve_subdiv copied-from, back to 4", c, 4);
  check_crv("curve_subdiv copy, 2 (no copy left to keep apart: a re-send)", d, 2);
}

// ---- --fixture: what the scenes of the two scenarios above can tell apart, on the host alone ----
struct HostCurvePred : nanort::BezierCurvePred {
  explicit HostCurvePred(const float *cps) : nanort::BezierCurvePred(cps) {}
};
template <typename T>
void fixture_motion(const char *prec) {
  typedef nanort::TriangleIntersection<T> H;
  MotionFixture<T> F;
  BVHAccel<T> a;  // (a predicate of another type: the host builder, over keyframe 0; the host refit makes the boxes hold keyframe 1 too)
  BUILD(a.Build(F.k0.nf, F.k0.tm(), HostPred<T>(F.k0.v.data(), F.k0.f.data(), sizeof(T) * 3)));
  BUILD(a.Refit(F.mesh()));
  std::vector<H> h0, h5, hp, hk, ho;
  std::vector<unsigned char> m0, m5, mp, mk, mo;
  host_records(a, F.rays, F.at_time(), [&](const nanort::MotionTriangleIntersector<T> &x, size_t) { x.SetTime(T(0)); }, &h0, &m0);
  host_records(a, F.rays, F.at_time(), [&](const nanort::MotionTriangleIntersector<T> &x, size_t i) { x.SetTime(F.times[i]); }, &h5, &m5);
  host_records(a, F.rays, F.masked(NULL), [&](const nanort::MaskedTriangleIntersector<T> &x, size_t) { x.SetRayMask(0xFFFFFFFFu); }, &hp, &mp);
  host_records(a, F.rays, F.masked(g_in.masks.data()), [&](const nanort::MaskedTriangleIntersector<T> &x, size_t i) { x.SetRayMask(F.ray_masks[i]); }, &hk, &mk);
  host_records(a, F.rays, F.masked(g_in.masks2.data()), [&](const nanort::MaskedTriangleIntersector<T> &x, size_t i) { x.SetRayMask(F.ray_masks[i]); }, &ho, &mo);
  const double n = static_cast<double>(F.rays.size());
  printf("fixture motion %s rays %zu faces %u time %.4f masks %.4f other_masks %.4f\n", prec, F.rays.size(), F.k0.nf, records_differ(h5, m5, h0, m0) / n,
         records_differ(hk, mk, hp, mp) / n, records_differ(ho, mo, hk, mk) / n);
}
void fixture_curves() {
  BVHAccel<float> a;
  nanort::BVHBuildOptions<float> o;
  o.cache_bbox = false;
  BUILD(a.Build(g_in.nk, nanort::BezierCurveGeometry(g_in.kc.data(), g_in.kr.data()), HostCurvePred(g_in.kc.data()), o));
  std::vector<nanort::BezierCurveIntersection> h2, h4;
  std::vector<unsigned char> m2, m4;
  host_curves(a, 2, &h2, &m2);
  host_curves(a, 4, &h4, &m4);
  size_t differ = 0, hit = 0;
  for (size_t i = 0; i < h2.size(); i++) {
    differ += m2[i] != m4[i] || memcmp(static_cast<const void *>(&h2[i]), static_cast<const void *>(&h4[i]), sizeof(h2[i])) != 0;
    hit += m2[i] || m4[i];
  }
  printf("fixture curves rays %zu curves %u subdivisions %.4f hit %.4f\n", h2.size(), g_in.nk, differ / static_cast<double>(h2.size()),
         hit / static_cast<double>(h2.size()));
}

struct Scenario {
  const char *name;
  bool f64;  // also runs with T = double
  void (*f32)(const char *);
  void (*f64fn)(const char *);
};
#define SC(fn) [](const char *) { fn<float>(); }, [](const char *) { fn<double>(); }
const Scenario kScenarios[] = {
    {"batch_first", true, SC(batch_first)},
    {"cyl_cap_first", false, [](const char *) { cyl_cap_first(); }, NULL},
    {"copy_then_rebuild_copy", true, [](const char *o) { copy_then_rebuild_copy<float>(o); }, [](const char *o) { copy_then_rebuild_copy<double>(o); }},
    {"copy_then_rebuild_original", true, SC(copy_then_rebuild_original)},
    {"copy_then_kind_change", false, [](const char *) { copy_then_kind_change(); }, NULL},
    {"copy_then_load", true, SC(copy_then_load)},
    {"copy_cyl_cap_flip", false, [](const char *) { copy_cyl_cap_flip(); }, NULL},
    {"move", true, SC(move)},
    {"vector_growth", true, SC(vector_growth)},
    {"kind_cycle", false, [](const char *) { kind_cycle(); }, NULL},
    {"empty_rebuild", true, SC(empty_rebuild)},
    {"load_refusals", true, SC(load_refusals)},
    {"threads_same_object", true, SC(threads_same_object)},
    {"threads_copies", true, SC(threads_copies)},
    {"replicas", true, SC(replicas)},
    {"motion_masks", true, SC(motion_masks)},
    {"curve_subdiv", false, [](const char *) { curve_subdiv(); }, NULL},
};

}  // namespace

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "--list")) {  // (no HIP call on this path: it runs where there is no GPU)
    for (const Scenario &s : kScenarios) printf("%s %s\n", s.name, s.f64 ? "f32,f64" : "f32");
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "--fixture")) {  // (host classes only: no HIP call on this path either)
    if (!read_inputs(argv[2])) {
      fprintf(stderr, "cannot read the inputs in %s\n", argv[2]);
      return 2;
    }
    fixture_motion<float>("f32");
    fixture_motion<double>("f64");
    fixture_curves();
    return 0;
  }
  if (argc < 4 || (strcmp(argv[2], "f32") && strcmp(argv[2], "f64"))) {
    fprintf(stderr, "usage: accel_lifecycle_check --list | --fixture DIR | SCENARIO f32|f64 DIR [OUT]\n");
    return 64;
  }
  const bool f64 = !strcmp(argv[2], "f64");
  for (const Scenario &s : kScenarios) {
    if (strcmp(s.name, argv[1])) continue;
    if (f64 && !s.f64) {
      fprintf(stderr, "%s: fp32 only\n", s.name);
      return 64;
    }
    g_dir = argv[3];
    if (!read_inputs(g_dir)) {
      fprintf(stderr, "cannot read the inputs in %s\n", argv[3]);
      return 2;
    }
    (f64 ? s.f64fn : s.f32)(argc > 4 ? argv[4] : NULL);
    printf("scenario %s checks %llu mismatches %llu refused %llu\n", s.name, g.checks, g.mismatches, g.refused);
    return g.mismatches ? 1 : 0;
  }
  fprintf(stderr, "unknown scenario %s (--list)\n", argv[1]);
  return 64;
}

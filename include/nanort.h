// include/nanort.h — header-only host side of the MI355X ray-tracing kernel.
//
// API-compatible with lighttransport/nanort's `nanort.h` for the hot path
// (BVHAccel<T>::Build / Traverse with Ray, BVHNode, TriangleMesh,
// TriangleSAHPred, TriangleIntersector<>, TriangleIntersection and the option
// structs), so the reference's examples (path_tracer, objrender,
// double_precision, the regression program, the custom-primitive demos)
// compile against it unchanged.  It is written from scratch: only names,
// argument meaning, struct layouts and result semantics follow the reference
// (cited as `ref nanort.h:LINE`).
//
// Two execution paths:
//
//   * Generic host path — any Prim / Pred / Intersector that satisfies the
//     reference's concepts (ref nanort.h:716-718, 757-759).  Needed for custom
//     primitives and for the per-ray Traverse() the reference API exposes.
//
//   * NANORT_USE_HIP_BACKEND — when Build() is called with the built-in
//     TriangleMesh<T> + TriangleSAHPred<T>, construction runs on the GPU through
//     the C ABI of libnanort_hip.so (include/nanort_hip.h): the node array and
//     index permutation stay on the device and are copied into nodes_/indices_
//     by the first host access, so GetNodes(), Dump(), BoundingBox() and the
//     per-ray Traverse() keep working while an application that only calls
//     TraverseBatch() never pays the read-back.  The one
//     API addition, TraverseBatch(), intersects N rays in one GPU launch; it
//     does not exist without the backend (there is no CPU stand-in for it).
//     Link with -lnanort_hip.
//
// Macros accepted for source compatibility: NANORT_USE_CPP11_FEATURE,
// NANORT_ENABLE_PARALLEL_BUILD (with OpenMP or NANORT_USE_CPP11_FEATURE the generic
// host build of user primitives runs in parallel and yields the same tree as the serial
// one; the built-in primitive types build on the GPU), NANORT_ENABLE_SERIALIZATION.
#ifndef NANORT_H_
#define NANORT_H_

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <queue>
#include <string>
#include <type_traits>
#include <vector>

#include "nanort_motion.h"  // the motion-blur vertex rule (MotionTriangleIntersector), shared with the device walk
#include "nanort_closest.h"  // the closest-point rule (BVHAccel::ClosestPoint), shared with the device kernel
#include "nanort_sdf.h"      // the signed-distance rule (BVHAccel::SignedDistance, FeatureNormals), shared with the device kernels
#ifdef NANORT_USE_HIP_BACKEND
#include <mutex>

#include "nanort_hip.h"
#endif
#ifdef _OPENMP
#include <omp.h>
#endif
#ifdef __linux__
#include <sched.h>  // sched_getaffinity: the CPUs this process may run on (detail::HostThreads)
#endif

#define kNANORT_MAX_STACK_DEPTH (512)
#define kNANORT_MIN_PRIMITIVES_FOR_PARALLEL_BUILD (1024 * 8)
#define kNANORT_SHALLOW_DEPTH (4)
#ifdef NANORT_USE_CPP11_FEATURE
// the reference's header pulls these in under this macro and its examples rely on that
#include <atomic>
#include <mutex>
#include <thread>
#define kNANORT_MAX_THREADS (256)
#ifndef NANORT_ENABLE_PARALLEL_BUILD
#define NANORT_ENABLE_PARALLEL_BUILD
#endif
#endif

namespace nanort {

namespace detail {

// Worker threads for the host-side loops of this header (the parallel host build, the hit scatter of TraverseBatch):
// what the process may actually use — the cgroup CPU quota when there is one (an OpenMP default of "every hardware
// thread" inside a quota'd container collapses, and starves the HIP runtime's own threads), else the OpenMP / hardware
// thread count, and never more than the CPUs of the process's affinity mask (taskset, cpusets: hardware_concurrency()
// counts every online CPU of the machine) — clamped to [1, 64].
inline unsigned int HostThreadsUncached() {
  unsigned int n = 1;
#if defined(_OPENMP)
  n = static_cast<unsigned int>(std::max(1, omp_get_max_threads()));
#elif defined(NANORT_USE_CPP11_FEATURE)
  n = std::max(1u, std::thread::hardware_concurrency());
#endif
  long quota = -1, period = 0;
  if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota|max> <period>"
    char q[32];
    if (std::fscanf(f, "%31s %ld", q, &period) == 2 && std::strcmp(q, "max") != 0) quota = std::atol(q);
    std::fclose(f);
  } else if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {  // cgroup v1
    if (std::fscanf(g, "%ld", &quota) != 1) quota = -1;
    std::fclose(g);
    if (FILE *h = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
      if (std::fscanf(h, "%ld", &period) != 1) period = 0;
      std::fclose(h);
    }
  }
  if (quota > 0 && period > 0 && static_cast<unsigned long>(quota / period) >= 1 && static_cast<unsigned long>(quota / period) < n)
    n = static_cast<unsigned int>(quota / period);
#if defined(__linux__) && defined(CPU_COUNT)
  cpu_set_t allowed;
  CPU_ZERO(&allowed);
  if (sched_getaffinity(0, sizeof(allowed), &allowed) == 0 && CPU_COUNT(&allowed) >= 1 && static_cast<unsigned int>(CPU_COUNT(&allowed)) < n)
    n = static_cast<unsigned int>(CPU_COUNT(&allowed));
#endif
  return std::min(64u, std::max(1u, n));
}
inline unsigned int HostThreads() {
  static const unsigned int cached = HostThreadsUncached();  // (function-local static: initialised once, thread-safely)
  return cached;
}

// f(i) for i in [0, n) on up to `threads` workers, dynamically scheduled; serial when the header was compiled without
// OpenMP and without NANORT_USE_CPP11_FEATURE (the reference's two ways of building in parallel, nanort.h:2018-2117).
template <class F>
inline void ParallelFor(unsigned int n, unsigned int threads, const F &f) {
  if (threads > n) threads = n;
#if defined(_OPENMP)
  if (threads > 1) {
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long long i = 0; i < static_cast<long long>(n); i++) f(static_cast<unsigned int>(i));
    return;
  }
#elif defined(NANORT_USE_CPP11_FEATURE)
  if (threads > 1) {
    std::atomic<unsigned int> next(0);
    std::vector<std::thread> pool;
    for (unsigned int t = 0; t < threads; t++)
      pool.push_back(std::thread([&]() {
        for (unsigned int i = next++; i < n; i = next++) f(i);
      }));
    for (size_t t = 0; t < pool.size(); t++) pool[t].join();
    return;
  }
#endif
  for (unsigned int i = 0; i < n; i++) f(i);
}

}  // namespace detail


typedef enum {
  RAY_TYPE_NONE = 0x0,
  RAY_TYPE_PRIMARY = 0x1,
  RAY_TYPE_SECONDARY = 0x2,
  RAY_TYPE_DIFFUSE = 0x4,
  RAY_TYPE_REFLECTION = 0x8,
  RAY_TYPE_REFRACTION = 0x10
} RayType;

// ---------------------------------------------------------------------------
// Small vector with the access idiom the reference's two-level traversal uses
// (`(*v)->clear()`, `v->size()`, `v[i]`; ref nanort.h:134-317, 784).  Capacity
// is reserved up front so the common case never reallocates.
// ---------------------------------------------------------------------------
template <typename TElem, size_t stack_capacity>
class StackVector {
 public:
  typedef std::vector<TElem> ContainerType;
  StackVector() { items_.reserve(stack_capacity); }
  StackVector(const StackVector &rhs) : items_(rhs.items_) { items_.reserve(stack_capacity); }
  StackVector &operator=(const StackVector &rhs) {
    items_ = rhs.items_;
    return *this;
  }
  ContainerType &container() { return items_; }
  const ContainerType &container() const { return items_; }
  ContainerType *operator->() { return &items_; }
  const ContainerType *operator->() const { return &items_; }
  TElem &operator[](size_t i) { return items_[i]; }
  const TElem &operator[](size_t i) const { return items_[i]; }

 private:
  ContainerType items_;
};

// ---------------------------------------------------------------------------
// 3-vector and helpers (ref nanort.h:321-472)
// ---------------------------------------------------------------------------
template <typename T = float>
class real3 {
 public:
  real3() {}
  real3(T s) { v[0] = v[1] = v[2] = s; }
  real3(T a, T b, T c) {
    v[0] = a;
    v[1] = b;
    v[2] = c;
  }
  explicit real3(const T *p) {
    v[0] = p[0];
    v[1] = p[1];
    v[2] = p[2];
  }
  T x() const { return v[0]; }
  T y() const { return v[1]; }
  T z() const { return v[2]; }
  real3 operator*(T s) const { return real3(v[0] * s, v[1] * s, v[2] * s); }
  real3 operator*(const real3 &o) const { return real3(v[0] * o.v[0], v[1] * o.v[1], v[2] * o.v[2]); }
  real3 operator/(const real3 &o) const { return real3(v[0] / o.v[0], v[1] / o.v[1], v[2] / o.v[2]); }
  real3 operator+(const real3 &o) const { return real3(v[0] + o.v[0], v[1] + o.v[1], v[2] + o.v[2]); }
  real3 operator-(const real3 &o) const { return real3(v[0] - o.v[0], v[1] - o.v[1], v[2] - o.v[2]); }
  real3 operator-() const { return real3(-v[0], -v[1], -v[2]); }
  real3 &operator+=(const real3 &o) {
    v[0] += o.v[0];
    v[1] += o.v[1];
    v[2] += o.v[2];
    return *this;
  }
  T operator[](int i) const { return v[i]; }
  T &operator[](int i) { return v[i]; }

  T v[3];
};

template <typename T>
inline real3<T> operator*(T s, const real3<T> &a) {
  return real3<T>(a[0] * s, a[1] * s, a[2] * s);
}
template <typename T>
inline real3<T> vneg(const real3<T> &a) {
  return real3<T>(-a[0], -a[1], -a[2]);
}
template <typename T>
inline T vdot(const real3<T> a, const real3<T> b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
template <typename T>
inline T vlength(const real3<T> &a) {
  return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
}
template <typename T>
inline real3<T> vnormalize(const real3<T> &a) {
  real3<T> r = a;
  const T len = vlength(a);
  if (std::fabs(len) > std::numeric_limits<T>::epsilon()) {
    const T inv = static_cast<T>(1.0) / len;
    r[0] *= inv;
    r[1] *= inv;
    r[2] *= inv;
  }
  return r;
}
template <typename T>
inline real3<T> vcross(const real3<T> a, const real3<T> b) {
  return real3<T>(a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]);
}

// Reciprocal that maps near-zero components to a signed infinity
// (ref nanort.h:414-465; both sign rules of the reference are kept).
template <typename T>
inline real3<T> vsafe_inverse(const real3<T> d) {
  real3<T> r;
  for (int k = 0; k < 3; k++) {
    if (std::fabs(d[k]) < std::numeric_limits<T>::epsilon()) {
#ifdef NANORT_USE_CPP11_FEATURE
      r[k] = std::numeric_limits<T>::infinity() * std::copysign(static_cast<T>(1), d[k]);
#else
      r[k] = std::numeric_limits<T>::infinity() * ((d[k] < static_cast<T>(0)) ? static_cast<T>(-1) : static_cast<T>(1));
#endif
    } else {
      r[k] = static_cast<T>(1.0) / d[k];
    }
  }
  return r;
}

template <typename real>
inline const real *get_vertex_addr(const real *p, const size_t idx, const size_t stride_bytes) {
  return reinterpret_cast<const real *>(reinterpret_cast<const unsigned char *>(p) + idx * stride_bytes);
}

// Comparison-based min/max that drop a NaN first argument (ref nanort.h:1236-1243).
template <class T>
const T &safemin(const T &a, const T &b) {
  return (a < b) ? a : b;
}
template <class T>
const T &safemax(const T &a, const T &b) {
  return (a > b) ? a : b;
}

// ---------------------------------------------------------------------------
// Wire-format PODs (layouts pinned below; ref nanort.h:474-639)
// ---------------------------------------------------------------------------
template <typename T = float>
class Ray {
 public:
  Ray() : min_t(static_cast<T>(0.0)), max_t(std::numeric_limits<T>::max()), type(RAY_TYPE_NONE) {
    org[0] = org[1] = org[2] = static_cast<T>(0.0);
    dir[0] = dir[1] = static_cast<T>(0.0);
    dir[2] = static_cast<T>(-1.0);
  }
  T org[3];
  T dir[3];
  T min_t;
  T max_t;
  unsigned int type;
};

template <typename T = float>
class BVHNode {
 public:
  BVHNode() {}
  T bmin[3];
  T bmax[3];
  int flag;  // 1 = leaf, 0 = branch
  int axis;
  // leaf: {primitive count, first slot in the index array}; branch: {low child, high child}
  unsigned int data[2];
};

template <class H>
class IntersectComparator {
 public:
  bool operator()(const H &a, const H &b) const { return a.t < b.t; }
};

template <typename T = float>
struct BVHBuildOptions {
  T cost_t_aabb;
  unsigned int min_leaf_primitives;
  unsigned int max_tree_depth;
  unsigned int bin_size;
  unsigned int shallow_depth;
  unsigned int min_primitives_for_parallel_build;
  bool cache_bbox;
  unsigned char pad[3];
  BVHBuildOptions()
      : cost_t_aabb(static_cast<T>(0.2)),
        min_leaf_primitives(4),
        max_tree_depth(256),
        bin_size(64),
        shallow_depth(kNANORT_SHALLOW_DEPTH),
        min_primitives_for_parallel_build(kNANORT_MIN_PRIMITIVES_FOR_PARALLEL_BUILD),
        cache_bbox(false) {
    pad[0] = pad[1] = pad[2] = 0;
  }
};

class BVHBuildStatistics {
 public:
  unsigned int max_tree_depth;
  unsigned int num_leaf_nodes;
  unsigned int num_branch_nodes;
  float build_secs;
  BVHBuildStatistics() : max_tree_depth(0), num_leaf_nodes(0), num_branch_nodes(0), build_secs(0.0f) {}
};

class BVHTraceOptions {
 public:
  unsigned int prim_ids_range[2];  // half-open [first, last)
  unsigned int skip_prim_id;       // 0xFFFFFFFF: skip nothing
  bool cull_back_face;
  unsigned char pad[3];
  BVHTraceOptions() {
    prim_ids_range[0] = 0;
    prim_ids_range[1] = 0x7FFFFFFF;
    skip_prim_id = static_cast<unsigned int>(-1);
    cull_back_face = false;
    pad[0] = pad[1] = pad[2] = 0;
  }
};

template <typename T>
class BBox {
 public:
  real3<T> bmin;
  real3<T> bmax;
  BBox() {
    bmin[0] = bmin[1] = bmin[2] = std::numeric_limits<T>::max();
    bmax[0] = bmax[1] = bmax[2] = -std::numeric_limits<T>::max();
  }
};

template <typename T>
class NodeHit {
 public:
  NodeHit()
      : t_min(std::numeric_limits<T>::max()), t_max(-std::numeric_limits<T>::max()), node_id(static_cast<unsigned int>(-1)) {}
  T t_min;
  T t_max;
  unsigned int node_id;
};

template <typename T>
class NodeHitComparator {
 public:
  inline bool operator()(const NodeHit<T> &a, const NodeHit<T> &b) { return a.t_min < b.t_min; }
};

// ---------------------------------------------------------------------------
// Built-in triangle plugin
// ---------------------------------------------------------------------------

// Partition predicate (ref nanort.h:863-919): sum of the three vertex
// coordinates on `axis` against 3*pos.
template <typename T = float>
class TriangleSAHPred {
 public:
  TriangleSAHPred(const T *vertices, const unsigned int *faces, size_t vertex_stride_bytes)
      : axis_(0), pos_(static_cast<T>(0.0)), vertices_(vertices), faces_(faces), vertex_stride_bytes_(vertex_stride_bytes) {}
  TriangleSAHPred(const TriangleSAHPred<T> &o)
      : axis_(o.axis_), pos_(o.pos_), vertices_(o.vertices_), faces_(o.faces_), vertex_stride_bytes_(o.vertex_stride_bytes_) {}
  TriangleSAHPred<T> &operator=(const TriangleSAHPred<T> &o) {
    axis_ = o.axis_;
    pos_ = o.pos_;
    vertices_ = o.vertices_;
    faces_ = o.faces_;
    vertex_stride_bytes_ = o.vertex_stride_bytes_;
    return *this;
  }
  void Set(int axis, T pos) const {
    axis_ = axis;
    pos_ = pos;
  }
  bool operator()(unsigned int i) const {
    const int a = axis_;
    const T s = get_vertex_addr<T>(vertices_, faces_[3 * i + 0], vertex_stride_bytes_)[a] +
                get_vertex_addr<T>(vertices_, faces_[3 * i + 1], vertex_stride_bytes_)[a] +
                get_vertex_addr<T>(vertices_, faces_[3 * i + 2], vertex_stride_bytes_)[a];
    return s < pos_ * static_cast<T>(3.0);
  }
  const T *GetVertices() const { return vertices_; }
  const unsigned int *GetFaces() const { return faces_; }
  size_t GetVertexStrideBytes() const { return vertex_stride_bytes_; }

 private:
  mutable int axis_;
  mutable T pos_;
  const T *vertices_;
  const unsigned int *faces_;
  size_t vertex_stride_bytes_;
};

// Primitive accessor (ref nanort.h:922-991).  Carries no vertex count.
template <typename T = float>
class TriangleMesh {
 public:
  TriangleMesh(const T *vertices, const unsigned int *faces, const size_t vertex_stride_bytes)
      : vertices_(vertices), faces_(faces), vertex_stride_bytes_(vertex_stride_bytes) {}

  void BoundingBox(real3<T> *bmin, real3<T> *bmax, unsigned int prim_index) const {
    const T *p = get_vertex_addr<T>(vertices_, faces_[3 * prim_index], vertex_stride_bytes_);
    for (int k = 0; k < 3; k++) (*bmin)[k] = (*bmax)[k] = p[k];
    for (unsigned int c = 1; c < 3; c++) {
      p = get_vertex_addr<T>(vertices_, faces_[3 * prim_index + c], vertex_stride_bytes_);
      for (int k = 0; k < 3; k++) {
        (*bmin)[k] = std::min((*bmin)[k], p[k]);
        (*bmax)[k] = std::max((*bmax)[k], p[k]);
      }
    }
  }

  void BoundingBoxAndCenter(real3<T> *bmin, real3<T> *bmax, real3<T> *center, unsigned int prim_index) const {
    const real3<T> a(get_vertex_addr<T>(vertices_, faces_[3 * prim_index + 0], vertex_stride_bytes_));
    const real3<T> b(get_vertex_addr<T>(vertices_, faces_[3 * prim_index + 1], vertex_stride_bytes_));
    const real3<T> c(get_vertex_addr<T>(vertices_, faces_[3 * prim_index + 2], vertex_stride_bytes_));
    for (int k = 0; k < 3; k++) {
      (*bmin)[k] = std::min(a[k], std::min(b[k], c[k]));
      (*bmax)[k] = std::max(a[k], std::max(b[k], c[k]));
    }
    *center = (a + b + c) * (T(1) / T(3));
  }

  const T *GetVertices() const { return vertices_; }
  const unsigned int *GetFaces() const { return faces_; }
  size_t GetVertexStrideBytes() const { return vertex_stride_bytes_; }

  const T *vertices_;
  const unsigned int *faces_;
  const size_t vertex_stride_bytes_;
};

template <typename T = float>
class TriangleIntersection {
 public:
  T u;
  T v;
  T t;
  unsigned int prim_id;
};

// The answer of BVHAccel::ClosestPoint() / ClosestPointBatch() (no reference counterpart; laid out as nrt_closest_f32 / _f64 of
// include/nanort_hip.h): the nearest point of the mesh, its squared distance, its barycentrics on face prim_id (u weighs the
// face's second vertex and v its third, as in TriangleIntersection).  Nothing within max_dist: point = the query point,
// dist2 = max_dist * max_dist, u = v = 0, prim_id = 0xFFFFFFFF.
template <typename T = float>
class ClosestPointResult {
 public:
  T point[3];
  T dist2;
  T u;
  T v;
  unsigned int prim_id;
  unsigned int pad;
};

// The answer of BVHAccel::SignedDistance() / SignedDistanceBatch() (laid out as nrt_signed_f32 / _f64): a ClosestPointResult with
// `feature` in the place of `pad` — bits 0..2 the feature of face prim_id that holds the nearest point (0 its interior, 1 / 2 / 3 the
// edge ab / ac / bc, 4 / 5 / 6 the vertex a / b / c), bit 31 set exactly when the query point is inside; 0 when nothing was found.
template <typename T = float>
class SignedDistanceResult {
 public:
  T point[3];
  T dist2;
  T u;
  T v;
  unsigned int prim_id;
  unsigned int feature;
  bool Inside() const { return (feature & nanort_sdf::kInsideBit) != 0u; }
  unsigned int Feature() const { return feature & nanort_sdf::kFeatureMask; }
  // The distance with its sign: negative inside.
  T Signed() const { return Inside() ? -std::sqrt(dist2) : std::sqrt(dist2); }
};

// Watertight ray/triangle test (Woop, Benthin, Wald 2013), same operation
// order and tie rules as the reference's intersector (ref nanort.h:1014-1229):
// edge functions recomputed from double products when one of them is exactly
// zero; a candidate replaces the current hit when its t is <= the best t and
// >= the ray's min_t.
template <typename T = float, class H = TriangleIntersection<T> >
class TriangleIntersector {
 public:
  template <class M>
  TriangleIntersector(const M &m) : vertices_(m.GetVertices()), faces_(m.GetFaces()), vertex_stride_bytes_(m.GetVertexStrideBytes()) {}
  template <class M>
  TriangleIntersector(const M *m) : vertices_(m->GetVertices()), faces_(m->GetFaces()), vertex_stride_bytes_(m->GetVertexStrideBytes()) {}
  TriangleIntersector(const T *vertices, const unsigned int *faces, const size_t vertex_stride_bytes)
      : vertices_(vertices), faces_(faces), vertex_stride_bytes_(vertex_stride_bytes) {}

  typedef struct {
    T Sx, Sy, Sz;
    int kx, ky, kz;
  } RayCoeff;

  bool Intersect(T *t_inout, const unsigned int prim_index) const {
    if (prim_index < trace_options_.prim_ids_range[0] || prim_index >= trace_options_.prim_ids_range[1]) return false;
    if (prim_index == trace_options_.skip_prim_id) return false;

    return IntersectVertices(t_inout, real3<T>(get_vertex_addr<T>(vertices_, faces_[3 * prim_index + 0], vertex_stride_bytes_)),
                             real3<T>(get_vertex_addr<T>(vertices_, faces_[3 * prim_index + 1], vertex_stride_bytes_)),
                             real3<T>(get_vertex_addr<T>(vertices_, faces_[3 * prim_index + 2], vertex_stride_bytes_)));
  }

  // THE arithmetic of the test, over the three corners wherever they come from (the mesh: Intersect above; two keyframes
  // interpolated to the ray's time: MotionTriangleIntersector).
  bool IntersectVertices(T *t_inout, const real3<T> &p0, const real3<T> &p1, const real3<T> &p2) const {
    const real3<T> A = p0 - ray_org_;
    const real3<T> B = p1 - ray_org_;
    const real3<T> C = p2 - ray_org_;
    const int kx = ray_coeff_.kx, ky = ray_coeff_.ky, kz = ray_coeff_.kz;

    const T Ax = A[kx] - ray_coeff_.Sx * A[kz], Ay = A[ky] - ray_coeff_.Sy * A[kz];
    const T Bx = B[kx] - ray_coeff_.Sx * B[kz], By = B[ky] - ray_coeff_.Sy * B[kz];
    const T Cx = C[kx] - ray_coeff_.Sx * C[kz], Cy = C[ky] - ray_coeff_.Sy * C[kz];

    T U = Cx * By - Cy * Bx;
    T V = Ax * Cy - Ay * Cx;
    T W = Bx * Ay - By * Ax;
    const T zero = static_cast<T>(0.0);
    if (U == zero || V == zero || W == zero) {
      U = static_cast<T>(static_cast<double>(Cx) * static_cast<double>(By) - static_cast<double>(Cy) * static_cast<double>(Bx));
      V = static_cast<T>(static_cast<double>(Ax) * static_cast<double>(Cy) - static_cast<double>(Ay) * static_cast<double>(Cx));
      W = static_cast<T>(static_cast<double>(Bx) * static_cast<double>(Ay) - static_cast<double>(By) * static_cast<double>(Ax));
    }
    if (U < zero || V < zero || W < zero) {
      if (trace_options_.cull_back_face || U > zero || V > zero || W > zero) return false;
    }
    const T det = U + V + W;
    if (det == zero) return false;

    const T Az = ray_coeff_.Sz * A[kz], Bz = ray_coeff_.Sz * B[kz], Cz = ray_coeff_.Sz * C[kz];
    const T D = U * Az + V * Bz + W * Cz;
    const T rcp_det = static_cast<T>(1.0) / det;
    const T tt = D * rcp_det;
    if (tt > (*t_inout)) return false;
    if (tt < t_min_) return false;
    (*t_inout) = tt;
    u_ = V * rcp_det;
    v_ = W * rcp_det;
    return true;
  }

  T GetT() const { return t_; }

  void Update(T t, unsigned int prim_idx) const {
    t_ = t;
    prim_id_ = prim_idx;
  }

  void PrepareTraversal(const Ray<T> &ray, const BVHTraceOptions &trace_options) const {
    ray_org_ = real3<T>(ray.org[0], ray.org[1], ray.org[2]);
    int kz = 0;
    T longest = std::fabs(ray.dir[0]);
    for (int k = 1; k < 3; k++) {
      if (longest < std::fabs(ray.dir[k])) {  // strict: ties keep the lower axis
        kz = k;
        longest = std::fabs(ray.dir[k]);
      }
    }
    int kx = (kz + 1) % 3, ky = (kz + 2) % 3;
    if (ray.dir[kz] < static_cast<T>(0.0)) std::swap(kx, ky);  // keep the winding
    ray_coeff_.kx = kx;
    ray_coeff_.ky = ky;
    ray_coeff_.kz = kz;
    ray_coeff_.Sx = ray.dir[kx] / ray.dir[kz];
    ray_coeff_.Sy = ray.dir[ky] / ray.dir[kz];
    ray_coeff_.Sz = static_cast<T>(1.0) / ray.dir[kz];
    trace_options_ = trace_options;
    t_min_ = ray.min_t;
    u_ = v_ = static_cast<T>(0.0);
  }

  void PostTraversal(const Ray<T> &ray, bool hit, H *isect) const {
    (void)ray;
    if (hit && isect) {
      isect->t = t_;
      isect->u = u_;
      isect->v = v_;
      isect->prim_id = prim_id_;
    }
  }

 protected:
  const T *vertices_;
  const unsigned int *faces_;
  const size_t vertex_stride_bytes_;
  mutable real3<T> ray_org_;
  mutable RayCoeff ray_coeff_;
  mutable BVHTraceOptions trace_options_;
  mutable T t_min_;
  mutable T t_;
  mutable T u_;
  mutable T v_;
  mutable unsigned int prim_id_;
};

// ---------------------------------------------------------------------------
// Motion blur: a triangle mesh with a second vertex keyframe (include/nanort_hip.h, "motion blur").  Host classes first: Build()
// over (MotionTriangleMesh, MotionTriangleSAHPred) and the per-ray Traverse() with a MotionTriangleIntersector whose SetTime()
// was called for the ray work without the backend.  With NANORT_USE_HIP_BACKEND the same Build() runs on the GPU
// (nrtSetMesh + nrtSetMeshMotion + nrtBuild) and TraverseBatchMotion() / OccludedBatchMotion() trace a batch with one time per ray.
// ---------------------------------------------------------------------------
// Primitive accessor: keyframe 0 and keyframe 1 share the faces and the stride.  A primitive's box is the union of the triangle
// rule's box on each keyframe, its SAH position the mean of the two keyframes' centres.
template <typename T = float>
class MotionTriangleMesh {
 public:
  MotionTriangleMesh(const T *vertices0, const T *vertices1, const unsigned int *faces, const size_t vertex_stride_bytes)
      : k0_(vertices0, faces, vertex_stride_bytes), k1_(vertices1, faces, vertex_stride_bytes) {}

  void BoundingBox(real3<T> *bmin, real3<T> *bmax, unsigned int prim_index) const {
    real3<T> lo1, hi1;
    k0_.BoundingBox(bmin, bmax, prim_index);
    k1_.BoundingBox(&lo1, &hi1, prim_index);
    for (int k = 0; k < 3; k++) {
      (*bmin)[k] = std::min((*bmin)[k], lo1[k]);
      (*bmax)[k] = std::max((*bmax)[k], hi1[k]);
    }
  }

  void BoundingBoxAndCenter(real3<T> *bmin, real3<T> *bmax, real3<T> *center, unsigned int prim_index) const {
    real3<T> lo1, hi1, c1;
    k0_.BoundingBoxAndCenter(bmin, bmax, center, prim_index);
    k1_.BoundingBoxAndCenter(&lo1, &hi1, &c1, prim_index);
    for (int k = 0; k < 3; k++) {
      (*bmin)[k] = std::min((*bmin)[k], lo1[k]);
      (*bmax)[k] = std::max((*bmax)[k], hi1[k]);
    }
    *center = (*center + c1) * T(0.5);
  }

  const T *GetVertices() const { return k0_.GetVertices(); }    // keyframe 0
  const T *GetVertices1() const { return k1_.GetVertices(); }   // keyframe 1
  const unsigned int *GetFaces() const { return k0_.GetFaces(); }
  size_t GetVertexStrideBytes() const { return k0_.GetVertexStrideBytes(); }

 private:
  TriangleMesh<T> k0_, k1_;
};

// Partition predicate: the primitive's SAH position (MotionTriangleMesh::BoundingBoxAndCenter) on `axis` against pos.
template <typename T = float>
class MotionTriangleSAHPred {
 public:
  MotionTriangleSAHPred(const T *vertices0, const T *vertices1, const unsigned int *faces, size_t vertex_stride_bytes)
      : axis_(0), pos_(static_cast<T>(0.0)), vertices0_(vertices0), vertices1_(vertices1), faces_(faces), vertex_stride_bytes_(vertex_stride_bytes) {}
  void Set(int axis, T pos) const {
    axis_ = axis;
    pos_ = pos;
  }
  bool operator()(unsigned int i) const {
    real3<T> lo, hi, c;
    MotionTriangleMesh<T>(vertices0_, vertices1_, faces_, vertex_stride_bytes_).BoundingBoxAndCenter(&lo, &hi, &c, i);
    return c[axis_] < pos_;
  }
  const T *GetVertices() const { return vertices0_; }
  const T *GetVertices1() const { return vertices1_; }
  const unsigned int *GetFaces() const { return faces_; }
  size_t GetVertexStrideBytes() const { return vertex_stride_bytes_; }

 private:
  mutable int axis_;
  mutable T pos_;
  const T *vertices0_;
  const T *vertices1_;
  const unsigned int *faces_;
  size_t vertex_stride_bytes_;
};

// TriangleIntersector over the two keyframes: the three corners are interpolated to the time last given to SetTime() by the shared
// rule (nanort_motion.h), then tested by TriangleIntersector's own arithmetic.  SetTime() before Traverse(), once per ray.
template <typename T = float, class H = TriangleIntersection<T> >
class MotionTriangleIntersector : public TriangleIntersector<T, H> {
  typedef TriangleIntersector<T, H> Base;

 public:
  template <class M>
  MotionTriangleIntersector(const M &m) : Base(m), vertices1_(m.GetVertices1()), shutter_(static_cast<T>(0.0)) {}
  MotionTriangleIntersector(const T *vertices0, const T *vertices1, const unsigned int *faces, const size_t vertex_stride_bytes)
      : Base(vertices0, faces, vertex_stride_bytes), vertices1_(vertices1), shutter_(static_cast<T>(0.0)) {}

  // The ray's time: clamped to [0, 1], NaN and negatives to 0.
  void SetTime(T time) const { shutter_ = nanort_motion::ClampTime<T>(time); }
  T GetShutterTime() const { return shutter_; }

  bool Intersect(T *t_inout, const unsigned int prim_index) const {
    if (prim_index < this->trace_options_.prim_ids_range[0] || prim_index >= this->trace_options_.prim_ids_range[1]) return false;
    if (prim_index == this->trace_options_.skip_prim_id) return false;
    real3<T> p[3];
    for (int c = 0; c < 3; c++) {
      const unsigned int vi = this->faces_[3 * prim_index + c];
      const T *a = get_vertex_addr<T>(this->vertices_, vi, this->vertex_stride_bytes_);
      const T *b = get_vertex_addr<T>(vertices1_, vi, this->vertex_stride_bytes_);
      for (int k = 0; k < 3; k++) p[c][k] = nanort_motion::Lerp<T>(a[k], b[k], shutter_);
    }
    return this->IntersectVertices(t_inout, p[0], p[1], p[2]);
  }

 private:
  const T *vertices1_;
  mutable T shutter_;
};

// Visibility masks (include/nanort_hip.h, "visibility masks"): a TriangleIntersector that holds one 32-bit word per primitive and the
// word of the ray being traced, and returns false from Intersect() for a primitive the ray does not see — (prim_mask & ray_mask)
// == 0 — before any of its arithmetic: the reference's template-filter mechanism, as data.  Works on the host without the backend;
// SetRayMask() before Traverse(), once per ray.  prim_masks == NULL: every primitive carries 0xFFFFFFFF.
template <typename T = float, class H = TriangleIntersection<T> >
class MaskedTriangleIntersector : public TriangleIntersector<T, H> {
  typedef TriangleIntersector<T, H> Base;

 public:
  template <class M>
  MaskedTriangleIntersector(const M &m, const unsigned int *prim_masks) : Base(m), prim_masks_(prim_masks), ray_mask_(0xFFFFFFFFu) {}
  MaskedTriangleIntersector(const T *vertices, const unsigned int *faces, const size_t vertex_stride_bytes, const unsigned int *prim_masks)
      : Base(vertices, faces, vertex_stride_bytes), prim_masks_(prim_masks), ray_mask_(0xFFFFFFFFu) {}

  void SetRayMask(unsigned int ray_mask) const { ray_mask_ = ray_mask; }
  unsigned int GetRayMask() const { return ray_mask_; }

  bool Intersect(T *t_inout, const unsigned int prim_index) const {
    if (((prim_masks_ ? prim_masks_[prim_index] : 0xFFFFFFFFu) & ray_mask_) == 0u) return false;
    return Base::Intersect(t_inout, prim_index);
  }

 private:
  const unsigned int *prim_masks_;
  mutable unsigned int ray_mask_;
};

// The three per-ray things at once (include/nanort_hip.h, "one descriptor for every triangle ray query"): a TriangleIntersector that
// holds, besides the mesh, a second vertex keyframe and one word per primitive — both optional — and of the ray being traced its
// time, its word and its skip id.  Intersect() returns false BEFORE ANY ARITHMETIC for a primitive the ray does not see
// ((prim_mask & ray_mask) == 0), one outside prim_ids_range, and the ray's skip id; the corners of every other primitive are
// interpolated to the ray's time by the shared rule (nanort_motion.h) when there is a keyframe 1 (none: keyframe 0 as stored) and
// tested by TriangleIntersector's own arithmetic.  SetRay() before Traverse(), once per ray; an intersector SetRay() was never
// called on traces at time 0 with the word 0xFFFFFFFF and the options' skip_prim_id.  Works on the host without the backend.
template <typename T = float, class H = TriangleIntersection<T> >
class QueryTriangleIntersector : public TriangleIntersector<T, H> {
  typedef TriangleIntersector<T, H> Base;

 public:
  // vertices1 == NULL: no motion; prim_masks == NULL: every primitive carries 0xFFFFFFFF
  QueryTriangleIntersector(const T *vertices0, const unsigned int *faces, const size_t vertex_stride_bytes, const T *vertices1 = NULL,
                           const unsigned int *prim_masks = NULL)
      : Base(vertices0, faces, vertex_stride_bytes), vertices1_(vertices1), prim_masks_(prim_masks), shutter_(static_cast<T>(0.0)),
        ray_mask_(0xFFFFFFFFu), skip_prim_id_(0xFFFFFFFFu), own_skip_(false) {}

  // The ray's time (clamped to [0, 1], NaN and negatives to 0), its visibility word, and its skip id — which takes the place of
  // the trace options' skip_prim_id for this ray (0xFFFFFFFF, or an id that names no primitive: nothing is skipped).
  void SetRay(T time, unsigned int ray_mask, unsigned int skip_prim_id) const {
    shutter_ = nanort_motion::ClampTime<T>(time);
    ray_mask_ = ray_mask;
    skip_prim_id_ = skip_prim_id;
    own_skip_ = true;
  }
  T GetShutterTime() const { return shutter_; }
  unsigned int GetRayMask() const { return ray_mask_; }

  bool Intersect(T *t_inout, const unsigned int prim_index) const {
    if (((prim_masks_ ? prim_masks_[prim_index] : 0xFFFFFFFFu) & ray_mask_) == 0u) return false;
    if (prim_index < this->trace_options_.prim_ids_range[0] || prim_index >= this->trace_options_.prim_ids_range[1]) return false;
    if (prim_index == (own_skip_ ? skip_prim_id_ : this->trace_options_.skip_prim_id)) return false;
    real3<T> p[3];
    for (int c = 0; c < 3; c++) {
      const unsigned int vi = this->faces_[3 * prim_index + c];
      const T *a = get_vertex_addr<T>(this->vertices_, vi, this->vertex_stride_bytes_);
      if (vertices1_) {
        const T *b = get_vertex_addr<T>(vertices1_, vi, this->vertex_stride_bytes_);
        for (int k = 0; k < 3; k++) p[c][k] = nanort_motion::Lerp<T>(a[k], b[k], shutter_);
      } else {
        for (int k = 0; k < 3; k++) p[c][k] = a[k];
      }
    }
    return this->IntersectVertices(t_inout, p[0], p[1], p[2]);
  }

 private:
  const T *vertices1_;
  const unsigned int *prim_masks_;
  mutable T shutter_;
  mutable unsigned int ray_mask_;
  mutable unsigned int skip_prim_id_;
  mutable bool own_skip_;
};

// What BVHAccel::TraverseBatchQuery() is asked for: a wave of rays and whichever of a time, a visibility word and a skip id each of
// them carries.  `motion` / `masked` say whether the keyframes are interpolated / the masks applied (times == NULL with motion:
// every ray at time 0; ray_masks == NULL with masked: every ray 0xFFFFFFFF; an array whose flag is off is not read).
// skip_prim_ids == NULL: options.skip_prim_id for every ray.  `occlusion`: only hit_out is written (required then), each ray
// stopping at the first triangle that settles it; otherwise EVERY record of isects is written — a miss stores {0, 0, ray.max_t,
// 0xFFFFFFFF} — and hit_out (optional) receives 1 / 0.
template <typename T = float>
struct BatchQuery {
  BatchQuery()
      : rays(NULL), num_rays(0), times(NULL), ray_masks(NULL), skip_prim_ids(NULL), motion(false), masked(false), occlusion(false), isects(NULL),
        hit_out(NULL) {}
  const Ray<T> *rays;
  size_t num_rays;
  const T *times;
  const unsigned int *ray_masks;
  const unsigned int *skip_prim_ids;
  bool motion, masked, occlusion;
  BVHTraceOptions options;
  TriangleIntersection<T> *isects;
  unsigned char *hit_out;
};

// What BVHAccel::MultiHitTraverseBatchQuery() is asked for: BatchQuery's wave — `motion`, `masked` and the three arrays mean what they
// mean there — for the max_hits frontmost hits of every ray.  isects[i * max_hits + j] holds ray i's hits in ascending (t, prim_id)
// order, then miss records {0, 0, ray.max_t, 0xFFFFFFFF}: every record is written.  counts_out (optional) receives the hits held.
template <typename T = float>
struct MultiHitBatchQuery {
  MultiHitBatchQuery()
      : rays(NULL), num_rays(0), times(NULL), ray_masks(NULL), skip_prim_ids(NULL), motion(false), masked(false), isects(NULL), max_hits(0),
        counts_out(NULL) {}
  const Ray<T> *rays;
  size_t num_rays;
  const T *times;
  const unsigned int *ray_masks;
  const unsigned int *skip_prim_ids;
  bool motion, masked;
  BVHTraceOptions options;
  TriangleIntersection<T> *isects;
  unsigned int max_hits;
  unsigned int *counts_out;
};

// Robust slab test (Ize 2013), t_max terms widened by MaxMult
// (ref nanort.h:2278-2370).
namespace detail {
template <typename T>
struct MaxMult;
template <>
struct MaxMult<float> {
  static float value() { return 1.00000024f; }
};
template <>
struct MaxMult<double> {
  static double value() { return 1.0000000000000004; }
};
}  // namespace detail

template <typename T>
inline bool IntersectRayAABB(T *tminOut, T *tmaxOut, T min_t, T max_t, const T bmin[3], const T bmax[3], real3<T> ray_org,
                             real3<T> ray_inv_dir, int ray_dir_sign[3]) {
  T lo = min_t, hi = max_t;
  const T widen = detail::MaxMult<T>::value();
  for (int k = 0; k < 3; k++) {
    const T near_plane = ray_dir_sign[k] ? bmax[k] : bmin[k];
    const T far_plane = ray_dir_sign[k] ? bmin[k] : bmax[k];
    const T t_near = (near_plane - ray_org[k]) * ray_inv_dir[k];
    const T t_far = (far_plane - ray_org[k]) * ray_inv_dir[k] * widen;
    lo = safemax(t_near, lo);
    hi = safemin(t_far, hi);
  }
  if (lo <= hi) {
    *tminOut = lo;
    *tmaxOut = hi;
    return true;
  }
  return false;
}

// ---------------------------------------------------------------------------
// Built-in sphere ("particle") primitive.  Not in the reference header: the reference ships it as user code in
// examples/particle_primitive/main.cc (SpherePred :82-108, SphereGeometry :113-147, SphereIntersection :149-159,
// SphereIntersector :161-291).  Same concepts, same arithmetic, same names — an application drops its local
// copies and uses these; with NANORT_USE_HIP_BACKEND, Build() over (SphereGeometry, SpherePred) and
// TraverseBatch() with SphereIntersection run on the GPU (nrtSetSpheres_f32).  fp32, like the example.
// ---------------------------------------------------------------------------
class SpherePred {
 public:
  explicit SpherePred(const float *centers) : axis_(0), pos_(0.0f), centers_(centers) {}
  void Set(int axis, float pos) const {
    axis_ = axis;
    pos_ = pos;
  }
  bool operator()(unsigned int i) const { return centers_[3 * i + axis_] < pos_; }

 private:
  mutable int axis_;
  mutable float pos_;
  const float *centers_;
};

class SphereGeometry {
 public:
  SphereGeometry(const float *centers, const float *radii) : centers_(centers), radii_(radii) {}
  void BoundingBox(real3<float> *bmin, real3<float> *bmax, unsigned int i) const {
    for (int k = 0; k < 3; k++) {
      (*bmin)[k] = centers_[3 * i + k] - radii_[i];
      (*bmax)[k] = centers_[3 * i + k] + radii_[i];
    }
  }
  void BoundingBoxAndCenter(real3<float> *bmin, real3<float> *bmax, real3<float> *center, unsigned int i) const {
    BoundingBox(bmin, bmax, i);
    for (int k = 0; k < 3; k++) (*center)[k] = centers_[3 * i + k];
  }
  const float *GetCenters() const { return centers_; }
  const float *GetRadii() const { return radii_; }

 private:
  const float *centers_;
  const float *radii_;
};

class SphereIntersection {
 public:
  SphereIntersection() : u(0.0f), v(0.0f), t(std::numeric_limits<float>::max()), prim_id(static_cast<unsigned int>(-1)) {}
  float u, v;  // spherical coordinates of the hit normal, both in [0, 1]
  float t;
  unsigned int prim_id;
};

template <class H = SphereIntersection>
class SphereIntersector {
 public:
  SphereIntersector(const float *centers, const float *radii) : centers_(centers), radii_(radii), t_(0.0f), prim_id_(0) {}

  // Nearest root of |org + t dir - c|^2 = r^2 that lies in front of the origin, accepted iff <= *t_inout.
  bool Intersect(float *t_inout, unsigned int i) const {
    if (i < opts_.prim_ids_range[0] || i >= opts_.prim_ids_range[1]) return false;
    const real3<float> oc = org_ - real3<float>(&centers_[3 * i]);
    const float a = vdot(dir_, dir_);
    const float b = 2.0f * vdot(dir_, oc);
    const float c = vdot(oc, oc) - radii_[i] * radii_[i];
    const float disc = b * b - 4.0f * a * c;
    if (disc < 0.0f) return false;
    float t0, t1;
    if (std::fabs(disc) < std::numeric_limits<float>::epsilon()) {
      t0 = t1 = -0.5f * (b / a);
    } else {
      const float root = std::sqrt(disc);
      const float q = (b < 0) ? (-b - root) / 2.0f : (-b + root) / 2.0f;
      t0 = q / a;
      t1 = c / q;
    }
    if (t0 > t1) std::swap(t0, t1);
    if (t1 < 0) return false;
    const float t = (t0 < 0) ? t1 : t0;
    if (t > *t_inout) return false;
    *t_inout = t;
    return true;
  }
  float GetT() const { return t_; }
  void Update(float t, unsigned int i) const {
    t_ = t;
    prim_id_ = i;
  }
  void PrepareTraversal(const Ray<float> &ray, const BVHTraceOptions &options) const {
    org_ = real3<float>(ray.org);
    dir_ = real3<float>(ray.dir);
    opts_ = options;
  }
  void PostTraversal(const Ray<float> &, bool hit, H *isect) const {
    if (!hit) return;
    const real3<float> n = vnormalize((org_ + t_ * dir_) - real3<float>(&centers_[3 * prim_id_]));
    const double pi = 3.14159265358979323846;
    isect->t = t_;
    isect->prim_id = prim_id_;
    isect->u = float(std::atan2(double(n[0]), double(n[2])) + pi) * 0.5f * float(1.0 / pi);
    isect->v = float(std::acos(double(n[1])) / pi);
  }

 private:
  const float *centers_;
  const float *radii_;
  mutable real3<float> org_, dir_;
  mutable BVHTraceOptions opts_;
  mutable float t_;
  mutable unsigned int prim_id_;
};

// ---------------------------------------------------------------------------
// Built-in cylinder primitive: the reference's second custom-primitive example, examples/cylinder_primitive/main.cc
// (solve2e :61-90, CylinderPred :94-120, CylinderGeometry :124-210, CylinderIntersection :213-224,
// CylinderIntersector :226-424) — same concepts, same arithmetic.  Two end points and two radii per cylinder (the
// intersector uses the larger radius for the whole cylinder).  With NANORT_USE_HIP_BACKEND, Build() over
// (CylinderGeometry, CylinderPred) and TraverseBatch() with CylinderIntersection run on the GPU.
// One difference: PostTraversal also stores isect->t (the example leaves it untouched).
// ---------------------------------------------------------------------------
class CylinderPred {
 public:
  explicit CylinderPred(const float *endpoints) : axis_(0), pos_(0.0f), endpoints_(endpoints) {}
  void Set(int axis, float pos) const {
    axis_ = axis;
    pos_ = pos;
  }
  bool operator()(unsigned int i) const { return (endpoints_[6 * i + axis_] + endpoints_[6 * i + 3 + axis_]) / 2.0f < pos_; }

 private:
  mutable int axis_;
  mutable float pos_;
  const float *endpoints_;
};

class CylinderGeometry {
 public:
  CylinderGeometry(const float *endpoints, const float *radii) : endpoints_(endpoints), radii_(radii) {}
  void BoundingBox(real3<float> *bmin, real3<float> *bmax, unsigned int i) const {
    for (int k = 0; k < 3; k++) {
      const float a = endpoints_[6 * i + k], b = endpoints_[6 * i + 3 + k];
      (*bmin)[k] = std::min(b - radii_[2 * i + 1], a - radii_[2 * i]);
      (*bmax)[k] = std::max(b + radii_[2 * i + 1], a + radii_[2 * i]);
    }
  }
  void BoundingBoxAndCenter(real3<float> *bmin, real3<float> *bmax, real3<float> *center, unsigned int i) const {
    BoundingBox(bmin, bmax, i);
    for (int k = 0; k < 3; k++) (*center)[k] = (endpoints_[6 * i + k] + endpoints_[6 * i + 3 + k]) / 2.0f;
  }
  const float *GetEndpoints() const { return endpoints_; }
  const float *GetRadii() const { return radii_; }

 private:
  const float *endpoints_;
  const float *radii_;
};

class CylinderIntersection {
 public:
  CylinderIntersection() : u(0.0f), v(0.0f), normal(0.0f), t(std::numeric_limits<float>::max()), prim_id(static_cast<unsigned int>(-1)) {}
  float u;  // distance from the axis on a cap hit, 0 on the side
  float v;  // 0 / 1 on the first / second cap, the axis parameter in [0, 1] on the side
  real3<float> normal;
  float t;
  unsigned int prim_id;
};

template <class H = CylinderIntersection>
class CylinderIntersector {
 public:
  CylinderIntersector(const float *endpoints, const float *radii, bool test_cap = true)
      : endpoints_(endpoints), radii_(radii), test_cap_(test_cap), t_(0.0f), prim_id_(0), hit_cap_(false), u_param_(0.0f), v_param_(0.0f) {}

  bool Intersect(float *t_inout, unsigned int i) const {
    if (i < opts_.prim_ids_range[0] || i >= opts_.prim_ids_range[1]) return false;
    const float eps = 1.0e-6f;
    const real3<float> p0(&endpoints_[6 * i]), p1(&endpoints_[6 * i + 3]);
    const float tmax = *t_inout;
    const float rr = std::max<float>(radii_[2 * i], radii_[2 * i + 1]);
    const real3<float> d = p1 - p0, m = org_ - p0;
    const float md = vdot(m, d), nd = vdot(dir_, d), dd = vdot(d, d);
    bool hit_cap = false;
    float cap_t = std::numeric_limits<float>::max();
    if (test_cap_) {  // the two end planes first
      const real3<float> n0 = vnormalize(p0 - p1), n1 = vneg(n0), rd = vnormalize(dir_);
      if (std::fabs(vdot(dir_, n0)) > eps) {
        const float d0 = -vdot(p0, n0), d1 = -vdot(p1, n1);
        const float t0 = -(vdot(org_, n0) + d0) / vdot(rd, n0);
        const float t1 = -(vdot(org_, n1) + d1) / vdot(rd, n1);
        const real3<float> q0 = org_ + t0 * rd, q1 = org_ + t1 * rd;
        const float r0sq = vdot(q0 - p0, q0 - p0), r1sq = vdot(q1 - p1, q1 - p1);
        if (t0 > 0.0 && t0 < tmax && (r0sq < rr * rr)) {
          hit_cap_ = hit_cap = true;
          cap_t = t0;
          *t_inout = cap_t;
          u_param_ = std::sqrt(r0sq);
          v_param_ = 0;
        }
        if (t1 > 0.0 && t1 < tmax && t1 < cap_t && (r1sq < rr * rr)) {
          hit_cap_ = hit_cap = true;
          cap_t = t1;
          *t_inout = cap_t;
          u_param_ = std::sqrt(r1sq);
          v_param_ = 1.0;
        }
      }
    }
    if (md <= 0.0 && nd <= 0.0) return hit_cap;  // origin behind the first cap, pointing away
    if (md >= dd && nd >= 0.0) return hit_cap;   // origin beyond the second cap, pointing away
    const float nn = vdot(dir_, dir_), mn = vdot(m, dir_);
    const float A = dd * nn - nd * nd;
    const float k = vdot(m, m) - rr * rr;
    const float C = dd * k - md * md;
    const float B = dd * mn - nd * md;
    float root = 0.0f;
    if (SmallerRoot(&root, A, B, C)) {
      const float t = root;
      if (0 <= t && t <= tmax && t <= cap_t) {
        float s = md + t * nd;
        s /= dd;
        if (0 <= s && s <= 1) {
          hit_cap_ = false;
          *t_inout = t;
          u_param_ = 0;
          v_param_ = s;
          return true;
        }
      }
    }
    return hit_cap;
  }
  float GetT() const { return t_; }
  void Update(float t, unsigned int i) const {
    t_ = t;
    prim_id_ = i;
  }
  void PrepareTraversal(const Ray<float> &ray, const BVHTraceOptions &options) const {
    org_ = real3<float>(ray.org);
    dir_ = real3<float>(ray.dir);
    opts_ = options;
  }
  void PostTraversal(const Ray<float> &, bool hit, H *isect) const {
    if (!hit) return;
    const real3<float> p0(&endpoints_[6 * prim_id_]), p1(&endpoints_[6 * prim_id_ + 3]);
    const real3<float> axis_point = p0 + real3<float>(v_param_, v_param_, v_param_) * (p1 - p0);
    const real3<float> position = org_ + t_ * dir_;
    real3<float> n;
    if (hit_cap_) {
      const real3<float> mid = 0.5f * (p1 - p0) + p0;
      n = vnormalize(p1 - p0);
      if (!(vdot(position - mid, n) > 0.0)) n = vneg(n);
    } else {
      n = vnormalize(position - axis_point);
    }
    isect->u = u_param_;
    isect->v = v_param_;
    isect->normal = n;
    isect->t = t_;
    isect->prim_id = prim_id_;
  }

 private:
  // The smaller root of A x^2 + 2 B x + C = 0 in the example's formulation (its solve2e); false when there is none.
  static bool SmallerRoot(float *root, float A, float B, float C) {
    if (std::fabs(A) <= 1.0e-6f) {
      *root = -C / B;
      return true;
    }
    const float D = B * B - A * C;
    if (D < 0) return false;
    if (D == 0) {
      *root = -B / A;
      return true;
    }
    float x1 = (std::fabs(B) + std::sqrt(D)) / A;
    if (B >= 0.0) x1 = -x1;
    const float x2 = C / (A * x1);
    *root = (x1 > x2) ? x2 : x1;
    return true;
  }

  const float *endpoints_;
  const float *radii_;
  const bool test_cap_;
  mutable real3<float> org_, dir_;
  mutable BVHTraceOptions opts_;
  mutable float t_;
  mutable unsigned int prim_id_;
  mutable bool hit_cap_;
  mutable float u_param_, v_param_;

 public:
  bool TestsCaps() const { return test_cap_; }
};

// ---------------------------------------------------------------------------
// Built-in curve primitive: hair and fur as cubic Bezier curves, the reference's third custom-primitive example,
// examples/curves_primitive/main.cc (GetZAlign :382-417, Xform :419-430, EvaluateBezier :432-454, EvaluateBezierTangent
// :456-462, CurvePred :481-509, CurveGeometry :513-604, CurveIntersection :606-619, CurveIntersector :621-840) — same concepts,
// same arithmetic.  Named BezierCurve* so that a program which still carries the example's own Curve* classes compiles
// against this header unchanged.  Four control points (12 floats) and four radii per curve; the intersector walks the curve
// as `num_subdivisions` line segments in a frame whose z axis is the ray and reads the first and the last radius.  With
// NANORT_USE_HIP_BACKEND, Build() over (BezierCurveGeometry, BezierCurvePred) and TraverseBatch() with
// BezierCurveIntersection run on the GPU (nrtSetCurves_f32).  fp32, like the example.
// ---------------------------------------------------------------------------
class BezierCurvePred {
 public:
  explicit BezierCurvePred(const float *control_points) : axis_(0), pos_(0.0f), cps_(control_points) {}
  void Set(int axis, float pos) const {
    axis_ = axis;
    pos_ = pos;
  }
  bool operator()(unsigned int i) const {
    const float *p = cps_ + 12 * static_cast<size_t>(i) + axis_;
    return (p[0] + p[3] + p[6] + p[9]) / 4.0f < pos_;
  }

 private:
  mutable int axis_;
  mutable float pos_;
  const float *cps_;
};

class BezierCurveGeometry {
 public:
  BezierCurveGeometry(const float *control_points, const float *radii) : cps_(control_points), radii_(radii) {}
  // (a Bezier curve lies inside the hull of its control points: the box of the four points, each grown by its radius)
  void BoundingBox(real3<float> *bmin, real3<float> *bmax, unsigned int i) const {
    const float *p = cps_ + 12 * static_cast<size_t>(i), *r = radii_ + 4 * static_cast<size_t>(i);
    for (int k = 0; k < 3; k++) {
      (*bmin)[k] = p[k] - r[0];
      (*bmax)[k] = p[k] + r[0];
      for (int j = 1; j < 4; j++) {
        (*bmin)[k] = std::min(p[3 * j + k] - r[j], (*bmin)[k]);
        (*bmax)[k] = std::max(p[3 * j + k] + r[j], (*bmax)[k]);
      }
    }
  }
  void BoundingBoxAndCenter(real3<float> *bmin, real3<float> *bmax, real3<float> *center, unsigned int i) const {
    BoundingBox(bmin, bmax, i);
    const float *p = cps_ + 12 * static_cast<size_t>(i);
    for (int k = 0; k < 3; k++) (*center)[k] = (p[k] + p[3 + k] + p[6 + k] + p[9 + k]) / 4.0f;
  }
  const float *GetControlPoints() const { return cps_; }
  const float *GetRadii() const { return radii_; }

 private:
  const float *cps_;
  const float *radii_;
};

class BezierCurveIntersection {
 public:
  BezierCurveIntersection() : t(std::numeric_limits<float>::max()), prim_id(static_cast<unsigned int>(-1)), u(0.0f), v(0.0f), tangent(0.0f), normal(0.0f) {}
  float t;
  unsigned int prim_id;
  float u;                // curve parameter of the hit, over the whole curve
  float v;                // distance of the ray from the curve's axis there
  real3<float> tangent;   // curve direction
  real3<float> normal;    // perpendicular to the curve, in the plane of the ray and the tangent
};

template <class H = BezierCurveIntersection>
class BezierCurveIntersector {
 public:
  BezierCurveIntersector(const float *control_points, const float *radii, int num_subdivisions = 4)
      : cps_(control_points), radii_(radii), num_subdivisions_(num_subdivisions), t_(0.0f), u_(0.0f), v_(0.0f), prim_id_(0), u_param_(0.0f),
        v_param_(0.0f) {}

  bool Intersect(float *t_inout, unsigned int i) const {
    if (i < opts_.prim_ids_range[0] || i >= opts_.prim_ids_range[1]) return false;
    float m[3][3], tr[3];
    ZAlign(m, tr);
    const float *p = cps_ + 12 * static_cast<size_t>(i);
    const float r0 = radii_[4 * static_cast<size_t>(i)], r3 = radii_[4 * static_cast<size_t>(i) + 3];
    float c[4][3];
    float t_z = 0.0f;
    for (int j = 0; j < 4; j++) {
      for (int k = 0; k < 3; k++) c[j][k] = p[3 * j] * m[0][k] + p[3 * j + 1] * m[1][k] + p[3 * j + 2] * m[2][k] + tr[k];
      if (t_z < c[j][2]) t_z = c[j][2];
    }
    const float uw = std::max(r0, r3) / 2.0f;
    if (t_z < 4.0f * uw) return false;
    bool has_hit = false;
    const int n = num_subdivisions_;
    const float inv_n = 1.0f / static_cast<float>(n);
    const float w0 = 0.5f * r0, w1 = 0.5f * r3;
    for (int s = 0; s < n; s++) {
      float p0[3], p1[3];
      Bezier(c, s / static_cast<float>(n), p0);
      Bezier(c, (s + 1) / static_cast<float>(n), p1);
      const float ax = 0.0f - p0[0], ay = 0.0f - p0[1];  // the origin, projected onto the segment in the frame's xy plane
      const float bx = p1[0] - p0[0], by = p1[1] - p0[1], bz = p1[2] - p0[2], bw = w1 - w0;
      const float d0 = (ax * bx) + (ay * by), d1 = (bx * bx) + (by * by);
      float u = d0 / d1;
      u = std::max(0.0f, std::min(1.0f, u));  // (a NaN u, from a zero-length segment, becomes 1)
      const float px = p0[0] + (u * bx), py = p0[1] + (u * by), t = p0[2] + (u * bz), r = w0 + (u * bw);
      const float r2 = r * r, d2 = (px * px) + (py * py);
      if ((d2 <= r2) && (t < (*t_inout))) {
        u_param_ = (u + static_cast<float>(s)) * inv_n;
        v_param_ = std::sqrt(d2);
        (*t_inout) = t;
        has_hit = true;
      }
    }
    return has_hit;
  }
  float GetT() const { return t_; }
  void Update(float t, unsigned int i) const {
    t_ = t;
    prim_id_ = i;
    u_ = u_param_;
    v_ = v_param_;
  }
  void PrepareTraversal(const Ray<float> &ray, const BVHTraceOptions &options) const {
    org_ = real3<float>(ray.org);
    dir_ = real3<float>(ray.dir);
    opts_ = options;
  }
  void PostTraversal(const Ray<float> &, bool hit, H *isect) const {
    if (!hit || !isect) return;
    const float *p = cps_ + 12 * static_cast<size_t>(prim_id_);
    const real3<float> v0(p), v1(p + 3), v2(p + 6), v3(p + 9);
    const real3<float> C1 = v3 - (3.0f * v2) + (3.0f * v1) - v0;
    const real3<float> C2 = (3.0f * v2) - (6.0f * v1) + (3.0f * v0);
    const real3<float> C3 = (3.0f * v1) - (3.0f * v0);
    isect->tangent = vnormalize((3.0f * C1 * u_ * u_) + (2.0f * C2 * u_) + C3);
    isect->normal = vnormalize(vcross(vcross(dir_, isect->tangent), isect->tangent));
    isect->t = t_;
    isect->u = u_;
    isect->v = v_;
    isect->prim_id = prim_id_;
  }
  int NumSubdivisions() const { return num_subdivisions_; }

 private:
  // The rotation that puts the ray's direction on the z axis, and the translation that puts its origin at 0.
  void ZAlign(float m[3][3], float tr[3]) const {
    const float lx = dir_[0], ly = dir_[1], lz = dir_[2];
    const float dxz = std::sqrt(lx * lx + lz * lz);
    if (dxz > 0) {
      const float lxdxz = lx / dxz, lydxz = ly / dxz, lzdxz = lz / dxz;
      m[0][0] = lzdxz;
      m[0][1] = -lxdxz * ly;
      m[0][2] = lx;
      m[1][0] = 0;
      m[1][1] = dxz;
      m[1][2] = ly;
      m[2][0] = -lxdxz;
      m[2][1] = -lydxz * lz;
      m[2][2] = lz;
    } else {
      m[0][0] = 1;
      m[0][1] = 0;
      m[0][2] = 0;
      m[1][0] = 0;
      m[1][1] = 0;
      m[1][2] = (ly > 0) ? -1.0f : 1.0f;
      m[2][0] = 0;
      m[2][1] = (ly > 0) ? 1.0f : -1.0f;
      m[2][2] = 0;
    }
    for (int k = 0; k < 3; k++) tr[k] = -(org_[0] * m[0][k] + org_[1] * m[1][k] + org_[2] * m[2][k]);
  }
  static void Bezier(const float c[4][3], float t, float out[3]) {  // de Casteljau
    const float u = 1 - t;
    for (int k = 0; k < 3; k++) {
      const float a0 = c[0][k] * u + c[1][k] * t, a1 = c[1][k] * u + c[2][k] * t, a2 = c[2][k] * u + c[3][k] * t;
      const float b0 = a0 * u + a1 * t, b1 = a1 * u + a2 * t;
      out[k] = b0 * u + b1 * t;
    }
  }

  const float *cps_;
  const float *radii_;
  const int num_subdivisions_;
  mutable real3<float> org_, dir_;
  mutable BVHTraceOptions opts_;
  mutable float t_, u_, v_;
  mutable unsigned int prim_id_;
  mutable float u_param_, v_param_;
};

// ---------------------------------------------------------------------------
// BVHAccel
// ---------------------------------------------------------------------------
namespace detail {
template <class A, class B>
struct same_type {
  static const bool value = false;
};
template <class A>
struct same_type<A, A> {
  static const bool value = true;
};
struct generic_tag {};
struct triangle_tag {};
struct sphere_tag {};
struct cylinder_tag {};
struct curve_tag {};
struct motion_triangle_tag {};
template <typename T, class Prim, class Pred>
struct build_tag {
#ifdef NANORT_USE_HIP_BACKEND
  typedef typename std::conditional<
      same_type<Prim, TriangleMesh<T> >::value && same_type<Pred, TriangleSAHPred<T> >::value, triangle_tag,
      typename std::conditional<
          same_type<Prim, MotionTriangleMesh<T> >::value && same_type<Pred, MotionTriangleSAHPred<T> >::value, motion_triangle_tag,
      typename std::conditional<
          same_type<T, float>::value && same_type<Prim, SphereGeometry>::value && same_type<Pred, SpherePred>::value, sphere_tag,
          typename std::conditional<
              same_type<T, float>::value && same_type<Prim, CylinderGeometry>::value && same_type<Pred, CylinderPred>::value, cylinder_tag,
              typename std::conditional<same_type<T, float>::value && same_type<Prim, BezierCurveGeometry>::value && same_type<Pred, BezierCurvePred>::value,
                                        curve_tag, generic_tag>::type>::type>::type>::type>::type type;
#else
  typedef generic_tag type;
#endif
};

#ifdef NANORT_USE_HIP_BACKEND
// float/double -> the matching C-ABI entry points (include/nanort_hip.h): ONE list, a line per entry point, instantiated for
// {float, f32} and {double, f64}.  (constexpr pointers: a call through one is a direct call, and none needs a definition.)
template <typename T>
struct HipApi;
#define NANORT_HIP_ENTRY(name, entry, S) static constexpr decltype(&entry##_##S) name = &entry##_##S;
#define NANORT_HIP_API(T, S)                                                      \
  template <>                                                                     \
  struct HipApi<T> {                                                              \
    typedef nrt_ray_##S RayPod;                                                   \
    typedef nrt_node_##S NodePod;                                                 \
    typedef nrt_hit_##S HitPod;                                                   \
    typedef nrt_build_options_##S BuildPod;                                       \
    NANORT_HIP_ENTRY(SetMesh, nrtSetMesh, S)                                      \
    NANORT_HIP_ENTRY(Build, nrtBuild, S)                                          \
    NANORT_HIP_ENTRY(GetTree, nrtGetTree, S)                                      \
    NANORT_HIP_ENTRY(TreeBounds, nrtGetTreeBounds, S)                             \
    NANORT_HIP_ENTRY(SetTree, nrtSetTree, S)                                      \
    NANORT_HIP_ENTRY(Refit, nrtRefit, S)                                          \
    NANORT_HIP_ENTRY(Traverse, nrtTraverseBatch, S)                               \
    NANORT_HIP_ENTRY(TraverseDevice, nrtTraverseBatchDevice, S)                   \
    NANORT_HIP_ENTRY(TraverseBatches, nrtTraverseBatchesDevice, S)                \
    NANORT_HIP_ENTRY(TraverseBatchesHost, nrtTraverseBatches, S)                  \
    NANORT_HIP_ENTRY(TraverseMulti, nrtTraverseBatchMulti, S)                     \
    NANORT_HIP_ENTRY(Occluded, nrtOccludedBatch, S)                               \
    NANORT_HIP_ENTRY(OccludedDevice, nrtOccludedBatchDevice, S)                   \
    /* per-ray skip ids: the calls above with one skip id per ray */              \
    NANORT_HIP_ENTRY(TraverseSkip, nrtTraverseBatchSkip, S)                       \
    NANORT_HIP_ENTRY(TraverseSkipDevice, nrtTraverseBatchSkipDevice, S)           \
    NANORT_HIP_ENTRY(OccludedSkip, nrtOccludedBatchSkip, S)                       \
    NANORT_HIP_ENTRY(OccludedSkipDevice, nrtOccludedBatchSkipDevice, S)           \
    NANORT_HIP_ENTRY(TraverseBatchesSkip, nrtTraverseBatchesSkipDevice, S)        \
    NANORT_HIP_ENTRY(TraverseBatchesSkipHost, nrtTraverseBatchesSkip, S)          \
    NANORT_HIP_ENTRY(MultiHit, nrtMultiHitTraverseBatch, S)                       \
    NANORT_HIP_ENTRY(MultiHitDevice, nrtMultiHitTraverseBatchDevice, S)           \
    /* motion blur: the second vertex keyframe, the queries with a time per ray */ \
    NANORT_HIP_ENTRY(SetMeshMotion, nrtSetMeshMotion, S)                          \
    NANORT_HIP_ENTRY(TraverseMotion, nrtTraverseBatchMotion, S)                   \
    NANORT_HIP_ENTRY(OccludedMotion, nrtOccludedBatchMotion, S)                   \
    /* visibility masks: the queries with one word per ray (the setter, nrtSetPrimMasks, has no precision) */ \
    NANORT_HIP_ENTRY(TraverseMasked, nrtTraverseBatchMasked, S)                   \
    NANORT_HIP_ENTRY(OccludedMasked, nrtOccludedBatchMasked, S)                   \
    /* skip ids, words and times on the same ray: one descriptor */              \
    typedef nrt_ray_query_##S QueryPod;                                           \
    NANORT_HIP_ENTRY(Query, nrtQueryBatch, S)                                     \
    NANORT_HIP_ENTRY(QueryDevice, nrtQueryBatchDevice, S)                         \
    /* ... and the multi-hit query with the same three: its own descriptor */     \
    typedef nrt_multihit_query_##S MultiHitQueryPod;                              \
    NANORT_HIP_ENTRY(MultiHitQuery, nrtMultiHitQueryBatch, S)                     \
    NANORT_HIP_ENTRY(MultiHitQueryDevice, nrtMultiHitQueryBatchDevice, S)         \
    /* closest-point queries */                                                   \
    typedef nrt_point_##S PointPod;                                               \
    typedef nrt_closest_##S ClosestPod;                                           \
    NANORT_HIP_ENTRY(ClosestPoint, nrtClosestPointBatch, S)                       \
    /* signed distance queries */                                                 \
    typedef nrt_signed_##S SignedPod;                                             \
    NANORT_HIP_ENTRY(SignedDistance, nrtSignedDistanceBatch, S)                   \
    /* nearest-faces queries */                                                   \
    NANORT_HIP_ENTRY(NearestFaces, nrtNearestFacesBatch, S)                       \
  };
NANORT_HIP_API(float, f32)
NANORT_HIP_API(double, f64)
#undef NANORT_HIP_API
#undef NANORT_HIP_ENTRY
struct CtxDeleter {
  void operator()(nrt_ctx *c) const { nrtDestroy(c); }
};
// serialises the on-demand read-back of GPU-built trees (BVHAccel::EnsureHostTree); one per process is plenty
inline std::mutex &HostTreeMutex() {
  static std::mutex m;
  return m;
}
#endif
}  // namespace detail

// The angle-weighted pseudonormals of a triangle mesh, built on the host by the rule of nanort_sdf.h (BuildFeatureNormals): what
// BVHAccel::SignedDistance() signs with.  face_normals: [num_faces][4][3] — the unit normal, then the edge normals of ab, ac, bc;
// vertex_normals: [num_vertices][3], num_vertices the largest vertex index + 1.  Vertices are identified by index, not position.
// (The GPU derives its own from the device-resident mesh: nrtGetFeatureNormals; face and edge normals are the same bytes, vertex
// normals differ by the device's atan2.)
template <typename T = float>
class FeatureNormals {
 public:
  FeatureNormals() : num_faces(0), num_vertices(0) {}
  FeatureNormals(const TriangleMesh<T> &mesh, size_t num_faces_) { Build(mesh, num_faces_); }
  void Build(const TriangleMesh<T> &mesh, size_t num_faces_) {
    num_faces = num_faces_;
    num_vertices = 0;
    for (size_t i = 0; i < 3 * num_faces; i++) num_vertices = std::max(num_vertices, static_cast<size_t>(mesh.faces_[i]) + 1);
    std::vector<T> tight(3 * num_vertices);
    for (size_t v = 0; v < num_vertices; v++) {
      const T *src = get_vertex_addr<T>(mesh.vertices_, v, mesh.vertex_stride_bytes_);
      tight[3 * v + 0] = src[0], tight[3 * v + 1] = src[1], tight[3 * v + 2] = src[2];
    }
    face_normals.assign(12 * num_faces, static_cast<T>(0.0));
    vertex_normals.assign(3 * num_vertices, static_cast<T>(0.0));
    nanort_sdf::BuildFeatureNormals<T>(tight.empty() ? NULL : &tight[0], mesh.faces_, num_faces, num_vertices,
                                       face_normals.empty() ? NULL : &face_normals[0], vertex_normals.empty() ? NULL : &vertex_normals[0]);
  }
  // The normal of `feature` (0..6) of face `prim`.
  const T *Of(const TriangleMesh<T> &mesh, unsigned int prim, unsigned int feature) const {
    if (feature < nanort_sdf::kFeatureVertexA) return &face_normals[12 * static_cast<size_t>(prim) + 3 * feature];
    return &vertex_normals[3 * static_cast<size_t>(mesh.faces_[3 * static_cast<size_t>(prim) + (feature - nanort_sdf::kFeatureVertexA)])];
  }
  std::vector<T> face_normals, vertex_normals;
  size_t num_faces, num_vertices;
};

template <typename T>
class BVHAccel {
 public:
  BVHAccel() : pad0_(0) { (void)pad0_; }
  ~BVHAccel() {}
#ifdef NANORT_USE_HIP_BACKEND
  // A GPU Build() leaves the tree on the device: nodes_ / indices_ are fetched by the first host access (GetNodes(),
  // GetIndices(), Traverse(), MultiHitTraverse(), ListNodeIntersections(), Dump(), Debug(), copying).  A copy takes the host
  // arrays with it (copying materialises them first) and shares the device contexts (shared_ptr) until either side changes
  // what a context holds: Build(), the upload of a Load()ed tree and the cylinder cap re-send first move the object that
  // makes the change to contexts of its own (copy-on-write: the primitive arrays Build() was given are sent again, so they
  // must outlive the accel, as the reference's Traverse() already requires).  Neither side ever traces the other's tree.
  // A move transfers the contexts, a pending read-back and the staging buffers as they are (no read-back); the source is
  // left empty (IsValid() false), ready to be rebuilt or destroyed.  What the device holds travels as two records (DeviceState,
  // DeviceGeometry below): the copy copies them, the move takes them and leaves default-constructed ones in the source.
  BVHAccel(const BVHAccel &o) : pad0_(0) { CopyFrom(o); }
  BVHAccel &operator=(const BVHAccel &o) {
    if (this != &o) CopyFrom(o);
    return *this;
  }
  BVHAccel(BVHAccel &&o) noexcept : pad0_(0) { MoveFrom(&o); }  // (noexcept: std::vector moves rather than copies)
  BVHAccel &operator=(BVHAccel &&o) noexcept {
    if (this != &o) MoveFrom(&o);
    return *this;
  }
#endif

  // Build a BVH over `num_primitives` primitives (ref nanort.h:716-718).
  // Returns false iff num_primitives == 0.
  template <class Prim, class Pred>
  bool Build(const unsigned int num_primitives, const Prim &p, const Pred &pred, const BVHBuildOptions<T> &options = BVHBuildOptions<T>()) {
    return BuildImpl(num_primitives, p, pred, options, typename detail::build_tag<T, Prim, Pred>::type());
  }

  BVHBuildStatistics GetStatistics() const { return stats_; }

  // Refit: the tree's boxes recomputed bottom-up for primitives that moved, its topology and index array kept (no rebuild).
  // Each reachable leaf's box becomes the union of its primitives' BoundingBox(&bmin, &bmax, prim_index), each reachable
  // branch's the union of its two children's (an empty leaf: {+max, -max}); records the walk from the root never reaches keep
  // theirs.  A refit tree may trace slower than a fresh Build() over the same primitives: rebuild when they moved far.
  // Returns false (nothing changed) when there is no tree or the tree is malformed (a child or leaf slot out of range, a
  // record reached twice).
  template <class Prim>
  bool Refit(const Prim &p) {
#ifdef NANORT_USE_HIP_BACKEND
    if (dev_.ctx && !dev_.tree_stale) {  // (the GPU holds this tree: refit it there — Refit(TriangleMesh) — or rebuild)
      backend_error_ = "Refit: this tree was built on the GPU over built-in primitives; refit a triangle mesh with Refit(TriangleMesh)";
      return false;
    }
#endif
    return RefitHost(p);
  }
#ifdef NANORT_USE_HIP_BACKEND
  // The GPU refit (nrtRefit, include/nanort_hip.h) of every context this object holds, the NANORT_HIP_DEVICES replicas
  // included, from the mesh's vertices and stride; its faces must equal the built ones.  An object that shares its contexts
  // with a copy first moves to contexts of its own (copy-on-write: the copy keeps its tree and positions) and keeps the new
  // vertex array, as Build() does: it must outlive the accel.  The host copy of the tree is read back on the next host access.
  bool Refit(const TriangleMesh<T> &mesh) {
    if (!dev_.ctx) return RefitHost(mesh);  // (a tree built on the host or Load()ed before any GPU Build())
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (geom_.kind >= 1 && geom_.kind <= 3) return NoGpuRefit(geom_.kind);
    if (geom_.kind != 0) {
      backend_error_ = "Refit: no triangle tree (Build() with TriangleMesh/TriangleSAHPred first)";
      return false;
    }
    if (geom_.vertices1) {  // (the library refuses too: nrtRefit on a context that holds a motion keyframe)
      backend_error_ = "Refit: this accel was built over a MotionTriangleMesh: its boxes hold both keyframes (Build() again)";
      return false;
    }
    if (mesh.GetFaces() != geom_.faces &&
        (!mesh.GetFaces() || !geom_.faces || std::memcmp(mesh.GetFaces(), geom_.faces, 3 * sizeof(unsigned int) * geom_.count) != 0)) {
      backend_error_ = "Refit: the mesh's faces differ from the ones the tree was built over";
      return false;
    }
    if (!RefitContexts(0, [&](nrt_ctx *c) { return Api::Refit(c, mesh.GetVertices(), mesh.GetVertexStrideBytes()); })) return false;
    geom_.vertices = mesh.GetVertices();  // (a later detach sends these)
    geom_.stride = mesh.GetVertexStrideBytes();
    return RefitDone();
  }
  bool Refit(const SphereGeometry &) { return NoGpuRefit(1); }
  bool Refit(const CylinderGeometry &) { return NoGpuRefit(2); }
  bool Refit(const BezierCurveGeometry &) { return NoGpuRefit(3); }
  // The GPU refit of a sphere or curve accel (nrtRefitPrims, include/nanort_hip.h) from the geometry's arrays, as Refit(TriangleMesh)
  // for a mesh: every context this object holds, after a copy-on-write detach when they are shared with copies; the new arrays
  // are kept as Build() keeps its own (they must outlive the accel).  The geometry carries no count: `num_primitives`, when
  // given, must be the count of the Build().  False with a reason (LastBackendError()) when the object holds another kind or count.
  bool RefitGeometry(const SphereGeometry &geom, unsigned int num_primitives = ~0u) {
    return RefitPrims("RefitGeometry(SphereGeometry)", 1, geom.GetCenters(), geom.GetRadii(), num_primitives);
  }
  bool RefitGeometry(const BezierCurveGeometry &geom, unsigned int num_primitives = ~0u) {
    return RefitPrims("RefitGeometry(BezierCurveGeometry)", 3, geom.GetControlPoints(), geom.GetRadii(), num_primitives);
  }
#endif

#if defined(NANORT_ENABLE_SERIALIZATION)
  // Raw host-endian dump: size_t count, nodes, size_t count, indices (ref nanort.h:2164-2276).
  bool Dump(const char *filename) const {
    FILE *fp = fopen(filename, "wb");
    if (!fp) return false;
    const bool ok = Dump(fp);
    fclose(fp);
    return ok;
  }
  bool Dump(FILE *fp) const {
    EnsureHostTree();
    const size_t nn = nodes_.size(), ni = indices_.size();
    if (nn == 0) return false;
    bool ok = fwrite(&nn, sizeof(size_t), 1, fp) == 1;
    ok = ok && fwrite(&nodes_[0], sizeof(BVHNode<T>), nn, fp) == nn;
    ok = ok && fwrite(&ni, sizeof(size_t), 1, fp) == 1;
    ok = ok && (ni == 0 || fwrite(&indices_[0], sizeof(unsigned int), ni, fp) == ni);
    return ok;
  }
  bool Load(const char *filename) {
    FILE *fp = fopen(filename, "rb");
    if (!fp) return false;
    const bool ok = Load(fp);
    fclose(fp);
    return ok;
  }
  bool Load(FILE *fp) {
#ifdef NANORT_USE_HIP_BACKEND
    DropPendingHostTree();
#endif
    size_t nn = 0, ni = 0;
    if (fread(&nn, sizeof(size_t), 1, fp) != 1 || nn == 0) return false;
    nodes_.resize(nn);
    if (fread(&nodes_[0], sizeof(BVHNode<T>), nn, fp) != nn) return false;
    if (fread(&ni, sizeof(size_t), 1, fp) != 1) return false;
    indices_.resize(ni);
    if (ni && fread(&indices_[0], sizeof(unsigned int), ni, fp) != ni) return false;
#ifdef NANORT_USE_HIP_BACKEND
    dev_.tree_stale = true;  // re-uploaded lazily by TraverseBatch once a mesh is known
#endif
    return true;
  }
#endif

  void Debug() {
    EnsureHostTree();
    for (size_t i = 0; i < indices_.size(); i++) printf("index[%d] = %d\n", int(i), int(indices_[i]));
    for (size_t i = 0; i < nodes_.size(); i++) {
      printf("node[%d] : bmin %f, %f, %f, bmax %f, %f, %f\n", int(i), double(nodes_[i].bmin[0]), double(nodes_[i].bmin[1]),
             double(nodes_[i].bmin[2]), double(nodes_[i].bmax[0]), double(nodes_[i].bmax[1]), double(nodes_[i].bmax[2]));
    }
  }

  // Closest hit along one ray (ref nanort.h:757-759, 2487-2556).
  template <class I, class H>
  bool Traverse(const Ray<T> &ray, const I &intersector, H *isect, const BVHTraceOptions &options = BVHTraceOptions()) const {
    EnsureHostTree();
    unsigned int todo[kNANORT_MAX_STACK_DEPTH];
    int top = 0;
    todo[0] = 0;

    T best_t = ray.max_t;
    intersector.Update(best_t, static_cast<unsigned int>(-1));
    intersector.PrepareTraversal(ray, options);

    int dir_sign[3];
    real3<T> dir;
    for (int k = 0; k < 3; k++) {
      dir_sign[k] = ray.dir[k] < static_cast<T>(0.0) ? 1 : 0;
      dir[k] = ray.dir[k];
    }
    const real3<T> inv_dir = vsafe_inverse(dir);
    const real3<T> org(ray.org[0], ray.org[1], ray.org[2]);

    T box_t0, box_t1;
    while (top >= 0) {
      const BVHNode<T> &node = nodes_[todo[top--]];
      if (!IntersectRayAABB(&box_t0, &box_t1, ray.min_t, best_t, node.bmin, node.bmax, org, inv_dir, dir_sign)) continue;
      if (node.flag == 0) {
        const int near_side = dir_sign[node.axis];
        todo[++top] = node.data[1 - near_side];  // far child waits
        todo[++top] = node.data[near_side];      // near child is visited next
        assert(top < kNANORT_MAX_STACK_DEPTH);
      } else {
        T t = intersector.GetT();
        bool any = false;
        for (unsigned int i = 0; i < node.data[0]; i++) {
          const unsigned int prim = indices_[node.data[1] + i];
          T cand = t;
          if (intersector.Intersect(&cand, prim)) {
            t = cand;
            intersector.Update(t, prim);
            any = true;
          }
        }
        if (any) best_t = intersector.GetT();
      }
    }
    const bool hit = intersector.GetT() < ray.max_t;  // strict
    intersector.PostTraversal(ray, hit, isect);
    return hit;
  }

  // The K = max_intersections frontmost hits along one ray, ascending by (t, prim_id) (the reference's declared
  // MultiHitTraverse, nanort.h:761-770 — kept there inside `#if 0` — without its non-deducible comparator).  The contract of
  // include/nanort_hip.h nrtMultiHitTraverseBatch: the binary loop over nodes_ / indices_, slab test on [ray.min_t, B] with
  // B = ray.max_t while fewer than K hits are held, else the t of the worst held hit; a primitive the intersector accepts
  // against B with t < ray.max_t enters when fewer than K are held or when its key is below the worst, which is evicted.
  // Any intersector (Intersect / Update / PostTraversal, as for Traverse); isects receives the held hits only.
  template <class I, class H>
  bool MultiHitTraverse(const Ray<T> &ray, int max_intersections, const I &intersector, StackVector<H, 128> *isects,
                        const BVHTraceOptions &options = BVHTraceOptions()) const {
    EnsureHostTree();
    (*isects)->clear();
    if (max_intersections <= 0) return false;
    const size_t K = static_cast<size_t>(max_intersections);
    struct Held {
      T t;
      unsigned int prim;
      H isect;
    };
    std::vector<Held> held;  // sorted by (t, prim)
    held.reserve(K + 1);
    unsigned int todo[kNANORT_MAX_STACK_DEPTH];
    int top = 0;
    todo[0] = 0;

    T bound = ray.max_t;
    intersector.Update(bound, static_cast<unsigned int>(-1));
    intersector.PrepareTraversal(ray, options);

    int dir_sign[3];
    real3<T> dir;
    for (int k = 0; k < 3; k++) {
      dir_sign[k] = ray.dir[k] < static_cast<T>(0.0) ? 1 : 0;
      dir[k] = ray.dir[k];
    }
    const real3<T> inv_dir = vsafe_inverse(dir);
    const real3<T> org(ray.org[0], ray.org[1], ray.org[2]);

    T box_t0, box_t1;
    while (top >= 0) {
      const BVHNode<T> &node = nodes_[todo[top--]];
      if (!IntersectRayAABB(&box_t0, &box_t1, ray.min_t, bound, node.bmin, node.bmax, org, inv_dir, dir_sign)) continue;
      if (node.flag == 0) {
        const int near_side = dir_sign[node.axis];
        todo[++top] = node.data[1 - near_side];
        todo[++top] = node.data[near_side];
        assert(top < kNANORT_MAX_STACK_DEPTH);
        continue;
      }
      for (unsigned int i = 0; i < node.data[0]; i++) {
        const unsigned int prim = indices_[node.data[1] + i];
        T cand = bound;
        if (!intersector.Intersect(&cand, prim)) continue;
        if (!(cand < ray.max_t)) continue;  // (a NaN t too)
        if (held.size() == K && !(cand < bound || prim < held.back().prim)) continue;  // accepted: cand <= bound
        Held h;
        h.t = cand;
        h.prim = prim;
        intersector.Update(cand, prim);
        intersector.PostTraversal(ray, true, &h.isect);
        size_t j = held.size();
        while (j > 0 && (held[j - 1].t > cand || (held[j - 1].t == cand && held[j - 1].prim > prim))) j--;
        held.insert(held.begin() + static_cast<std::ptrdiff_t>(j), h);
        if (held.size() > K) held.pop_back();
        if (held.size() == K) bound = held.back().t;
      }
    }
    for (size_t j = 0; j < held.size(); j++) (*isects)->push_back(held[j].isect);
    return !held.empty();
  }

  // The K nearest leaf primitives' [t_min, t_max] intervals along the ray, front to back, for
  // two-level traversal (ref nanort.h:781-784, 2558-2692).  `I` is the *interval* intersector
  // concept: PrepareTraversal(ray), Intersect(&t_min, &t_max, prim).
  template <class I>
  bool ListNodeIntersections(const Ray<T> &ray, int max_intersections, const I &intersector,
                             StackVector<NodeHit<T>, 128> *hits) const {
    EnsureHostTree();
    std::priority_queue<NodeHit<T>, std::vector<NodeHit<T> >, NodeHitComparator<T> > farthest_first;
    (*hits)->clear();
    unsigned int todo[kNANORT_MAX_STACK_DEPTH];
    int top = 0;
    todo[0] = 0;
    int dir_sign[3];
    real3<T> dir;
    for (int k = 0; k < 3; k++) {
      dir_sign[k] = ray.dir[k] < static_cast<T>(0.0) ? 1 : 0;
      dir[k] = ray.dir[k];
    }
    const real3<T> inv_dir = vsafe_inverse(dir);
    const real3<T> org(ray.org[0], ray.org[1], ray.org[2]);
    T box_t0, box_t1;
    while (top >= 0) {
      const BVHNode<T> &node = nodes_[todo[top--]];
      if (!IntersectRayAABB(&box_t0, &box_t1, ray.min_t, ray.max_t, node.bmin, node.bmax, org, inv_dir, dir_sign)) continue;
      if (node.flag == 0) {
        const int near_side = dir_sign[node.axis];
        todo[++top] = node.data[1 - near_side];
        todo[++top] = node.data[near_side];
      } else {
        intersector.PrepareTraversal(ray);
        for (unsigned int i = 0; i < node.data[0]; i++) {
          const unsigned int prim = indices_[node.data[1] + i];
          NodeHit<T> h;
          if (!intersector.Intersect(&h.t_min, &h.t_max, prim)) continue;
          h.node_id = prim;
          if (farthest_first.size() < static_cast<size_t>(max_intersections)) {
            farthest_first.push(h);
          } else if (h.t_min < farthest_first.top().t_min) {
            farthest_first.pop();
            farthest_first.push(h);
          }
        }
      }
    }
    if (farthest_first.empty()) return false;
    const size_t n = farthest_first.size();
    (*hits)->resize(n);
    for (size_t i = 0; i < n; i++) {
      (*hits)[n - i - 1] = farthest_first.top();
      farthest_first.pop();
    }
    return true;
  }

  // The batch call on the HOST, with or without NANORT_USE_HIP_BACKEND and for any intersector: N calls of Traverse(), ray i
  // through a copy of `intersector` of its own and with its own options — `options` with skip_prim_id replaced by
  // skip_prim_ids[i] when the array is given (the contract of include/nanort_hip.h, "per-ray skip ids": 0xFFFFFFFF or an id
  // that names no primitive skips nothing).  isects[i] is written only when ray i hits; hit_out[i] (optional) receives 1 / 0.
  template <class I, class H>
  bool TraverseBatch(const Ray<T> *rays, size_t num_rays, const I &intersector, H *isects, unsigned char *hit_out = NULL,
                     const BVHTraceOptions &options = BVHTraceOptions(), const unsigned int *skip_prim_ids = NULL) const {
    for (size_t i = 0; i < num_rays; i++) {
      const I ray_intersector(intersector);
      BVHTraceOptions ray_options(options);
      if (skip_prim_ids) ray_options.skip_prim_id = skip_prim_ids[i];
      H isect;
      const bool hit = Traverse(rays[i], ray_intersector, &isect, ray_options);
      if (hit) isects[i] = isect;
      if (hit_out) hit_out[i] = hit ? 1 : 0;
    }
    return true;
  }
  // The occlusion query on the HOST, with or without NANORT_USE_HIP_BACKEND and for any intersector whose intersection record is
  // H: occluded_out[i] is 1 / 0, the flag of Traverse() for ray i through a copy of `intersector` of its own.  This is the
  // statement of what OccludedBatchSpheres / OccludedBatchCylinders / OccludedBatchCurves (and nrtOccludedBatchPrims_f32) answer.
  template <class I, class H>
  bool OccludedBatch(const Ray<T> *rays, size_t num_rays, const I &intersector, unsigned char *occluded_out,
                     const BVHTraceOptions &options = BVHTraceOptions()) const {
    for (size_t i = 0; i < num_rays; i++) {
      const I ray_intersector(intersector);
      H isect;
      occluded_out[i] = Traverse(rays[i], ray_intersector, &isect, options) ? 1 : 0;
    }
    return true;
  }
  // The combined query on the HOST, with or without NANORT_USE_HIP_BACKEND (BatchQuery and QueryTriangleIntersector above; the
  // contract of include/nanort_hip.h, "one descriptor for every triangle ray query"): N calls of Traverse(), ray i through a copy of
  // `intersector` of its own on which SetRay() was called with the ray's time (q.motion: q.times[i], or 0), word (q.masked:
  // q.ray_masks[i], or 0xFFFFFFFF) and skip id (q.skip_prim_ids[i], or q.options.skip_prim_id).  It is the caller who gives
  // `intersector` keyframe 1 for a q.motion query and the primitives' words for a q.masked one.  Every record is written (a miss:
  // {0, 0, ray.max_t, 0xFFFFFFFF}); with q.occlusion only q.hit_out.  Returns false, nothing written, when the query has rays and
  // lacks them or its output.
  bool TraverseBatchQuery(const BatchQuery<T> &q, const QueryTriangleIntersector<T> &intersector) const {
    if (q.num_rays && (!q.rays || !(q.occlusion ? static_cast<const void *>(q.hit_out) : static_cast<const void *>(q.isects)))) return false;
    for (size_t i = 0; i < q.num_rays; i++) {
      const QueryTriangleIntersector<T> ray_intersector(intersector);
      ray_intersector.SetRay((q.motion && q.times) ? q.times[i] : static_cast<T>(0.0), (q.masked && q.ray_masks) ? q.ray_masks[i] : 0xFFFFFFFFu,
                             q.skip_prim_ids ? q.skip_prim_ids[i] : q.options.skip_prim_id);
      TriangleIntersection<T> isect;
      const bool hit = Traverse(q.rays[i], ray_intersector, &isect, q.options);
      if (!q.occlusion) {
        TriangleIntersection<T> &out = q.isects[i];  // (field by field: the caller's padding bytes stay the caller's)
        out.u = hit ? isect.u : static_cast<T>(0.0);
        out.v = hit ? isect.v : static_cast<T>(0.0);
        out.t = hit ? isect.t : q.rays[i].max_t;
        out.prim_id = hit ? isect.prim_id : 0xFFFFFFFFu;
      }
      if (q.hit_out) q.hit_out[i] = hit ? 1 : 0;
    }
    return true;
  }

  // Multi-hit under the combined intersector on the HOST, with or without NANORT_USE_HIP_BACKEND (MultiHitBatchQuery above; the
  // contract of include/nanort_hip.h, nrtMultiHitQueryBatch): N calls of MultiHitTraverse(), ray i through a copy of `intersector` of
  // its own on which SetRay() was called as TraverseBatchQuery() does.  Rows and counts in the library's layout, miss records
  // included.  Returns false, nothing written, when max_hits is outside 1..64 or the query has rays and lacks them or its rows.
  bool MultiHitTraverseBatchQuery(const MultiHitBatchQuery<T> &q, const QueryTriangleIntersector<T> &intersector) const {
    if (q.max_hits == 0 || q.max_hits > 64) return false;
    if (q.num_rays && (!q.rays || !q.isects)) return false;
    StackVector<TriangleIntersection<T>, 128> held;
    for (size_t i = 0; i < q.num_rays; i++) {
      const QueryTriangleIntersector<T> ray_intersector(intersector);
      ray_intersector.SetRay((q.motion && q.times) ? q.times[i] : static_cast<T>(0.0), (q.masked && q.ray_masks) ? q.ray_masks[i] : 0xFFFFFFFFu,
                             q.skip_prim_ids ? q.skip_prim_ids[i] : q.options.skip_prim_id);
      MultiHitTraverse(q.rays[i], static_cast<int>(q.max_hits), ray_intersector, &held, q.options);
      const size_t count = held->size();
      for (size_t j = 0; j < q.max_hits; j++) {
        TriangleIntersection<T> &out = q.isects[i * q.max_hits + j];  // (field by field: the caller's padding bytes stay the caller's)
        out.u = j < count ? held[j].u : static_cast<T>(0.0);
        out.v = j < count ? held[j].v : static_cast<T>(0.0);
        out.t = j < count ? held[j].t : q.rays[i].max_t;
        out.prim_id = j < count ? held[j].prim_id : 0xFFFFFFFFu;
      }
      if (q.counts_out) q.counts_out[i] = static_cast<unsigned int>(count);
    }
    return true;
  }

  // The nearest face of `mesh` to the point `p` and where on it, among the faces `options` admits (prim_ids_range, skip_prim_id;
  // cull_back_face is ignored) and within max_dist — on the HOST, with or without NANORT_USE_HIP_BACKEND.  The rule is
  // nanort_closest.h's: the smallest dist2, among equal dist2 the smallest prim_id, so the answer does not depend on the tree; the
  // walk of nodes_ enters the nearer child first and skips a subtree iff its box lies strictly farther than the best so far.
  // Returns whether a face was found; *out is written either way (ClosestPointResult above).  `mesh`: the one the tree was built over.
  bool ClosestPoint(const T p[3], T max_dist, const TriangleMesh<T> &mesh, const BVHTraceOptions &options, ClosestPointResult<T> *out) const {
    unsigned int feature;
    return ClosestWalk(p, max_dist, mesh, options, out, &feature);
  }
  // The walk behind ClosestPoint() and SignedDistance(): *feature receives the winning candidate's code of the answer (0: none).
  bool ClosestWalk(const T p[3], T max_dist, const TriangleMesh<T> &mesh, const BVHTraceOptions &options, ClosestPointResult<T> *out,
                   unsigned int *feature) const {
    EnsureHostTree();
    *feature = 0u;
    out->point[0] = p[0], out->point[1] = p[1], out->point[2] = p[2];
    out->dist2 = max_dist * max_dist;
    out->u = out->v = static_cast<T>(0.0);
    out->prim_id = 0xFFFFFFFFu;
    out->pad = 0u;
    if (nodes_.empty() || !nanort_closest::Searchable<T>(p, max_dist)) return false;
    std::vector<unsigned int> todo(1, 0u);  // (a vector: no depth limit)
    while (!todo.empty()) {
      const BVHNode<T> &node = nodes_[todo.back()];
      todo.pop_back();
      if (nanort_closest::Culled<T>(nanort_closest::BoxDist2<T>(p, node.bmin, node.bmax), out->dist2)) continue;
      if (node.flag == 0) {
        const BVHNode<T> &n0 = nodes_[node.data[0]], &n1 = nodes_[node.data[1]];
        const T d0 = nanort_closest::BoxDist2<T>(p, n0.bmin, n0.bmax), d1 = nanort_closest::BoxDist2<T>(p, n1.bmin, n1.bmax);
        const bool second = d1 < d0;  // on ties the first child
        if (!nanort_closest::Culled<T>(second ? d0 : d1, out->dist2)) todo.push_back(node.data[second ? 0 : 1]);  // the farther child waits
        if (!nanort_closest::Culled<T>(second ? d1 : d0, out->dist2)) todo.push_back(node.data[second ? 1 : 0]);
      } else {
        for (unsigned int i = 0; i < node.data[0]; i++) {
          const unsigned int prim = indices_[node.data[1] + i];
          if (prim < options.prim_ids_range[0] || prim >= options.prim_ids_range[1] || prim == options.skip_prim_id) continue;
          const T *a = get_vertex_addr<T>(mesh.vertices_, mesh.faces_[3 * prim + 0], mesh.vertex_stride_bytes_);
          const T *b = get_vertex_addr<T>(mesh.vertices_, mesh.faces_[3 * prim + 1], mesh.vertex_stride_bytes_);
          const T *c = get_vertex_addr<T>(mesh.vertices_, mesh.faces_[3 * prim + 2], mesh.vertex_stride_bytes_);
          T u, v, q[3];
          unsigned int f;
          const T dist2 = nanort_closest::ClosestFeatureOnTriangle<T>(p, a, b, c, &u, &v, q, &f);
          if (!nanort_closest::Better<T>(dist2, prim, out->dist2, out->prim_id)) continue;
          out->point[0] = q[0], out->point[1] = q[1], out->point[2] = q[2];
          out->dist2 = dist2;
          out->u = u, out->v = v;
          out->prim_id = prim;
          *feature = f;
        }
      }
    }
    return out->prim_id != 0xFFFFFFFFu;
  }
  // ClosestPoint(), and on which side of the surface p lies (nanort_sdf.h: the sign of (p - point) . n for the pseudonormal n of
  // the feature that holds the nearest point) — on the HOST, with or without the backend.  `normals`: FeatureNormals of `mesh`,
  // always of the WHOLE mesh, whatever faces `options` admits.  Returns whether a face was found.
  bool SignedDistance(const T p[3], T max_dist, const TriangleMesh<T> &mesh, const FeatureNormals<T> &normals, const BVHTraceOptions &options,
                      SignedDistanceResult<T> *out) const {
    static_assert(sizeof(SignedDistanceResult<T>) == sizeof(ClosestPointResult<T>), "a signed record is a closest-point record");
    ClosestPointResult<T> r;
    unsigned int feature;
    const bool found = ClosestWalk(p, max_dist, mesh, options, &r, &feature);
    out->point[0] = r.point[0], out->point[1] = r.point[1], out->point[2] = r.point[2];
    out->dist2 = r.dist2, out->u = r.u, out->v = r.v, out->prim_id = r.prim_id;
    out->feature = found ? nanort_sdf::FeatureWord<T>(p, r.point, normals.Of(mesh, r.prim_id, feature), feature) : 0u;
    return found;
  }
  bool SignedDistanceBatchHost(const T *points, const T *max_dists, size_t num_points, const TriangleMesh<T> &mesh, const FeatureNormals<T> &normals,
                               SignedDistanceResult<T> *out, unsigned char *found_out = NULL, const BVHTraceOptions &options = BVHTraceOptions()) const {
    for (size_t i = 0; i < num_points; i++) {
      const bool found = SignedDistance(points + 3 * i, max_dists ? max_dists[i] : std::numeric_limits<T>::infinity(), mesh, normals, options, &out[i]);
      if (found_out) found_out[i] = found ? 1 : 0;
    }
    return true;
  }
  // The batch call: with NANORT_USE_HIP_BACKEND and a triangle tree on the GPU one launch of nrtSignedDistanceBatch, which signs with
  // the normals the GPU derived from its own copy of the mesh (`normals` is not read: point, dist2, u, v, prim_id and the feature code
  // are byte-identical to the host loop's, the sign may differ where (p - point) . n is within rounding of 0 at a vertex); the host
  // loop otherwise.
  bool SignedDistanceBatch(const T *points, const T *max_dists, size_t num_points, const TriangleMesh<T> &mesh, const FeatureNormals<T> &normals,
                           SignedDistanceResult<T> *out, unsigned char *found_out = NULL, const BVHTraceOptions &options = BVHTraceOptions()) const {
#ifdef NANORT_USE_HIP_BACKEND
    if (dev_.ctx && geom_.kind == 0) return SignedDistanceBatchBackend(points, max_dists, num_points, out, found_out, options);
#endif
    return SignedDistanceBatchHost(points, max_dists, num_points, mesh, normals, out, found_out, options);
  }
  // ... for `num_points` points, point i at points[3 * i] with max_dists[i] (NULL: +inf for every point): N calls of ClosestPoint().
  // Every record is written; found_out[i] (optional) receives 1 / 0.
  bool ClosestPointBatchHost(const T *points, const T *max_dists, size_t num_points, const TriangleMesh<T> &mesh, ClosestPointResult<T> *out,
                             unsigned char *found_out = NULL, const BVHTraceOptions &options = BVHTraceOptions()) const {
    for (size_t i = 0; i < num_points; i++) {
      const bool found = ClosestPoint(points + 3 * i, max_dists ? max_dists[i] : std::numeric_limits<T>::infinity(), mesh, options, &out[i]);
      if (found_out) found_out[i] = found ? 1 : 0;
    }
    return true;
  }
  // The batch call: with NANORT_USE_HIP_BACKEND and a triangle tree on the GPU one launch of nrtClosestPointBatch (records
  // byte-identical to the host loop's: the answer does not depend on the tree or on who walks it), the host loop otherwise.
  bool ClosestPointBatch(const T *points, const T *max_dists, size_t num_points, const TriangleMesh<T> &mesh, ClosestPointResult<T> *out,
                         unsigned char *found_out = NULL, const BVHTraceOptions &options = BVHTraceOptions()) const {
#ifdef NANORT_USE_HIP_BACKEND
    if (dev_.ctx && geom_.kind == 0) return ClosestPointBatchBackend(points, max_dists, num_points, out, found_out, options);
#endif
    return ClosestPointBatchHost(points, max_dists, num_points, mesh, out, found_out, options);
  }

  // The `max_faces` nearest faces of `mesh` to the point `p`, in order — on the HOST, with or without NANORT_USE_HIP_BACKEND.  The
  // rule is nanort_closest.h's K-nearest rule: the candidates are the faces `options` admits (as ClosestPoint) with dist2 <= max_dist^2,
  // ranked by (dist2, prim_id) ascending, so the answer does not depend on the tree; the walk of nodes_ is ClosestPoint's with the
  // bound at the worst held dist2 once max_faces are held.  out[0 .. *count) receives the found records, out[*count .. max_faces) the
  // not-found record of ClosestPoint; `count` may be NULL.  Returns false (and writes nothing) when max_faces is 0.
  bool NearestFaces(const T p[3], T max_dist, unsigned int max_faces, const TriangleMesh<T> &mesh, const BVHTraceOptions &options,
                    ClosestPointResult<T> *out, unsigned int *count = NULL) const {
    if (max_faces == 0) return false;
    EnsureHostTree();
    const T r2 = max_dist * max_dist;
    unsigned int held = 0;
    if (!nodes_.empty() && nanort_closest::Searchable<T>(p, max_dist)) {
      std::vector<unsigned int> todo(1, 0u);  // (a vector: no depth limit)
      while (!todo.empty()) {
        const BVHNode<T> &node = nodes_[todo.back()];
        todo.pop_back();
        const T bound = nanort_closest::NearestBound<T>(held, max_faces, r2, held ? out[held - 1].dist2 : r2);
        if (nanort_closest::Culled<T>(nanort_closest::BoxDist2<T>(p, node.bmin, node.bmax), bound)) continue;
        if (node.flag == 0) {
          const BVHNode<T> &n0 = nodes_[node.data[0]], &n1 = nodes_[node.data[1]];
          const T d0 = nanort_closest::BoxDist2<T>(p, n0.bmin, n0.bmax), d1 = nanort_closest::BoxDist2<T>(p, n1.bmin, n1.bmax);
          const bool second = d1 < d0;  // on ties the first child
          if (!nanort_closest::Culled<T>(second ? d0 : d1, bound)) todo.push_back(node.data[second ? 0 : 1]);  // the farther child waits
          if (!nanort_closest::Culled<T>(second ? d1 : d0, bound)) todo.push_back(node.data[second ? 1 : 0]);
        } else {
          for (unsigned int i = 0; i < node.data[0]; i++) {
            const unsigned int prim = indices_[node.data[1] + i];
            if (prim < options.prim_ids_range[0] || prim >= options.prim_ids_range[1] || prim == options.skip_prim_id) continue;
            const T *a = get_vertex_addr<T>(mesh.vertices_, mesh.faces_[3 * prim + 0], mesh.vertex_stride_bytes_);
            const T *b = get_vertex_addr<T>(mesh.vertices_, mesh.faces_[3 * prim + 1], mesh.vertex_stride_bytes_);
            const T *c = get_vertex_addr<T>(mesh.vertices_, mesh.faces_[3 * prim + 2], mesh.vertex_stride_bytes_);
            ClosestPointResult<T> rec;
            rec.dist2 = nanort_closest::ClosestPointOnTriangle<T>(p, a, b, c, &rec.u, &rec.v, rec.point);
            rec.prim_id = prim;
            rec.pad = 0u;
            const bool full = held == max_faces;
            if (!nanort_closest::NearestEnters<T>(rec.dist2, prim, r2, held, max_faces, full ? out[held - 1].dist2 : r2,
                                                  full ? out[held - 1].prim_id : 0xFFFFFFFFu))
              continue;
            held = nanort_closest::NearestInsert(out, held, max_faces, rec);
          }
        }
      }
    }
    for (unsigned int j = held; j < max_faces; j++) {
      out[j].point[0] = p[0], out[j].point[1] = p[1], out[j].point[2] = p[2];
      out[j].dist2 = r2;
      out[j].u = out[j].v = static_cast<T>(0.0);
      out[j].prim_id = 0xFFFFFFFFu;
      out[j].pad = 0u;
    }
    if (count) *count = held;
    return true;
  }
  // ... for `num_points` points, point i at points[3 * i] with max_dists[i] (NULL: +inf for every point): N calls of NearestFaces(),
  // row i at out[i * max_faces].  Every record is written; counts_out[i] (optional) receives the count.
  bool NearestFacesBatchHost(const T *points, const T *max_dists, size_t num_points, unsigned int max_faces, const TriangleMesh<T> &mesh,
                             ClosestPointResult<T> *out, unsigned int *counts_out = NULL, const BVHTraceOptions &options = BVHTraceOptions()) const {
    if (max_faces == 0) return false;
    for (size_t i = 0; i < num_points; i++)
      NearestFaces(points + 3 * i, max_dists ? max_dists[i] : std::numeric_limits<T>::infinity(), max_faces, mesh, options, out + i * max_faces,
                   counts_out ? counts_out + i : NULL);
    return true;
  }
  // The batch call: with NANORT_USE_HIP_BACKEND and a triangle tree on the GPU one call of nrtNearestFacesBatch (max_faces up to
  // NRT_MAX_NEAREST; rows byte-identical to the host loop's), the host loop otherwise.
  bool NearestFacesBatch(const T *points, const T *max_dists, size_t num_points, unsigned int max_faces, const TriangleMesh<T> &mesh,
                         ClosestPointResult<T> *out, unsigned int *counts_out = NULL, const BVHTraceOptions &options = BVHTraceOptions()) const {
#ifdef NANORT_USE_HIP_BACKEND
    if (dev_.ctx && geom_.kind == 0) return NearestFacesBatchBackend(points, max_dists, num_points, max_faces, out, counts_out, options);
#endif
    return NearestFacesBatchHost(points, max_dists, num_points, max_faces, mesh, out, counts_out, options);
  }

#ifdef NANORT_USE_HIP_BACKEND
  // Closest hit for each of `num_rays` rays in one GPU launch.  isects[i] is written only when
  // ray i hits (exactly like N calls of Traverse()); hit_out[i] (optional) receives 1 / 0.
  // Requires a tree built by Build() with the built-in triangle types (or Load() after such a
  // Build set the mesh).  Returns false and leaves the outputs untouched on a backend error
  // (LastBackendError() tells why).
  // Threads: the batch methods below (const, like Traverse()) may be called on one object from many threads at once.  A
  // per-object mutex (batch_mutex_, a fresh one for every copy) guards the shared staging buffers from the launch to the
  // scatter into the caller's arrays, and the lazy device-side updates (the upload of a Load()ed tree, the cylinder cap
  // re-send, a copy-on-write detach); calls on one object are thereby serialised, calls on different objects (copies
  // included) are not.
  // `skip_prim_ids` (here and on the Device / Occluded / Batches forms below; triangle accels): one id per ray, traced in the place
  // of options.skip_prim_id for that ray — a bounce or shadow wave whose rays leave different triangles needs no epsilon
  // (include/nanort_hip.h, "per-ray skip ids"; NULL: the call as it always was).  On a multi-device accel such a batch is traced
  // by the first device alone: the records are the same.
  bool TraverseBatch(const Ray<T> *rays, size_t num_rays, TriangleIntersection<T> *isects, unsigned char *hit_out = NULL,
                     const BVHTraceOptions &options = BVHTraceOptions(), const unsigned int *skip_prim_ids = NULL) const {
    return TraverseBatchImpl(rays, num_rays, isects, hit_out, options, skip_prim_ids);
  }
  // The same launch for callers that keep their ray waves in HBM (a wavefront renderer whose shading runs on the GPU):
  // `d_rays`, `d_isects`, `d_hit` are device pointers, the call is asynchronous on `hip_stream` (a hipStream_t).
  // Unlike the host variant every record is written: a miss stores {u = 0, v = 0, t = ray.max_t, prim_id = 0xFFFFFFFF}.
  // Launches on different streams may overlap on the GPU.
  bool TraverseBatchDevice(const Ray<T> *d_rays, size_t num_rays, TriangleIntersection<T> *d_isects, unsigned char *d_hit,
                           void *hip_stream, const BVHTraceOptions &options = BVHTraceOptions(), const unsigned int *d_skip_prim_ids = NULL) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!TriangleTreeOnDevice("TraverseBatchDevice: no triangle tree on the GPU (Build() with the built-in triangle types, or TraverseBatch() once after Load())")) return false;
    const nrt_trace_options o = TraceOptions(options);
    return Ok(d_skip_prim_ids ? Api::TraverseSkipDevice(Context(), Pod(d_rays), num_rays, &o, d_skip_prim_ids, Pod(d_isects), d_hit, hip_stream)
                              : Api::TraverseDevice(Context(), Pod(d_rays), num_rays, &o, Pod(d_isects), d_hit, hip_stream));
  }
  // Several independent device-resident waves in ONE launch (nrtTraverseBatchesDevice): `occlusion[k]` != 0 makes wave k an
  // occlusion query (only d_hit[k] is written, d_isects[k] may be NULL).  One launch tail for all the waves — a renderer's
  // shadow query and next path wave, without a second stream.  Records equal those of separate calls.  `occlusion` may be NULL.
  bool TraverseBatchesDevice(size_t num_waves, const Ray<T> *const *d_rays, const size_t *num_rays, TriangleIntersection<T> *const *d_isects,
                             unsigned char *const *d_hit, const unsigned char *occlusion, void *hip_stream,
                             const BVHTraceOptions &options = BVHTraceOptions(), const unsigned int *const *d_skip_prim_ids = NULL) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!TriangleTreeOnDevice("TraverseBatchesDevice: no triangle tree on the GPU")) return false;
    const nrt_trace_options o = TraceOptions(options);
    std::vector<const RayPod *> r(num_waves);
    std::vector<HitPod *> h(num_waves);
    std::vector<uint8_t *> m(num_waves);
    std::vector<uint64_t> n(num_waves);
    std::vector<uint32_t> fl(num_waves);
    for (size_t k = 0; k < num_waves; k++) {
      r[k] = Pod(d_rays[k]);
      h[k] = Pod(d_isects ? d_isects[k] : NULL);
      m[k] = d_hit ? d_hit[k] : NULL;
      n[k] = num_rays[k];
      fl[k] = (occlusion && occlusion[k]) ? NRT_BATCH_OCCLUSION : 0u;
    }
    const uint32_t nw = static_cast<uint32_t>(num_waves);
    return Ok(d_skip_prim_ids ? Api::TraverseBatchesSkip(Context(), nw, r.data(), n.data(), &o, d_skip_prim_ids, h.data(), m.data(), fl.data(), hip_stream)
                              : Api::TraverseBatches(Context(), nw, r.data(), n.data(), &o, h.data(), m.data(), fl.data(), hip_stream));
  }
  // Several independent HOST waves in ONE launch (nrtTraverseBatches): what a host-shaded wavefront renderer has ready at the
  // same time — the shadow query of one depth and the path wave of the next — uploaded together, walked by one persistent
  // launch (one launch tail instead of one per wave), downloaded together.  `occlusion[k]` != 0 makes wave k an occlusion
  // query: only hit_out[k] (required) is written.  For the other waves isects[k][i] is written only on a hit, like
  // TraverseBatch(); hit_out[k] may be NULL.  Records and flags are exactly those of separate TraverseBatch() /
  // OccludedBatch() calls.  `occlusion` may be NULL.
  bool TraverseBatches(size_t num_waves, const Ray<T> *const *rays, const size_t *num_rays, TriangleIntersection<T> *const *isects,
                       unsigned char *const *hit_out, const unsigned char *occlusion, const BVHTraceOptions &options = BVHTraceOptions(),
                       const unsigned int *const *skip_prim_ids = NULL) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!DeviceTreeReady(0)) return false;  // (context, primitive kind, a tree adopted by Load())
    size_t total = 0;
    for (size_t k = 0; k < num_waves; k++) total += num_rays[k];
    if (total == 0) return true;
    HitPod *tmp = static_cast<HitPod *>(StageEnsure(&stage_hits_, &stage_hits_cap_, total * sizeof(HitPod)));
    unsigned char *tmask = static_cast<unsigned char *>(StageEnsure(&stage_mask_, &stage_mask_cap_, total));
    if (!tmp || !tmask) {
      backend_error_ = "TraverseBatches: out of host memory for the staging buffers";
      return false;
    }
    std::vector<const RayPod *> r(num_waves);
    std::vector<HitPod *> h(num_waves);
    std::vector<uint8_t *> m(num_waves);
    std::vector<uint64_t> n(num_waves);
    std::vector<uint32_t> fl(num_waves);
    size_t off = 0;
    for (size_t k = 0; k < num_waves; k++) {
      const bool occ = occlusion && occlusion[k];
      if (num_rays[k] && occ && !(hit_out && hit_out[k])) {
        backend_error_ = "TraverseBatches: an occlusion wave needs its hit_out array";
        return false;
      }
      r[k] = Pod(rays[k]);
      h[k] = occ ? NULL : tmp + off;
      m[k] = (hit_out && hit_out[k]) ? hit_out[k] : tmask + off;
      n[k] = num_rays[k];
      fl[k] = occ ? NRT_BATCH_OCCLUSION : 0u;
      off += num_rays[k];
    }
    const nrt_trace_options o = TraceOptions(options);
    const uint32_t nw = static_cast<uint32_t>(num_waves);
    if (!Ok(skip_prim_ids ? Api::TraverseBatchesSkipHost(Context(), nw, r.data(), n.data(), &o, skip_prim_ids, h.data(), m.data(), fl.data())
                          : Api::TraverseBatchesHost(Context(), nw, r.data(), n.data(), &o, h.data(), m.data(), fl.data())))
      return false;
    for (size_t k = 0; k < num_waves; k++) {
      if (fl[k] || !isects || !isects[k]) continue;
      const HitPod *src = h[k];
      const uint8_t *mk = m[k];
      TriangleIntersection<T> *dst = isects[k];
      for (size_t i = 0; i < num_rays[k]; i++)
        if (mk[i]) std::memcpy(static_cast<void *>(&dst[i]), &src[i], sizeof(HitPod));
    }
    return true;
  }
  // Opt-in extension without a reference counterpart: occlusion queries.  occluded_out[i] is exactly what
  // TraverseBatch() would report in hit_out[i], but a ray stops at the first primitive it accepts (shadow rays).
  bool OccludedBatch(const Ray<T> *rays, size_t num_rays, unsigned char *occluded_out, const BVHTraceOptions &options = BVHTraceOptions(),
                     const unsigned int *skip_prim_ids = NULL) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!TriangleTreeOnDevice("OccludedBatch: no triangle tree on the GPU (Build() with the built-in triangle types, or TraverseBatch() once after Load())")) return false;
    const nrt_trace_options o = TraceOptions(options);
    return Ok(skip_prim_ids ? Api::OccludedSkip(Context(), Pod(rays), num_rays, &o, skip_prim_ids, occluded_out)
                            : Api::Occluded(Context(), Pod(rays), num_rays, &o, occluded_out));
  }
  // ... and with device pointers, asynchronous on `hip_stream` (see TraverseBatchDevice).
  bool OccludedBatchDevice(const Ray<T> *d_rays, size_t num_rays, unsigned char *d_occluded, void *hip_stream,
                           const BVHTraceOptions &options = BVHTraceOptions(), const unsigned int *d_skip_prim_ids = NULL) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!TriangleTreeOnDevice("OccludedBatchDevice: no triangle tree on the GPU")) return false;
    const nrt_trace_options o = TraceOptions(options);
    return Ok(d_skip_prim_ids ? Api::OccludedSkipDevice(Context(), Pod(d_rays), num_rays, &o, d_skip_prim_ids, d_occluded, hip_stream)
                              : Api::OccludedDevice(Context(), Pod(d_rays), num_rays, &o, d_occluded, hip_stream));
  }
  // The max_hits frontmost hits of each of `num_rays` rays in one GPU launch (nrtMultiHitTraverseBatch: the contract of
  // MultiHitTraverse above, on a GPU-built or adopted triangle tree).  isects[i * max_hits + j] holds ray i's hits in ascending
  // (t, prim_id) order, then miss records {0, 0, ray.max_t, 0xFFFFFFFF}; counts_out[i] (may be NULL) how many it holds.
  bool MultiHitTraverseBatch(const Ray<T> *rays, size_t num_rays, unsigned int max_hits, TriangleIntersection<T> *isects,
                             unsigned int *counts_out = NULL, const BVHTraceOptions &options = BVHTraceOptions()) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!DeviceTreeReady(0)) return false;  // (context, primitive kind, a tree adopted by Load())
    const nrt_trace_options o = TraceOptions(options);
    return Ok(Api::MultiHit(Context(), Pod(rays), num_rays, max_hits, &o, Pod(isects), counts_out));
  }
  // Motion blur (include/nanort_hip.h, "motion blur"): the closest hit of each of `num_rays` rays at its own time, over a tree built
  // by Build() with MotionTriangleMesh / MotionTriangleSAHPred.  times[i] is ray i's time (clamped to [0, 1]; NULL: every ray at
  // time 0).  EVERY record is written — a miss stores {0, 0, ray.max_t, 0xFFFFFFFF} — and each equals what the per-ray Traverse()
  // with a MotionTriangleIntersector set to that time gives over the same tree; hit_out[i] (optional) receives 1 / 0.
  bool TraverseBatchMotion(const Ray<T> *rays, const T *times, size_t num_rays, TriangleIntersection<T> *isects, unsigned char *hit_out = NULL,
                           const BVHTraceOptions &options = BVHTraceOptions()) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!MotionTreeReady("TraverseBatchMotion")) return false;
    const nrt_trace_options o = TraceOptions(options);
    return Ok(Api::TraverseMotion(Context(), Pod(rays), times, num_rays, &o, Pod(isects), hit_out));
  }
  // ... and its occlusion query: occluded_out[i] is exactly the hit_out[i] of TraverseBatchMotion().
  bool OccludedBatchMotion(const Ray<T> *rays, const T *times, size_t num_rays, unsigned char *occluded_out,
                           const BVHTraceOptions &options = BVHTraceOptions()) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!MotionTreeReady("OccludedBatchMotion")) return false;
    const nrt_trace_options o = TraceOptions(options);
    return Ok(Api::OccludedMotion(Context(), Pod(rays), times, num_rays, &o, occluded_out));
  }
  // Visibility masks (include/nanort_hip.h, "visibility masks"): one word per primitive of the triangle mesh the accel was built
  // over (`count` must be its primitive count; NULL removes the masks).  The array is copied to the GPU now and kept by pointer, as
  // Build() keeps the mesh's arrays (a copy-on-write detach sends it again): it must outlive the accel or the next SetPrimMasks().
  // The tree is untouched: no Build(), no Refit().  An object that shares its contexts with copies first moves to contexts of its
  // own, so the copies keep their visibility.  Build() over a new mesh drops the masks.
  bool SetPrimMasks(const unsigned int *prim_masks, size_t count) {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!dev_.ctx || geom_.kind != 0) {
      backend_error_ = "SetPrimMasks: no triangle mesh on the GPU (Build() with the built-in triangle types first)";
      return false;
    }
    if (prim_masks && count != geom_.count) {
      backend_error_ = "SetPrimMasks: count differs from the number of primitives the tree was built over";
      return false;
    }
    if (!RefitContexts(0, [&](nrt_ctx *c) { return nrtSetPrimMasks(c, prim_masks, count); })) return false;
    geom_.masks = prim_masks;
    return true;
  }
  // The closest hit of each of `num_rays` rays among the triangles it sees: ray i sees primitive p iff (prim_masks[p] & ray_masks[i])
  // != 0 (ray_masks == NULL: every ray 0xFFFFFFFF).  EVERY record is written — a miss stores {0, 0, ray.max_t, 0xFFFFFFFF} — and each
  // equals what the per-ray Traverse() with a MaskedTriangleIntersector set to that ray's mask gives over the same tree; hit_out[i]
  // (optional) receives 1 / 0.
  bool TraverseBatchMasked(const Ray<T> *rays, const unsigned int *ray_masks, size_t num_rays, TriangleIntersection<T> *isects,
                           unsigned char *hit_out = NULL, const BVHTraceOptions &options = BVHTraceOptions()) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!MaskedTreeReady("TraverseBatchMasked")) return false;
    const nrt_trace_options o = TraceOptions(options);
    return Ok(Api::TraverseMasked(Context(), Pod(rays), ray_masks, num_rays, &o, Pod(isects), hit_out));
  }
  // ... and its occlusion query: occluded_out[i] is exactly the hit_out[i] of TraverseBatchMasked().
  bool OccludedBatchMasked(const Ray<T> *rays, const unsigned int *ray_masks, size_t num_rays, unsigned char *occluded_out,
                           const BVHTraceOptions &options = BVHTraceOptions()) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!MaskedTreeReady("OccludedBatchMasked")) return false;
    const nrt_trace_options o = TraceOptions(options);
    return Ok(Api::OccludedMasked(Context(), Pod(rays), ray_masks, num_rays, &o, occluded_out));
  }
  // The combined query on the GPU (nrtQueryBatch: include/nanort_hip.h, "one descriptor for every triangle ray query"): each ray
  // at its own time (q.motion: a tree built with MotionTriangleMesh), among the triangles it sees (q.masked: SetPrimMasks() first)
  // and other than the one it left (q.skip_prim_ids).  Records and flags equal those of the host form above, TraverseBatchQuery(q,
  // intersector), over the same tree.  A query with one of the three alone is the existing call for it.
  bool TraverseBatchQuery(const BatchQuery<T> &q) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!QueryTreeReady(q, "TraverseBatchQuery")) return false;
    const nrt_trace_options o = TraceOptions(q.options);
    const typename Api::QueryPod d = QueryDescriptor(q, &o);
    return Ok(Api::Query(Context(), &d));
  }
  // ... and with device pointers in every array of `q`, asynchronous on `hip_stream` (see TraverseBatchDevice).
  bool TraverseBatchQueryDevice(const BatchQuery<T> &q, void *hip_stream) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!TriangleTreeOnDevice("TraverseBatchQueryDevice: no triangle tree on the GPU") || !QueryTreeReady(q, "TraverseBatchQueryDevice")) return false;
    const nrt_trace_options o = TraceOptions(q.options);
    const typename Api::QueryPod d = QueryDescriptor(q, &o);
    return Ok(Api::QueryDevice(Context(), &d, hip_stream));
  }
  // Multi-hit under the combined intersector on the GPU (nrtMultiHitQueryBatch): rows and counts equal those of the host form above,
  // MultiHitTraverseBatchQuery(q, intersector), over the same tree.  A query with none of the three is MultiHitTraverseBatch().
  bool MultiHitTraverseBatchQuery(const MultiHitBatchQuery<T> &q) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!QueryTreeReady(q, "MultiHitTraverseBatchQuery")) return false;
    const nrt_trace_options o = TraceOptions(q.options);
    const typename Api::MultiHitQueryPod d = MultiHitQueryDescriptor(q, &o);
    return Ok(Api::MultiHitQuery(Context(), &d));
  }
  // ... and with device pointers in every array of `q`, asynchronous on `hip_stream` (see TraverseBatchDevice).
  bool MultiHitTraverseBatchQueryDevice(const MultiHitBatchQuery<T> &q, void *hip_stream) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!TriangleTreeOnDevice("MultiHitTraverseBatchQueryDevice: no triangle tree on the GPU") || !QueryTreeReady(q, "MultiHitTraverseBatchQueryDevice")) return false;
    const nrt_trace_options o = TraceOptions(q.options);
    const typename Api::MultiHitQueryPod d = MultiHitQueryDescriptor(q, &o);
    return Ok(Api::MultiHitQueryDevice(Context(), &d, hip_stream));
  }
  // ... and with device pointers, asynchronous on `hip_stream` (see TraverseBatchDevice).
  bool MultiHitTraverseBatchDevice(const Ray<T> *d_rays, size_t num_rays, unsigned int max_hits, TriangleIntersection<T> *d_isects,
                                   unsigned int *d_counts, void *hip_stream, const BVHTraceOptions &options = BVHTraceOptions()) const {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!TriangleTreeOnDevice("MultiHitTraverseBatchDevice: no triangle tree on the GPU (Build() with the built-in triangle types, or TraverseBatch() once after Load())")) return false;
    const nrt_trace_options o = TraceOptions(options);
    return Ok(Api::MultiHitDevice(Context(), Pod(d_rays), num_rays, max_hits, &o, Pod(d_isects), d_counts, hip_stream));
  }
  // Same for a tree built over the built-in sphere primitive (SphereGeometry + SpherePred).
  bool TraverseBatch(const Ray<T> *rays, size_t num_rays, SphereIntersection *isects, unsigned char *hit_out = NULL,
                     const BVHTraceOptions &options = BVHTraceOptions()) const {
    static_assert(detail::same_type<T, float>::value, "the sphere primitive is fp32");
    return TraverseBatchImpl(rays, num_rays, isects, hit_out, options);
  }
  // Same for a tree built over the built-in cylinder primitive (CylinderGeometry + CylinderPred); `test_cap` is the
  // CylinderIntersector constructor flag.
  bool TraverseBatch(const Ray<T> *rays, size_t num_rays, CylinderIntersection *isects, unsigned char *hit_out = NULL,
                     const BVHTraceOptions &options = BVHTraceOptions(), bool test_cap = true) const {
    static_assert(detail::same_type<T, float>::value, "the cylinder primitive is fp32");
    static_assert(sizeof(CylinderIntersection) == sizeof(nrt_cyl_hit_f32), "CylinderIntersection layout");
    std::lock_guard<std::mutex> lock(batch_mutex_);
    return CylinderTreeReady("TraverseBatch(CylinderIntersection*)", test_cap) &&
           StagedTrace<nrt_cyl_hit_f32>(rays, num_rays, isects, hit_out, options, nrtTraverseBatchCylinders_f32);
  }
  // Same for a tree built over the built-in curve primitive (BezierCurveGeometry + BezierCurvePred); `num_subdivisions` is the
  // BezierCurveIntersector constructor argument (1..64).
  bool TraverseBatch(const Ray<T> *rays, size_t num_rays, BezierCurveIntersection *isects, unsigned char *hit_out = NULL,
                     const BVHTraceOptions &options = BVHTraceOptions(), int num_subdivisions = 4) const {
    static_assert(detail::same_type<T, float>::value, "the curve primitive is fp32");
    static_assert(sizeof(BezierCurveIntersection) == sizeof(nrt_curve_hit_f32), "BezierCurveIntersection layout");
    std::lock_guard<std::mutex> lock(batch_mutex_);
    return CurveTreeReady("TraverseBatch(BezierCurveIntersection*)", num_subdivisions) &&
           StagedTrace<nrt_curve_hit_f32>(rays, num_rays, isects, hit_out, options, nrtTraverseBatchCurves_f32);
  }
  // Opt-in extension without a reference counterpart: occlusion queries of the sphere, cylinder and curve accels
  // (nrtOccludedBatchPrims_f32).  occluded_out[i] is 1 / 0: exactly the flag of the host OccludedBatch(rays, n, intersector, out)
  // above with the kind's intersector — of TraverseBatch(<Kind>Intersection*)'s hit_out[i] != 0 — but a ray stops at the first
  // primitive that settles it and no record is produced, staged or copied.  Refusals are those of the matching TraverseBatch().
  // (OccludedBatch() / OccludedBatchDevice() above stay the triangle accels' calls and refuse these kinds.)
  bool OccludedBatchSpheres(const Ray<T> *rays, size_t num_rays, unsigned char *occluded_out, const BVHTraceOptions &options = BVHTraceOptions()) const {
    static_assert(detail::same_type<T, float>::value, "the sphere primitive is fp32");
    std::lock_guard<std::mutex> lock(batch_mutex_);
    return DeviceTreeReady(1) && OccludedPrims(rays, num_rays, occluded_out, options, false, NULL);
  }
  bool OccludedBatchCylinders(const Ray<T> *rays, size_t num_rays, unsigned char *occluded_out, const BVHTraceOptions &options = BVHTraceOptions(),
                              bool test_cap = true) const {
    static_assert(detail::same_type<T, float>::value, "the cylinder primitive is fp32");
    std::lock_guard<std::mutex> lock(batch_mutex_);
    return CylinderTreeReady("OccludedBatchCylinders", test_cap) && OccludedPrims(rays, num_rays, occluded_out, options, false, NULL);
  }
  bool OccludedBatchCurves(const Ray<T> *rays, size_t num_rays, unsigned char *occluded_out, const BVHTraceOptions &options = BVHTraceOptions(),
                           int num_subdivisions = 4) const {
    static_assert(detail::same_type<T, float>::value, "the curve primitive is fp32");
    std::lock_guard<std::mutex> lock(batch_mutex_);
    return CurveTreeReady("OccludedBatchCurves", num_subdivisions) && OccludedPrims(rays, num_rays, occluded_out, options, false, NULL);
  }
  // ... and with device pointers, asynchronous on `hip_stream` (see TraverseBatchDevice).
  bool OccludedBatchSpheresDevice(const Ray<T> *d_rays, size_t num_rays, unsigned char *d_occluded, void *hip_stream,
                                  const BVHTraceOptions &options = BVHTraceOptions()) const {
    static_assert(detail::same_type<T, float>::value, "the sphere primitive is fp32");
    std::lock_guard<std::mutex> lock(batch_mutex_);
    return DeviceTreeReady(1) && OccludedPrims(d_rays, num_rays, d_occluded, options, true, hip_stream);
  }
  bool OccludedBatchCylindersDevice(const Ray<T> *d_rays, size_t num_rays, unsigned char *d_occluded, void *hip_stream,
                                    const BVHTraceOptions &options = BVHTraceOptions(), bool test_cap = true) const {
    static_assert(detail::same_type<T, float>::value, "the cylinder primitive is fp32");
    std::lock_guard<std::mutex> lock(batch_mutex_);
    return CylinderTreeReady("OccludedBatchCylindersDevice", test_cap) && OccludedPrims(d_rays, num_rays, d_occluded, options, true, hip_stream);
  }
  bool OccludedBatchCurvesDevice(const Ray<T> *d_rays, size_t num_rays, unsigned char *d_occluded, void *hip_stream,
                                 const BVHTraceOptions &options = BVHTraceOptions(), int num_subdivisions = 4) const {
    static_assert(detail::same_type<T, float>::value, "the curve primitive is fp32");
    std::lock_guard<std::mutex> lock(batch_mutex_);
    return CurveTreeReady("OccludedBatchCurvesDevice", num_subdivisions) && OccludedPrims(d_rays, num_rays, d_occluded, options, true, hip_stream);
  }
  const std::string &LastBackendError() const { return backend_error_; }
  // The C-ABI context behind this accel (NULL before a GPU Build()): what nrtSceneAddNode_f32 takes (include/nanosg_hip.h).
  nrt_ctx *HipContext() const { return dev_.tree_stale ? NULL : dev_.ctx.get(); }
  // Multi-GPU (environment variable NANORT_HIP_DEVICES = "all" or a list such as "0,1,2,3"; read by Build()): Build() makes a
  // replica of the tree on every listed device (the build is deterministic: the replicas are bit-identical) and
  // TraverseBatch() splits a host batch over them in interleaved rows of this many rays (default 4096; a renderer passes its
  // image width).  Records are the single-device ones.
  size_t NumHipDevices() const { return dev_.ctx ? 1 + dev_.peers.size() : 0; }
  void SetTraverseBatchRowLength(size_t rays_per_row) { dev_.batch_row_len = rays_per_row; }

 private:
  typedef detail::HipApi<T> Api;
  typedef typename Api::RayPod RayPod;
  typedef typename Api::HitPod HitPod;
  static const RayPod *Pod(const Ray<T> *r) { return reinterpret_cast<const RayPod *>(r); }
  static HitPod *Pod(TriangleIntersection<T> *h) { return reinterpret_cast<HitPod *>(h); }
  // Context 0 is the primary, 1 .. NumHipDevices() - 1 the replicas on the other devices of NANORT_HIP_DEVICES.
  nrt_ctx *Context(size_t k = 0) const { return k == 0 ? dev_.ctx.get() : dev_.peers[k - 1].get(); }
  // The call path of every C-ABI call: its status becomes the method's result, with the reason of the context it came from
  // (default: the primary) in LastBackendError(); the options cross as the C struct of the same layout.
  bool Ok(nrt_status st, nrt_ctx *c) const {
    if (st == NRT_OK) return true;
    backend_error_ = nrtLastError(c);
    return false;
  }
  bool Ok(nrt_status st) const { return Ok(st, Context()); }
  static nrt_trace_options TraceOptions(const BVHTraceOptions &options) {
    static_assert(sizeof(BVHTraceOptions) == sizeof(nrt_trace_options), "BVHTraceOptions layout");
    nrt_trace_options o;
    std::memcpy(&o, &options, sizeof(o));
    return o;
  }
  // The check of the Device forms and of OccludedBatch (caller holds batch_mutex_), which upload nothing: a triangle tree that is
  // on the GPU now, or `refusal`.
  bool TriangleTreeOnDevice(const char *refusal) const {
    if (dev_.ctx && !dev_.tree_stale && geom_.kind == 0) return true;
    backend_error_ = refusal;
    return false;
  }
  // Refit() of the kinds it does not refit on the GPU (1 spheres, 2 cylinders, 3 curves).
  bool NoGpuRefit(int kind) {
    backend_error_ = kind == 1 ? "Refit: sphere trees do not refit on the GPU (Build() again)"
                               : (kind == 2 ? "Refit: cylinder trees do not refit on the GPU (Build() again)"
                                            : "Refit: curve trees do not refit on the GPU (Build() again)");
    return false;
  }
  // What a GPU refit does around the call that is its own (caller holds batch_mutex_; `kind` is the object's geom_.kind):
  // an object that shares its contexts with copies first moves to contexts of its own, a Load()ed tree is uploaded, then
  // `refit_ctx` runs on the primary and on every replica.
  template <class RefitCtx>
  bool RefitContexts(int kind, RefitCtx refit_ctx) {
    if (SharesDeviceContext()) {  // copy-on-write: the copies keep the shared contexts, their tree and their positions
      EnsureHostTree();
      if (nodes_.empty()) {
        backend_error_ = "Refit: empty tree";
        return false;
      }
      if (!DetachDeviceContext(geom_.cyl_test_cap)) return false;
    }
    if (!DeviceTreeReady(kind)) return false;  // (a Load()ed tree is uploaded first)
    // The primary first: its refusal leaves everything as it was (a device error drops its tree: Build() again).  The
    // replicas pass the same checks, so only a device error can stop one: the object then traces on the primary alone, as
    // after a replica's failed build, and never on a replica that still holds the old boxes.
    if (!Ok(refit_ctx(Context()))) return false;
    for (size_t k = 1; k < NumHipDevices(); k++) {
      if (!Ok(refit_ctx(Context(k)), Context(k))) {
        fprintf(stderr, "[nanort] HIP refit of replica %zu failed (%s): tracing on one device\n", k, backend_error_.c_str());
        dev_.peers.clear();
        dev_.devices.resize(1);
        break;
      }
    }
    return true;
  }
  // ... and behind it: the root's box, and the host copy of the tree is read back on the next host access.
  bool RefitDone() {
    uint64_t nn = 0, ni = 0;
    if (!Ok(nrtTreeSize(Context(), &nn, &ni)) || !Ok(Api::TreeBounds(Context(), dev_.root_bmin, dev_.root_bmax))) return false;
    dev_.pending_nodes = nn;
    dev_.pending_indices = ni;
    __atomic_store_n(&host_tree_pending_, true, __ATOMIC_RELEASE);  // GetNodes(), Traverse(), Dump() and copies read the refit boxes
    return true;
  }
  // RefitGeometry: the object was built on the GPU over `kind` (1 spheres, 3 curves) and, when a count is given, over that many;
  // then the refit of every context, and the new arrays are the ones a later detach sends.
  bool RefitPrims(const char *who, int kind, const float *positions, const float *radii, unsigned int num_primitives) {
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!dev_.ctx || geom_.kind != kind) {
      backend_error_ = std::string(who) + (kind == 1 ? ": this accel was not built on the GPU over a SphereGeometry" : ": this accel was not built on the GPU over a BezierCurveGeometry");
      return false;
    }
    if (num_primitives != ~0u && num_primitives != geom_.count) {
      backend_error_ = std::string(who) + ": the tree was built over another number of primitives";
      return false;
    }
    if (!RefitContexts(kind, [&](nrt_ctx *c) { return nrtRefitPrims_f32(c, positions, radii, geom_.count); })) return false;
    geom_.positions = positions;
    geom_.radii = radii;
    return RefitDone();
  }
  // The checks of the motion queries (caller holds batch_mutex_): a triangle accel built over a MotionTriangleMesh.
  bool MotionTreeReady(const char *who) const {
    if (!dev_.ctx || geom_.kind != 0 || !geom_.vertices1) {
      backend_error_ = std::string(who) + ": Build() with MotionTriangleMesh/MotionTriangleSAHPred first";
      return false;
    }
    return DeviceTreeReady(0);
  }
  // The checks of the masked queries (caller holds batch_mutex_): a triangle accel that holds masks.
  bool MaskedTreeReady(const char *who) const {
    if (!dev_.ctx || geom_.kind != 0 || !geom_.masks) {
      backend_error_ = std::string(who) + ": SetPrimMasks() on an accel built over a TriangleMesh first";
      return false;
    }
    return DeviceTreeReady(0);
  }
  // The checks of the combined query (caller holds batch_mutex_): those of every feature it has, or of a plain triangle batch.
  template <class Q>
  bool QueryTreeReady(const Q &q, const char *who) const {
    if (q.motion && !MotionTreeReady(who)) return false;
    if (q.masked && !MaskedTreeReady(who)) return false;
    return DeviceTreeReady(0);
  }
  // ... and its descriptor for the C ABI (`o`: the caller's converted options, which outlive the call).
  typename Api::QueryPod QueryDescriptor(const BatchQuery<T> &q, const nrt_trace_options *o) const {
    typename Api::QueryPod d;
    d.struct_size = static_cast<uint32_t>(sizeof(d));
    d.flags = (q.occlusion ? NRT_QUERY_OCCLUSION : 0u) | (q.motion ? NRT_QUERY_MOTION : 0u) | (q.masked ? NRT_QUERY_MASKED : 0u);
    d.rays = Pod(q.rays);
    d.num_rays = q.num_rays;
    d.options = o;
    d.skip_prim_ids = q.skip_prim_ids;
    d.times = q.times;
    d.ray_masks = q.ray_masks;
    d.hits_out = Pod(q.isects);
    d.mask_out = q.hit_out;
    return d;
  }
  typename Api::MultiHitQueryPod MultiHitQueryDescriptor(const MultiHitBatchQuery<T> &q, const nrt_trace_options *o) const {
    typename Api::MultiHitQueryPod d;
    d.struct_size = static_cast<uint32_t>(sizeof(d));
    d.flags = (q.motion ? NRT_QUERY_MOTION : 0u) | (q.masked ? NRT_QUERY_MASKED : 0u);
    d.rays = Pod(q.rays);
    d.num_rays = q.num_rays;
    d.options = o;
    d.skip_prim_ids = q.skip_prim_ids;
    d.times = q.times;
    d.ray_masks = q.ray_masks;
    d.hits_out = Pod(q.isects);
    d.counts_out = q.counts_out;
    d.max_hits = q.max_hits;
    d.reserved = 0;
    return d;
  }
  // The GPU side of ClosestPointBatch() and SignedDistanceBatch(): the points packed into the library's 4-scalar records, one host
  // call of the library (`entry`: Api::ClosestPoint or Api::SignedDistance, whose records share one layout).
  template <class Entry, class Pod, class Result>
  bool PointBatchBackend(Entry entry, const T *points, const T *max_dists, size_t num_points, Result *out, unsigned char *found_out,
                         const BVHTraceOptions &options) const {
    static_assert(sizeof(Result) == sizeof(Pod), "point query record layout");
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!DeviceTreeReady(0)) return false;
    if (num_points == 0) return true;
    const std::vector<typename Api::PointPod> pts = PackPoints(points, max_dists, num_points);
    const nrt_trace_options o = TraceOptions(options);
    return Ok(entry(Context(), &pts[0], num_points, &o, reinterpret_cast<Pod *>(out), found_out));
  }
  std::vector<typename Api::PointPod> PackPoints(const T *points, const T *max_dists, size_t num_points) const {
    std::vector<typename Api::PointPod> pts(num_points);
    for (size_t i = 0; i < num_points; i++) {
      for (int k = 0; k < 3; k++) pts[i].p[k] = points[3 * i + k];
      pts[i].max_dist = max_dists ? max_dists[i] : std::numeric_limits<T>::infinity();
    }
    return pts;
  }
  // ... and of NearestFacesBatch(): max_faces records and one count per point.
  bool NearestFacesBatchBackend(const T *points, const T *max_dists, size_t num_points, unsigned int max_faces, ClosestPointResult<T> *out,
                                unsigned int *counts_out, const BVHTraceOptions &options) const {
    static_assert(sizeof(ClosestPointResult<T>) == sizeof(typename Api::ClosestPod) && sizeof(unsigned int) == sizeof(uint32_t), "point query record layout");
    std::lock_guard<std::mutex> lock(batch_mutex_);
    if (!DeviceTreeReady(0)) return false;
    const std::vector<typename Api::PointPod> pts = PackPoints(points, max_dists, num_points);
    const nrt_trace_options o = TraceOptions(options);
    return Ok(Api::NearestFaces(Context(), num_points ? &pts[0] : NULL, num_points, max_faces, &o, reinterpret_cast<typename Api::ClosestPod *>(out),
                                counts_out));
  }
  bool ClosestPointBatchBackend(const T *points, const T *max_dists, size_t num_points, ClosestPointResult<T> *out, unsigned char *found_out,
                                const BVHTraceOptions &options) const {
    return PointBatchBackend<decltype(Api::ClosestPoint), typename Api::ClosestPod>(Api::ClosestPoint, points, max_dists, num_points, out, found_out, options);
  }
  bool SignedDistanceBatchBackend(const T *points, const T *max_dists, size_t num_points, SignedDistanceResult<T> *out, unsigned char *found_out,
                                  const BVHTraceOptions &options) const {
    return PointBatchBackend<decltype(Api::SignedDistance), typename Api::SignedPod>(Api::SignedDistance, points, max_dists, num_points, out, found_out, options);
  }
  // The checks every host batch call makes (caller holds batch_mutex_): a context, the primitive kind the call's records are
  // for (0 triangles, 1 spheres), and a tree adopted by Load() uploaded — after a copy-on-write detach when the contexts are
  // shared with copies.
  bool DeviceTreeReady(int want_kind) const {
    if (!dev_.ctx) {
      backend_error_ = "TraverseBatch: no GPU context (Build() with TriangleMesh/TriangleSAHPred first)";
      return false;
    }
    if (geom_.kind != want_kind) {  // records of one primitive kind must not be read as another's
      backend_error_ = want_kind == 0 ? "TraverseBatch(TriangleIntersection*): this accel was not built over a TriangleMesh"
                                      : "TraverseBatch(SphereIntersection*): this accel was not built over a SphereGeometry";
      return false;
    }
    if (dev_.tree_stale) {
      EnsureHostTree();  // (Load() already dropped any pending read-back: a no-op, kept so the upload never sees a half state)
      if (nodes_.empty()) {
        backend_error_ = "TraverseBatch: empty tree";
        return false;
      }
      if (SharesDeviceContext() && !DetachDeviceContext(geom_.cyl_test_cap)) return false;  // copy-on-write
      for (size_t k = 0; k < NumHipDevices(); k++)  // (the replicas on the other devices adopt the same arrays)
        if (!Ok(Api::SetTree(Context(k), reinterpret_cast<const typename Api::NodePod *>(&nodes_[0]), nodes_.size(),
                             indices_.empty() ? NULL : &indices_[0], indices_.size()),
                Context(k)))
          return false;
      dev_.tree_stale = false;
    }
    return true;
  }
  // The same for the cylinder (kind 2) and the curve (kind 3) accels (caller holds batch_mutex_; `who` opens the error text).  The
  // intersector's constructor argument — test_cap, num_subdivisions; the other kind's is passed as it stands — lives with the
  // primitives on the device: when it differs from what was sent last, or the tree was adopted by Load(), the primitives go again
  // with the new value and the tree behind them.
  bool ResentTreeReady(const char *who, int kind, bool test_cap, int num_subdivisions) const {
    if (!dev_.ctx || !geom_.positions || geom_.kind != kind) {
      backend_error_ = std::string(who) + (kind == 2 ? ": Build() with CylinderGeometry/CylinderPred first" : ": Build() with BezierCurveGeometry/BezierCurvePred first");
      return false;
    }
    if (kind == 3 && (num_subdivisions < 1 || num_subdivisions > 64)) {
      backend_error_ = std::string(who) + ": num_subdivisions outside 1..64";
      return false;
    }
    if (test_cap == geom_.cyl_test_cap && num_subdivisions == geom_.crv_subdiv && !dev_.tree_stale) return true;
    // (the host tree first: it may still be pending after Build(), and sending the primitives frees the device tree)
    EnsureHostTree();
    if (nodes_.empty()) {
      backend_error_ = std::string(who) + ": empty tree";
      return false;
    }
    // The subdivision count is stored before the send, which reads it from the record; the cap goes into the send and is stored
    // only once the tree is up again.  A failed re-send therefore leaves what it always left: the new count, the old cap.
    geom_.crv_subdiv = num_subdivisions;
    if (SharesDeviceContext() ? !DetachDeviceContext(test_cap)  // copy-on-write: the shared context stays with the copies
                              : !Ok(SendPrimitives(Context(), test_cap)))
      return false;
    if (!Ok(nrtSetTree_f32(Context(), reinterpret_cast<const nrt_node_f32 *>(&nodes_[0]), nodes_.size(), &indices_[0], indices_.size()))) return false;
    geom_.cyl_test_cap = test_cap;
    dev_.tree_stale = false;
    return true;
  }
  bool CylinderTreeReady(const char *who, bool test_cap) const { return ResentTreeReady(who, 2, test_cap, geom_.crv_subdiv); }
  bool CurveTreeReady(const char *who, int num_subdivisions) const { return ResentTreeReady(who, 3, geom_.cyl_test_cap, num_subdivisions); }
  // The trace of the two kinds whose records are their own (caller holds batch_mutex_, the kind's tree is ready): staged, then
  // isects[i] is written only on a hit, like Traverse().
  template <class HitPodK, class Hit, class Trace>
  bool StagedTrace(const Ray<T> *rays, size_t num_rays, Hit *isects, unsigned char *hit_out, const BVHTraceOptions &options, Trace trace) const {
    if (num_rays == 0) return true;
    std::vector<Hit> tmp(num_rays);
    std::vector<unsigned char> mask(num_rays);
    const nrt_trace_options o = TraceOptions(options);
    if (!Ok(trace(Context(), reinterpret_cast<const nrt_ray_f32 *>(rays), num_rays, &o, reinterpret_cast<HitPodK *>(&tmp[0]), &mask[0]))) return false;
    for (size_t i = 0; i < num_rays; i++) {
      if (mask[i]) isects[i] = tmp[i];
      if (hit_out) hit_out[i] = mask[i];
    }
    return true;
  }
  // The launch of OccludedBatch<Kind>[Device] once the kind's tree is ready (caller holds batch_mutex_).
  bool OccludedPrims(const Ray<T> *rays, size_t num_rays, unsigned char *occluded, const BVHTraceOptions &options, bool device, void *hip_stream) const {
    const nrt_trace_options o = TraceOptions(options);
    const nrt_ray_f32 *r = reinterpret_cast<const nrt_ray_f32 *>(rays);
    return Ok(device ? nrtOccludedBatchPrimsDevice_f32(Context(), r, num_rays, &o, occluded, hip_stream)
                     : nrtOccludedBatchPrims_f32(Context(), r, num_rays, &o, occluded));
  }
  template <class Hit>
  bool TraverseBatchImpl(const Ray<T> *rays, size_t num_rays, Hit *isects, unsigned char *hit_out, const BVHTraceOptions &options,
                         const unsigned int *skip_prim_ids = NULL) const {
    static_assert(sizeof(Ray<T>) == sizeof(RayPod), "Ray layout");
    static_assert(sizeof(Hit) == sizeof(HitPod), "intersection record layout");
    const int want_kind = detail::same_type<Hit, TriangleIntersection<T> >::value ? 0 : 1;
    std::lock_guard<std::mutex> lock(batch_mutex_);  // (staging, launch and scatter: see the comment above TraverseBatch)
    if (!DeviceTreeReady(want_kind)) return false;
    if (num_rays == 0) return true;
    // Grow-only byte staging owned by the accel, page-locked when the backend can provide it (the device-to-host copy
    // then runs at PCIe speed; PODs: no per-element construction, no fresh pages to fault in on every wave); the caller's
    // mask array is used directly when there is one.
    HitPod *tmp = static_cast<HitPod *>(StageEnsure(&stage_hits_, &stage_hits_cap_, num_rays * sizeof(HitPod)));
    unsigned char *mask = hit_out ? hit_out : static_cast<unsigned char *>(StageEnsure(&stage_mask_, &stage_mask_cap_, num_rays));
    if (!tmp || !mask) {
      backend_error_ = "TraverseBatch: out of host memory for the staging buffers";
      return false;
    }
    const nrt_trace_options o = TraceOptions(options);
    nrt_status st;
    if (skip_prim_ids) {  // (one device: nrtTraverseBatchMulti takes no per-ray ids, and the records are the same)
      st = Api::TraverseSkip(Context(), Pod(rays), num_rays, &o, skip_prim_ids, tmp, mask);
    } else if (!dev_.peers.empty() && want_kind == 0) {
      // NANORT_HIP_DEVICES: the batch is split row-interleaved over the replicas, one per device (nrtTraverseBatchMulti)
      std::vector<nrt_ctx *> cs;
      for (size_t k = 0; k < NumHipDevices(); k++) cs.push_back(Context(k));
      st = Api::TraverseMulti(&cs[0], static_cast<uint32_t>(cs.size()), Pod(rays), num_rays, dev_.batch_row_len, &o, tmp, mask);
    } else {
      st = Api::Traverse(Context(), Pod(rays), num_rays, &o, tmp, mask);
    }
    if (!Ok(st)) return false;
    // isects[i] is written only on a hit, like Traverse().  (At most half of what the process may use, detail::HostThreads():
    // an OpenMP default of "all hardware threads" inside a CPU-quota'd container starves the HIP runtime's own threads —
    // measured 10x slower.)
#ifdef _OPENMP
    const int scatter_threads = static_cast<int>(std::min(8u, std::max(1u, detail::HostThreads() / 2)));
#pragma omp parallel for schedule(static) num_threads(scatter_threads) if (num_rays > (1u << 18))
#endif
    for (long long i = 0; i < static_cast<long long>(num_rays); i++)
      if (mask[i]) std::memcpy(static_cast<void *>(&isects[i]), &tmp[i], sizeof(HitPod));
    return true;
  }

 public:
#endif

  const std::vector<BVHNode<T> > &GetNodes() const {
    EnsureHostTree();
    return nodes_;
  }
  const std::vector<unsigned int> &GetIndices() const {
    EnsureHostTree();
    return indices_;
  }

  void BoundingBox(T bmin[3], T bmax[3]) const {
#ifdef NANORT_USE_HIP_BACKEND
    if (HostTreePending()) {  // (the root's box came back with the build: no need for the whole array)
      for (int k = 0; k < 3; k++) {
        bmin[k] = dev_.root_bmin[k];
        bmax[k] = dev_.root_bmax[k];
      }
      return;
    }
#endif
    for (int k = 0; k < 3; k++) {
      bmin[k] = nodes_.empty() ? std::numeric_limits<T>::max() : nodes_[0].bmin[k];
      bmax[k] = nodes_.empty() ? -std::numeric_limits<T>::max() : nodes_[0].bmax[k];
    }
  }

  bool IsValid() const { return HostTreePending() || nodes_.size() > 0; }

#ifdef NANORT_USE_HIP_BACKEND
  // The host copy of a GPU-built tree, on demand (thread-safe: Traverse() is const and may be called from many threads).
  void EnsureHostTree() const {
    if (!__atomic_load_n(&host_tree_pending_, __ATOMIC_ACQUIRE)) return;
    std::lock_guard<std::mutex> lock(detail::HostTreeMutex());
    if (!host_tree_pending_) return;
    nodes_.resize(static_cast<size_t>(dev_.pending_nodes));
    indices_.resize(static_cast<size_t>(dev_.pending_indices));
    if (!dev_.ctx || Api::GetTree(Context(), reinterpret_cast<typename Api::NodePod *>(&nodes_[0]), indices_.empty() ? NULL : &indices_[0]) != NRT_OK) {
      backend_error_ = dev_.ctx ? nrtLastError(Context()) : "host tree requested without a GPU context";
      fprintf(stderr, "[nanort] reading the tree back from the GPU failed: %s\n", backend_error_.c_str());
      nodes_.clear();
      indices_.clear();
    }
    __atomic_store_n(&host_tree_pending_, false, __ATOMIC_RELEASE);
  }
  bool HostTreePending() const { return __atomic_load_n(&host_tree_pending_, __ATOMIC_ACQUIRE); }
  // Set NANORT_HIP_EAGER_READBACK=1 (environment) to make Build() fetch the arrays itself, as rounds 1-5 did.
#else
  void EnsureHostTree() const {}
  bool HostTreePending() const { return false; }
#endif

 private:
  // Host refit over nodes_ / indices_.  The walk from the root is validated first (children and leaf slots in range, no record
  // reached twice) and yields the reachable records in post-order; only then are boxes written, so a malformed Load()ed tree
  // is refused with nodes_ unchanged.
  template <class Prim>
  bool RefitHost(const Prim &prim) {
    EnsureHostTree();
    const size_t nn = nodes_.size();
    if (nn == 0) return false;
    std::vector<unsigned int> order;  // reachable records, children before their parent
    std::vector<unsigned char> seen(nn, 0);
    std::vector<std::pair<unsigned int, bool> > st(1, std::make_pair(0u, false));
    while (!st.empty()) {
      const std::pair<unsigned int, bool> e = st.back();
      st.pop_back();
      const BVHNode<T> &n = nodes_[e.first];
      if (e.second) {
        order.push_back(e.first);
        continue;
      }
      if (seen[e.first]) return false;
      seen[e.first] = 1;
      if (n.flag == 0) {
        if (n.data[0] >= nn || n.data[1] >= nn) return false;
        st.push_back(std::make_pair(e.first, true));
        st.push_back(std::make_pair(n.data[1], false));
        st.push_back(std::make_pair(n.data[0], false));
      } else {
        if (static_cast<size_t>(n.data[1]) + n.data[0] > indices_.size()) return false;
        order.push_back(e.first);
      }
    }
    for (size_t i = 0; i < order.size(); i++) {
      BVHNode<T> &n = nodes_[order[i]];
      if (n.flag == 0) {
        const BVHNode<T> &a = nodes_[n.data[0]], &b = nodes_[n.data[1]];
        for (int k = 0; k < 3; k++) {
          n.bmin[k] = std::min(a.bmin[k], b.bmin[k]);
          n.bmax[k] = std::max(a.bmax[k], b.bmax[k]);
        }
      } else {
        BBox<T> acc;
        for (unsigned int j = 0; j < n.data[0]; j++) {
          real3<T> lo, hi;
          prim.BoundingBox(&lo, &hi, indices_[n.data[1] + j]);
          for (int k = 0; k < 3; k++) {
            acc.bmin[k] = std::min(acc.bmin[k], lo[k]);
            acc.bmax[k] = std::max(acc.bmax[k], hi[k]);
          }
        }
        for (int k = 0; k < 3; k++) {
          n.bmin[k] = acc.bmin[k];
          n.bmax[k] = acc.bmax[k];
        }
      }
    }
    return true;
  }

  // ---- generic host builder: binned SAH over all three axes, iterative, pre-order ----
  struct Pending {
    unsigned int lo, hi, depth, parent;
    bool is_high_child;
  };
  struct HostBin {
    BBox<T> box;
    size_t count;
    HostBin() : count(0) {}
  };

  static T HalfArea(const real3<T> &mn, const real3<T> &mx) {
    const real3<T> e = mx - mn;
    return e[0] * e[1] + e[1] * e[2] + e[2] * e[0];
  }

  // Bounding box of the primitives in indices_[lo, hi) (`threads` > 1: in chunks; min / max do not depend on the order).
  template <class Prim>
  void RangeBounds(const Prim &prim, unsigned int lo, unsigned int hi, unsigned int threads, real3<T> *out_min, real3<T> *out_max) const {
    const unsigned int count = hi - lo;
    const unsigned int chunks = (threads > 1 && count >= 16384u) ? threads * 4u : 1u;
    std::vector<BBox<T> > part(chunks);
    const unsigned int *idx = &indices_[0];
    detail::ParallelFor(chunks, threads, [&](unsigned int c) {
      const unsigned int b = lo + static_cast<unsigned int>((static_cast<unsigned long long>(count) * c) / chunks);
      const unsigned int e = lo + static_cast<unsigned int>((static_cast<unsigned long long>(count) * (c + 1)) / chunks);
      BBox<T> acc;
      for (unsigned int i = b; i < e; i++) {
        real3<T> a, bb;
        prim.BoundingBox(&a, &bb, idx[i]);
        for (int k = 0; k < 3; k++) {
          acc.bmin[k] = std::min(acc.bmin[k], a[k]);
          acc.bmax[k] = std::max(acc.bmax[k], bb[k]);
        }
      }
      part[c] = acc;
    });
    BBox<T> all = part[0];
    for (unsigned int c = 1; c < chunks; c++)
      for (int k = 0; k < 3; k++) {
        all.bmin[k] = std::min(all.bmin[k], part[c].bmin[k]);
        all.bmax[k] = std::max(all.bmax[k], part[c].bmax[k]);
      }
    *out_min = all.bmin;
    *out_max = all.bmax;
  }

  // One node of the generic host builder over indices_[lo, hi): its box, the leaf decision, or the binned-SAH split over
  // x, y and z followed by the partition of the range (pred is this thread's own copy: Set() mutates it).
  // Returns true for a leaf; else *mid and *axis describe the split.
  template <class Prim, class Pred>
  bool SplitRange(const Prim &prim, Pred &pred, unsigned int lo, unsigned int hi, unsigned int depth, unsigned int threads,
                  std::vector<HostBin> &bins, std::vector<BBox<T> > &sweep, BVHNode<T> *node, unsigned int *mid_out, int *axis_out) {
    const unsigned int K = options_.bin_size;
    real3<T> nmin, nmax;
    RangeBounds(prim, lo, hi, threads, &nmin, &nmax);
    for (int k = 0; k < 3; k++) {
      node->bmin[k] = nmin[k];
      node->bmax[k] = nmax[k];
    }
    const unsigned int count = hi - lo;
    if (count <= options_.min_leaf_primitives || depth >= options_.max_tree_depth || count < 2) {
      node->flag = 1;
      node->axis = 0;
      node->data[0] = count;
      node->data[1] = lo;
      return true;
    }
    // bin the centres over the node's box on x, y and z (`threads` > 1: per-chunk bins merged in chunk order — counts
    // add and boxes min / max, so the merged bins are the serial ones)
    real3<T> scale;
    for (int k = 0; k < 3; k++) {
      const T ext = nmax[k] - nmin[k];
      scale[k] = ext > static_cast<T>(0.0) ? static_cast<T>(K) / ext : static_cast<T>(0.0);
    }
    const unsigned int chunks = (threads > 1 && count >= 16384u) ? threads * 4u : 1u;
    std::vector<HostBin> chunk_bins;
    if (chunks > 1) chunk_bins.assign(static_cast<size_t>(chunks) * 3 * K, HostBin());
    std::fill(bins.begin(), bins.end(), HostBin());
    const unsigned int *idx = &indices_[0];
    detail::ParallelFor(chunks, threads, [&](unsigned int c) {
      HostBin *dst = chunks > 1 ? &chunk_bins[static_cast<size_t>(c) * 3 * K] : &bins[0];
      const unsigned int b = lo + static_cast<unsigned int>((static_cast<unsigned long long>(count) * c) / chunks);
      const unsigned int e = lo + static_cast<unsigned int>((static_cast<unsigned long long>(count) * (c + 1)) / chunks);
      for (unsigned int i = b; i < e; i++) {
        real3<T> a, bb, cc;
        prim.BoundingBoxAndCenter(&a, &bb, &cc, idx[i]);
        for (int k = 0; k < 3; k++) {
          const long q = static_cast<long>((cc[k] - nmin[k]) * scale[k]);
          const unsigned int slot = static_cast<unsigned int>(std::min<long>(static_cast<long>(K) - 1, std::max<long>(0, q)));
          HostBin &hb = dst[static_cast<size_t>(k) * K + slot];
          hb.count++;
          for (int d = 0; d < 3; d++) {
            hb.box.bmin[d] = std::min(hb.box.bmin[d], a[d]);
            hb.box.bmax[d] = std::max(hb.box.bmax[d], bb[d]);
          }
        }
      }
    });
    for (unsigned int c = 0; chunks > 1 && c < chunks; c++)
      for (size_t j = 0; j < static_cast<size_t>(3) * K; j++) {
        const HostBin &src = chunk_bins[static_cast<size_t>(c) * 3 * K + j];
        HostBin &hb = bins[j];
        hb.count += src.count;
        for (int d = 0; d < 3; d++) {
          hb.box.bmin[d] = std::min(hb.box.bmin[d], src.box.bmin[d]);
          hb.box.bmax[d] = std::max(hb.box.bmax[d], src.box.bmax[d]);
        }
      }
    // two sweeps per axis; candidate s splits bins [0,s) | [s,K)
    T axis_cost[3], axis_cut[3];
    for (int k = 0; k < 3; k++) {
      axis_cost[k] = std::numeric_limits<T>::infinity();
      axis_cut[k] = nmin[k] + (nmax[k] - nmin[k]) * static_cast<T>(0.5);
      BBox<T> acc;
      for (unsigned int s2 = K; s2-- > 1;) {  // suffix boxes
        const HostBin &hb = bins[static_cast<size_t>(k) * K + s2];
        for (int d = 0; d < 3; d++) {
          acc.bmin[d] = std::min(acc.bmin[d], hb.box.bmin[d]);
          acc.bmax[d] = std::max(acc.bmax[d], hb.box.bmax[d]);
        }
        sweep[s2] = acc;
      }
      size_t left_n = 0;
      BBox<T> left;
      for (unsigned int s2 = 1; s2 < K; s2++) {
        const HostBin &hb = bins[static_cast<size_t>(k) * K + s2 - 1];
        left_n += hb.count;
        for (int d = 0; d < 3; d++) {
          left.bmin[d] = std::min(left.bmin[d], hb.box.bmin[d]);
          left.bmax[d] = std::max(left.bmax[d], hb.box.bmax[d]);
        }
        const size_t right_n = count - left_n;
        if (left_n == 0 || right_n == 0) continue;
        const T c = static_cast<T>(left_n) * HalfArea(left.bmin, left.bmax) + static_cast<T>(right_n) * HalfArea(sweep[s2].bmin, sweep[s2].bmax);
        if (c < axis_cost[k]) {
          axis_cost[k] = c;
          axis_cut[k] = nmin[k] + (nmax[k] - nmin[k]) * (static_cast<T>(s2) / static_cast<T>(K));
        }
      }
    }
    int order[3] = {0, 1, 2};
    if (axis_cost[order[1]] < axis_cost[order[0]]) std::swap(order[0], order[1]);
    if (axis_cost[order[2]] < axis_cost[order[1]]) std::swap(order[1], order[2]);
    if (axis_cost[order[1]] < axis_cost[order[0]]) std::swap(order[0], order[1]);

    unsigned int mid = lo;
    int axis = order[0];
    for (int attempt = 0; attempt < 3; attempt++) {
      axis = order[attempt];
      pred.Set(axis, axis_cut[axis]);
      unsigned int *first = &indices_[lo];
      unsigned int *split = std::partition(first, first + count, pred);
      mid = lo + static_cast<unsigned int>(split - first);
      if (mid != lo && mid != hi) break;
      mid = lo + (count >> 1);  // object median when the predicate cannot separate them
    }
    node->flag = 0;
    node->axis = axis;
    node->data[0] = 0;
    node->data[1] = 0;
    *mid_out = mid;
    *axis_out = axis;
    return false;
  }

  // A subtree to be built by a worker: its range, depth, and the stub that stands for it among the top nodes.
  struct SubtreeTask {
    unsigned int lo, hi, depth, stub;
    std::vector<BVHNode<T> > nodes;  // local pre-order, child indices relative to nodes[0]
    unsigned int max_depth, leaves, branches;
  };

  // Pre-order build of indices_[lo, hi) into `out` (child indices local to `out`).  With `tasks`: ranges that reach
  // `stop_depth` with at least `stop_count` primitives are not descended into — a stub (flag 2) is emitted and the range
  // recorded instead.
  template <class Prim, class Pred>
  void BuildRange(const Prim &prim, Pred &pred, unsigned int lo0, unsigned int hi0, unsigned int depth0, unsigned int threads,
                  std::vector<BVHNode<T> > &out, unsigned int *max_depth, unsigned int *leaves, unsigned int *branches,
                  std::vector<SubtreeTask> *tasks, unsigned int stop_depth, unsigned int stop_count) {
    const unsigned int K = options_.bin_size;
    std::vector<HostBin> bins(3 * static_cast<size_t>(K));
    std::vector<BBox<T> > sweep(K);
    std::vector<Pending> todo;
    Pending root = {lo0, hi0, depth0, 0, false};
    todo.push_back(root);
    while (!todo.empty()) {
      const Pending cur = todo.back();
      todo.pop_back();
      const unsigned int me = static_cast<unsigned int>(out.size());
      if (me != 0 && cur.is_high_child) out[cur.parent].data[1] = me;
      if (tasks && cur.depth >= stop_depth && cur.hi - cur.lo >= stop_count && me != 0) {
        BVHNode<T> stub;
        stub.flag = 2;
        stub.axis = 0;
        stub.data[0] = static_cast<unsigned int>(tasks->size());
        stub.data[1] = 0;
        out.push_back(stub);
        SubtreeTask t;
        t.lo = cur.lo;
        t.hi = cur.hi;
        t.depth = cur.depth;
        t.stub = me;
        t.max_depth = t.leaves = t.branches = 0;
        tasks->push_back(t);
        continue;
      }
      *max_depth = std::max(*max_depth, cur.depth);
      BVHNode<T> node;
      unsigned int mid = 0;
      int axis = 0;
      if (SplitRange(prim, pred, cur.lo, cur.hi, cur.depth, threads, bins, sweep, &node, &mid, &axis)) {
        out.push_back(node);
        (*leaves)++;
        continue;
      }
      node.data[0] = me + 1;
      out.push_back(node);
      (*branches)++;
      Pending high = {mid, cur.hi, cur.depth + 1, me, true};
      Pending low = {cur.lo, mid, cur.depth + 1, me, false};
      todo.push_back(high);
      todo.push_back(low);
    }
  }

  // BVHAccel::Build for user primitives (nanort.h:1892-2149): binned SAH over x, y and z, pre-order node array.
  // Parallel (NANORT_ENABLE_PARALLEL_BUILD with OpenMP, or NANORT_USE_CPP11_FEATURE; n >=
  // min_primitives_for_parallel_build) in the reference's shape — a shallow top tree, then one worker per subtree,
  // then the splice (nanort.h:2018-2117) — with the top levels' box and bin passes chunked over the workers as well.
  // The tree does not depend on the number of threads: it is the serial one, node for node.
  template <class Prim, class Pred>
  bool BuildImpl(unsigned int n, const Prim &prim, const Pred &pred, const BVHBuildOptions<T> &options, detail::generic_tag) {
    options_ = options;
    stats_ = BVHBuildStatistics();
#ifdef NANORT_USE_HIP_BACKEND
    DropPendingHostTree();
#endif
    nodes_.clear();
    indices_.clear();
    assert(options_.bin_size > 1);
    if (n == 0) return false;
    indices_.resize(n);
    for (unsigned int i = 0; i < n; i++) indices_[i] = i;

    unsigned int threads = 1;
#if defined(NANORT_ENABLE_PARALLEL_BUILD) && (defined(_OPENMP) || defined(NANORT_USE_CPP11_FEATURE))
    if (n >= options_.min_primitives_for_parallel_build) threads = detail::HostThreads();
#endif
    Pred top_pred = pred;
    if (threads <= 1) {
      BuildRange(prim, top_pred, 0, n, 0, 1, nodes_, &stats_.max_tree_depth, &stats_.num_leaf_nodes, &stats_.num_branch_nodes,
                 static_cast<std::vector<SubtreeTask> *>(0), 0, 0);
    } else {
      // deep enough for a few subtrees per worker (at least the reference's shallow_depth)
      unsigned int stop_depth = std::max(1u, options_.shallow_depth);
      while ((1u << stop_depth) < 4u * threads && stop_depth < 12u) stop_depth++;
      std::vector<BVHNode<T> > top;
      std::vector<SubtreeTask> tasks;
      BuildRange(prim, top_pred, 0, n, 0, threads, top, &stats_.max_tree_depth, &stats_.num_leaf_nodes, &stats_.num_branch_nodes, &tasks,
                 stop_depth, 1024u);
      detail::ParallelFor(static_cast<unsigned int>(tasks.size()), threads, [&](unsigned int k) {
        SubtreeTask &t = tasks[k];
        Pred local_pred = pred;
        BuildRange(prim, local_pred, t.lo, t.hi, t.depth, 1, t.nodes, &t.max_depth, &t.leaves, &t.branches,
                   static_cast<std::vector<SubtreeTask> *>(0), 0, 0);
      });
      // splice: where each top node and each subtree lands in the final pre-order array
      std::vector<unsigned int> final_of(top.size());
      unsigned int at = 0;
      for (size_t i = 0; i < top.size(); i++) {
        final_of[i] = at;
        at += top[i].flag == 2 ? static_cast<unsigned int>(tasks[top[i].data[0]].nodes.size()) : 1u;
      }
      nodes_.resize(at);
      for (size_t i = 0; i < top.size(); i++) {
        if (top[i].flag == 2) {
          const SubtreeTask &t = tasks[top[i].data[0]];
          const unsigned int base = final_of[i];
          for (size_t j = 0; j < t.nodes.size(); j++) {
            BVHNode<T> nd = t.nodes[j];
            if (nd.flag == 0) {
              nd.data[0] += base;
              nd.data[1] += base;
            }
            nodes_[base + j] = nd;
          }
          stats_.max_tree_depth = std::max(stats_.max_tree_depth, t.max_depth);
          stats_.num_leaf_nodes += t.leaves;
          stats_.num_branch_nodes += t.branches;
        } else {
          BVHNode<T> nd = top[i];
          if (nd.flag == 0) {
            nd.data[0] = final_of[nd.data[0]];
            nd.data[1] = final_of[nd.data[1]];
          }
          nodes_[final_of[i]] = nd;
        }
      }
    }
#ifdef NANORT_USE_HIP_BACKEND
    // user primitives live on the host only: a device context left over from an earlier built-in Build() holds other
    // primitives and must not be traced against this tree
    dev_.ctx.reset();
    dev_.peers.clear();
    dev_.devices.clear();
    dev_.tree_stale = false;
    geom_.kind = -1;
#endif
    return true;
  }

#ifdef NANORT_USE_HIP_BACKEND
  // What the device holds, in two records: a copy copies them, a move takes them and leaves default-constructed ones behind, so
  // a new piece of per-context state is ONE field here and nothing in CopyFrom() / MoveFrom().
  // The contexts and what goes with them:
  struct DeviceState {
    std::shared_ptr<nrt_ctx> ctx;
    std::vector<std::shared_ptr<nrt_ctx> > peers;  // replicas on the other devices of NANORT_HIP_DEVICES
    std::vector<int> devices;                      // the devices of ctx, then of peers
    size_t batch_row_len = 0;                      // rays per interleaved row of a multi-device TraverseBatch (0: 4096)
    bool tree_stale = false;                       // the tree is in nodes_ / indices_ (Load(), a detach) and not on the device yet
    uint64_t pending_nodes = 0, pending_indices = 0;  // the sizes of a tree that is on the device only (host_tree_pending_) ...
    T root_bmin[3] = {T(0), T(0), T(0)}, root_bmax[3] = {T(0), T(0), T(0)};  // ... and its root's box
  };
  // The geometry the contexts were built over: the arrays the last built-in Build() (then Refit(), RefitGeometry(), SetPrimMasks())
  // was given, by pointer — SendPrimitives() sends a fresh context exactly this.
  struct DeviceGeometry {
    int kind = -1;           // 0 triangles, 1 spheres, 2 cylinders, 3 curves, -1 nothing usable
    unsigned int count = 0;  // primitives
    const T *vertices = NULL, *vertices1 = NULL;  // triangles: keyframe 0, keyframe 1 of a MotionTriangleMesh (NULL: none) ...
    size_t stride = 0;                            // ... their stride in bytes ...
    const unsigned int *faces = NULL, *masks = NULL;  // ... the faces, the visibility masks of the last SetPrimMasks() (NULL: none)
    const float *positions = NULL, *radii = NULL;  // spheres: centers; cylinders: endpoints; curves: control points
    bool cyl_test_cap = true;  // the cylinder intersector's flag and the curve intersector's subdivision count the contexts
    int crv_subdiv = 4;        // hold now (the intersectors' defaults after a Build())
  };
  static DeviceGeometry MeshRecord(unsigned int n, const T *vertices, const T *vertices1, size_t stride, const unsigned int *faces) {
    DeviceGeometry g;  // (no masks: nrtSetMesh drops them, they belong to the mesh)
    g.count = n;
    g.vertices = vertices;
    g.vertices1 = vertices1;
    g.stride = stride;
    g.faces = faces;
    return g;
  }
  static DeviceGeometry RadiusRecord(unsigned int n, const float *positions, const float *radii) {
    DeviceGeometry g;
    g.count = n;
    g.positions = positions;
    g.radii = radii;
    return g;
  }
  // Built-in primitive types: construction on the GPU through the C ABI.  Each overload states what the contexts will hold as a
  // fresh record (the arrays are kept by pointer: a copy-on-write detach sends them to the new context) and how to send it.
  bool BuildImpl(unsigned int n, const TriangleMesh<T> &mesh, const TriangleSAHPred<T> &pred, const BVHBuildOptions<T> &options,
                 detail::triangle_tag) {
    (void)pred;
    const DeviceGeometry g = MeshRecord(n, mesh.GetVertices(), NULL, mesh.GetVertexStrideBytes(), mesh.GetFaces());
    return HipBuild(options, 0, g, [&](nrt_ctx *c) { return Api::SetMesh(c, g.vertices, g.stride, g.faces, n); });
  }
  // A triangle mesh with a second vertex keyframe: nrtSetMesh + nrtSetMeshMotion + nrtBuild.  The accel stays a triangle accel (the
  // triangle batch methods answer for keyframe 0); TraverseBatchMotion() / OccludedBatchMotion() trace it with one time per ray.
  bool BuildImpl(unsigned int n, const MotionTriangleMesh<T> &mesh, const MotionTriangleSAHPred<T> &pred, const BVHBuildOptions<T> &options,
                 detail::motion_triangle_tag) {
    (void)pred;
    const DeviceGeometry g = MeshRecord(n, mesh.GetVertices(), mesh.GetVertices1(), mesh.GetVertexStrideBytes(), mesh.GetFaces());
    return HipBuild(options, 0, g, [&](nrt_ctx *c) {
      const nrt_status st = Api::SetMesh(c, g.vertices, g.stride, g.faces, n);
      return st != NRT_OK ? st : Api::SetMeshMotion(c, g.vertices1, g.stride);
    });
  }
  bool BuildImpl(unsigned int n, const SphereGeometry &geom, const SpherePred &pred, const BVHBuildOptions<T> &options,
                 detail::sphere_tag) {
    (void)pred;
    const DeviceGeometry g = RadiusRecord(n, geom.GetCenters(), geom.GetRadii());
    return HipBuild(options, 1, g, [&](nrt_ctx *c) { return nrtSetSpheres_f32(c, g.positions, g.radii, n); });
  }
  // (the intersector's test_cap flag and num_subdivisions are traversal-time properties: TraverseBatch() re-sends the primitives
  // when one differs from the record's, which starts at the intersectors' defaults: caps tested, 4 subdivisions)
  bool BuildImpl(unsigned int n, const CylinderGeometry &geom, const CylinderPred &pred, const BVHBuildOptions<T> &options,
                 detail::cylinder_tag) {
    (void)pred;
    const DeviceGeometry g = RadiusRecord(n, geom.GetEndpoints(), geom.GetRadii());
    return HipBuild(options, 2, g, [&](nrt_ctx *c) { return nrtSetCylinders_f32(c, g.positions, g.radii, n, g.cyl_test_cap ? 1 : 0); });
  }
  bool BuildImpl(unsigned int n, const BezierCurveGeometry &geom, const BezierCurvePred &pred, const BVHBuildOptions<T> &options,
                 detail::curve_tag) {
    (void)pred;
    const DeviceGeometry g = RadiusRecord(n, geom.GetControlPoints(), geom.GetRadii());
    return HipBuild(options, 3, g, [&](nrt_ctx *c) { return nrtSetCurves_f32(c, g.positions, g.radii, n, static_cast<uint32_t>(g.crv_subdiv)); });
  }

  // `g` becomes the object's record (its kind only once the tree is built: -1, nothing usable, until then); `set_prims` sends it.
  template <class SetPrims>
  bool HipBuild(const BVHBuildOptions<T> &options, int prim_kind, const DeviceGeometry &g, SetPrims set_prims) {
    const unsigned int n = g.count;
    geom_ = g;
    static_assert(sizeof(BVHNode<T>) == sizeof(typename Api::NodePod), "BVHNode layout");
    static_assert(sizeof(BVHBuildOptions<T>) == sizeof(typename Api::BuildPod), "BVHBuildOptions layout");
    static_assert(sizeof(BVHBuildStatistics) == sizeof(nrt_build_stats), "BVHBuildStatistics layout");
    options_ = options;
    stats_ = BVHBuildStatistics();
    DropPendingHostTree();
    nodes_.clear();
    indices_.clear();
    assert(options_.bin_size > 1);
    if (n == 0) return false;
    if (SharesDeviceContext()) {  // copy-on-write: the copies keep the contexts they share with this object
      dev_.ctx.reset();
      dev_.peers.clear();
    }
    if (!dev_.ctx && !CreateContexts(DeviceList())) return false;
    nrt_ctx *c = Context();
    typename Api::BuildPod o;
    std::memcpy(&o, &options, sizeof(o));
    nrt_build_stats st;
    uint64_t num_nodes = 0;
    if (!Ok(set_prims(c)) || !Ok(Api::Build(c, &o, &st, &num_nodes))) {
      fprintf(stderr, "[nanort] HIP build failed: %s\n", backend_error_.c_str());
      return false;
    }
    // (the index array names a primitive once per leaf slot: n entries, except for cylinders the library cut into segments for
    // its builder, which are named once per segment — the reference's Traverse takes such a tree as it is)
    uint64_t tree_nodes = num_nodes, tree_indices = n;
    if (nrtTreeSize(c, &tree_nodes, &tree_indices) != NRT_OK) tree_indices = n;
    // The arrays stay on the device until the host asks for them (EnsureHostTree): an application that only calls
    // TraverseBatch() never pays the 27 MB read-back of a 1 M-triangle tree.  The root's box comes back now (24 / 48 bytes).
    dev_.pending_nodes = num_nodes;
    dev_.pending_indices = tree_indices;
    if (!Ok(Api::TreeBounds(c, dev_.root_bmin, dev_.root_bmax))) return false;
    __atomic_store_n(&host_tree_pending_, true, __ATOMIC_RELEASE);
    static const bool eager = std::getenv("NANORT_HIP_EAGER_READBACK") != NULL && std::atoi(std::getenv("NANORT_HIP_EAGER_READBACK")) != 0;
    if (eager) {
      EnsureHostTree();
      if (nodes_.empty()) return false;
    }
    stats_.max_tree_depth = st.max_tree_depth;
    stats_.num_leaf_nodes = st.num_leaf_nodes;
    stats_.num_branch_nodes = st.num_branch_nodes;
    stats_.build_secs = st.build_secs;
    // replicas on the other devices: the same primitives, the same (deterministic) build
    for (size_t k = 1; k < NumHipDevices(); k++) {
      nrt_build_stats pst;
      uint64_t pn = 0;
      if (set_prims(Context(k)) != NRT_OK || Api::Build(Context(k), &o, &pst, &pn) != NRT_OK || pn != num_nodes) {
        backend_error_ = nrtLastError(Context(k));
        fprintf(stderr, "[nanort] HIP build of replica %zu failed (%s): tracing on one device\n", k, backend_error_.c_str());
        dev_.peers.clear();
        dev_.devices.resize(1);
        break;
      }
    }
    dev_.tree_stale = false;
    geom_.kind = prim_kind;
    return true;
  }

  // The devices a Build() uses: NANORT_HIP_DEVICES ("all" or a comma-separated list; the first is the primary) or the one of
  // NANORT_HIP_DEVICE (default 0).
  static std::vector<int> DeviceList() {
    std::vector<int> devices;
    if (const char *list = std::getenv("NANORT_HIP_DEVICES")) {
      if (std::strcmp(list, "all") == 0) {
        for (int d = 0; d < nrtDeviceCount(); d++) devices.push_back(d);
      } else {
        for (const char *p = list; *p;) {
          devices.push_back(std::atoi(p));
          while (*p && *p != ',') p++;
          if (*p == ',') p++;
        }
      }
    }
    if (devices.empty()) {
      int device = 0;
      if (const char *env = std::getenv("NANORT_HIP_DEVICE")) device = std::atoi(env);
      devices.push_back(device);
    }
    return devices;
  }
  // Fresh contexts on `devices` (the primary on the first, a replica on each other one that opens), replacing the current ones.
  bool CreateContexts(const std::vector<int> &devices) const {
    dev_.ctx.reset();
    dev_.peers.clear();
    dev_.devices.clear();
    for (size_t k = 0; k < devices.size(); k++) {
      nrt_ctx *raw = NULL;
      if (nrtCreate(devices[k], &raw) != NRT_OK) {
        backend_error_ = nrtLastError(NULL);
        if (k == 0) {
          fprintf(stderr, "[nanort] HIP backend unavailable: %s\n", backend_error_.c_str());
          return false;
        }
        fprintf(stderr, "[nanort] HIP device %d unavailable (%s): continuing with %zu device(s)\n", devices[k], backend_error_.c_str(), k);
        break;
      }
      if (k == 0)
        dev_.ctx = std::shared_ptr<nrt_ctx>(raw, detail::CtxDeleter());
      else
        dev_.peers.push_back(std::shared_ptr<nrt_ctx>(raw, detail::CtxDeleter()));
      dev_.devices.push_back(devices[k]);
    }
    return true;
  }
  // Copies share the contexts until one side changes what they hold (O(1): no device call, no read-back).
  bool SharesDeviceContext() const {
    if (dev_.ctx.use_count() > 1) return true;
    for (size_t k = 0; k < dev_.peers.size(); k++)
      if (dev_.peers[k].use_count() > 1) return true;
    return false;
  }
  // The record's primitives to one context (`cylinder_cap`: the cylinder intersector's flag to send, which may be a new one).
  nrt_status SendPrimitives(nrt_ctx *c, bool cylinder_cap) const {
    const DeviceGeometry &g = geom_;
    switch (g.kind) {
      case 0: {
        nrt_status st = Api::SetMesh(c, g.vertices, g.stride, g.faces, g.count);
        if (st == NRT_OK && g.vertices1) st = Api::SetMeshMotion(c, g.vertices1, g.stride);
        return (st != NRT_OK || !g.masks) ? st : nrtSetPrimMasks(c, g.masks, g.count);
      }
      case 1: return nrtSetSpheres_f32(c, g.positions, g.radii, g.count);
      case 2: return nrtSetCylinders_f32(c, g.positions, g.radii, g.count, cylinder_cap ? 1 : 0);
      case 3: return nrtSetCurves_f32(c, g.positions, g.radii, g.count, static_cast<uint32_t>(g.crv_subdiv));
      default: return NRT_ERR_INVALID;
    }
  }
  // Copy-on-write (caller holds batch_mutex_): leave the contexts shared with copies to them and move to fresh ones on the
  // same devices, holding this object's primitives; the caller then sends the tree (from the host arrays).
  bool DetachDeviceContext(bool cylinder_cap) const {
    const std::vector<int> devices = dev_.devices.empty() ? DeviceList() : dev_.devices;
    dev_.tree_stale = true;  // (until the caller has sent the tree: a failure below leaves a state the next call retries)
    if (!CreateContexts(devices)) return false;
    for (size_t k = 0; k < NumHipDevices(); k++)
      if (!Ok(SendPrimitives(Context(k), cylinder_cap), Context(k))) return false;
    return true;
  }
#endif

#ifdef NANORT_USE_HIP_BACKEND
  mutable std::vector<BVHNode<T> > nodes_;  // (mutable: filled by EnsureHostTree() on the first host access after a GPU build)
  mutable std::vector<unsigned int> indices_;
#else
  std::vector<BVHNode<T> > nodes_;
  std::vector<unsigned int> indices_;
#endif
  BVHBuildOptions<T> options_;
  BVHBuildStatistics stats_;
  unsigned int pad0_;
#ifdef NANORT_USE_HIP_BACKEND
  void DropPendingHostTree() { __atomic_store_n(&host_tree_pending_, false, __ATOMIC_RELEASE); }
  // A copy materialises the source's host tree first and takes it, shares the source's contexts and takes its record; the
  // staging stays with its owner (scratch, grown on the first TraverseBatch()) and nothing is pending in the copy.
  void CopyFrom(const BVHAccel &o) {
    o.EnsureHostTree();
    std::lock_guard<std::mutex> lock(o.batch_mutex_);  // (o's contexts may be replaced by a batch call of another thread)
    nodes_ = o.nodes_;
    indices_ = o.indices_;
    options_ = o.options_;
    stats_ = o.stats_;
    dev_ = o.dev_;
    geom_ = o.geom_;
    host_tree_pending_ = false;
    backend_error_ = o.backend_error_;
  }
  template <class Record>
  static Record Take(Record *r) noexcept {  // (what *r held; *r is left default-constructed)
    Record taken(std::move(*r));
    *r = Record();
    return taken;
  }
  // Everything as it is, the pending read-back and the staging included; `o` is left empty (IsValid() false): no contexts, the
  // records at their defaults.
  void MoveFrom(BVHAccel *o) noexcept {
    nodes_ = std::move(o->nodes_);
    indices_ = std::move(o->indices_);
    o->nodes_.clear();
    o->indices_.clear();
    options_ = o->options_;
    stats_ = o->stats_;
    host_tree_pending_ = o->HostTreePending();
    o->DropPendingHostTree();
    dev_ = Take(&o->dev_);
    geom_ = Take(&o->geom_);
    stage_hits_ = std::move(o->stage_hits_);
    stage_mask_ = std::move(o->stage_mask_);
    stage_hits_cap_ = o->stage_hits_cap_;
    stage_mask_cap_ = o->stage_mask_cap_;
    o->stage_hits_cap_ = o->stage_mask_cap_ = 0;
    backend_error_ = std::move(o->backend_error_);
    o->backend_error_.clear();
  }
  mutable bool host_tree_pending_ = false;  // the tree of the last GPU Build() has not been copied to nodes_ / indices_ yet
  // (mutable, both: a const batch call may move the object to contexts of its own, copy-on-write — DetachDeviceContext — and
  // re-send the primitives with a new cap flag or subdivision count)
  mutable DeviceState dev_;
  mutable DeviceGeometry geom_;
  mutable std::mutex batch_mutex_;  // one per object, never copied: see the comment above TraverseBatch
  // TraverseBatch staging (grow-only): pinned through nrtHostAlloc, plain malloc if that fails
  mutable std::shared_ptr<void> stage_hits_, stage_mask_;
  mutable size_t stage_hits_cap_ = 0, stage_mask_cap_ = 0;
  static void StageFreePinned(void *p) { nrtHostFree(p); }
  static void *StageEnsure(std::shared_ptr<void> *buf, size_t *cap, size_t bytes) {
    if (bytes <= *cap && buf->get()) return buf->get();
    const size_t want = bytes + bytes / 4;
    void *p = NULL;
    buf->reset();
    *cap = 0;
    if (nrtHostAlloc(want, &p) == NRT_OK && p) {
      buf->reset(p, StageFreePinned);
    } else {
      p = std::malloc(want);
      if (!p) return NULL;
      buf->reset(p, std::free);
    }
    *cap = want;
    return p;
  }
  mutable std::string backend_error_;
#endif
};

// Layouts shared with the device code and the reference.
static_assert(sizeof(Ray<float>) == 36 && sizeof(Ray<double>) == 72, "Ray layout");
static_assert(sizeof(BVHNode<float>) == 40 && sizeof(BVHNode<double>) == 64, "BVHNode layout");
static_assert(sizeof(TriangleIntersection<float>) == 16 && sizeof(TriangleIntersection<double>) == 32, "hit layout");
static_assert(sizeof(BVHBuildOptions<float>) == 28 && sizeof(BVHBuildOptions<double>) == 32, "build options layout");
static_assert(sizeof(BVHTraceOptions) == 16 && sizeof(BVHBuildStatistics) == 16, "trace options / stats layout");

}  // namespace nanort

#endif  // NANORT_H_

// nanort_amd/csrc/traverse_dev.h — the device pieces of the binary-loop traversal that more than one kernel file uses
// (traverse.hip and scene_kernels.hip through walk_dev.h; traverse.hip and own_walks.hip through binary_walk_dev.h, which
// states the loop itself): ray setup, slab and primitive tests, ray claims, streaming loads / stores, completion records, the lane
// stack and, at the end, the host side of a persistent launch.  Everything here is a template, forceinline device code or a static
// host function, so each including file compiles its own copy.
#pragma once

#include "common.h"

namespace nrt {

template <typename T>
struct Const;
template <>
struct Const<float> {
  static __device__ __forceinline__ float eps() { return 1.1920928955078125e-07f; }
  static __device__ __forceinline__ float inf() { return __builtin_huge_valf(); }
  static __device__ __forceinline__ float maxmult() { return 1.00000024f; }
  static __device__ __forceinline__ float abs(float x) { return __builtin_fabsf(x); }
  static __device__ __forceinline__ float fmax(float a, float b) { return __builtin_fmaxf(a, b); }
  static __device__ __forceinline__ float fmin(float a, float b) { return __builtin_fminf(a, b); }
  static __device__ __forceinline__ float sqrt(float x) { return __builtin_sqrtf(x); }
  static __device__ __forceinline__ float fltmax() { return 3.402823466e+38f; }
};
template <>
struct Const<double> {
  static __device__ __forceinline__ double eps() { return 2.220446049250313e-16; }
  static __device__ __forceinline__ double inf() { return __builtin_huge_val(); }
  static __device__ __forceinline__ double maxmult() { return 1.0000000000000004; }
  static __device__ __forceinline__ double abs(double x) { return __builtin_fabs(x); }
  static __device__ __forceinline__ double fmax(double a, double b) { return __builtin_fmax(a, b); }
  static __device__ __forceinline__ double fmin(double a, double b) { return __builtin_fmin(a, b); }
  static __device__ __forceinline__ double sqrt(double x) { return __builtin_sqrt(x); }
  static __device__ __forceinline__ double fltmax() { return 3.402823466e+38; } // the example is fp32 only
};

template <typename T>
__device__ __forceinline__ T sel3(T a0, T a1, T a2, int k) {
  return k == 0 ? a0 : (k == 1 ? a1 : a2);
}

// vsafe_inverse, non-C++11 arm (nanort.h:442-461).
template <typename T>
__device__ __forceinline__ T safe_inverse(T v) {
  if (Const<T>::abs(v) < Const<T>::eps()) {
    T sgn = (v < T(0)) ? T(-1) : T(1);
    return Const<T>::inf() * sgn;
  }
  return T(1.0) / v;
}

// Per-lane traversal state (all registers).
template <typename T>
struct Lane {
  // (scalars, not arrays, and no two floats of one kind next to each other: the vectoriser otherwise merges neighbours
  // into overlapping vector accesses that pin parts of the lane state in scratch memory)
  T org0, inv0, org1, inv1, org2, inv2;
  __device__ __forceinline__ T org(int k) const { return k == 0 ? org0 : (k == 1 ? org1 : org2); }
  __device__ __forceinline__ T inv(int k) const { return k == 0 ? inv0 : (k == 1 ? inv1 : inv2); }
  T min_t, max_t, hit_t; // hit_t == intersector t_ == best so far
  T d0, d1, d2;          // ray direction (sphere / cylinder kinds; dead otherwise)
  uint32_t cap;          // cylinder kind: hit_cap_ of the accepted hit (u, v hold u_param_, v_param_)
  // (floats and integers alternate on purpose: as neighbours, Sx Sy Sz u v get merged into overlapping two- and
  // four-float vector accesses by the vectoriser, which then pins all five in scratch memory instead of registers)
  T Sx;
  uint32_t pk; // (dir < 0 per axis) << 0..2 | kx << 3 | ky << 5 | kz << 7: six small integers in one register (the kernel sits near
               // the 80-register edge of six waves per SIMD; the loops turn the fields into lane masks once, on entry).  The signs
               // are the lowest bits so that sign(axis) is ONE bit-field extract at `axis` — three instructions fewer per step
               // than with the signs above the axes (round 6)
  T Sy;
  uint32_t prim;
  T Sz;
  uint32_t so0; // 48 if dir[k] < 0 else 0: byte offset of the ray's NEAR plane row inside a Wide4Node (bmax rows sit 48 bytes after bmin rows)
  T u;
  uint32_t so1;
  T v;
  uint32_t so2;
  __device__ __forceinline__ int kx() const { return (int)((pk >> 3) & 3u); }
  __device__ __forceinline__ int ky() const { return (int)((pk >> 5) & 3u); }
  __device__ __forceinline__ int kz() const { return (int)((pk >> 7) & 3u); }
  __device__ __forceinline__ int sign(int k) const { return (int)((pk >> k) & 1u); }
};

template <typename T>
__device__ __forceinline__ void lane_init(Lane<T> &L, const typename Wire<T>::Ray &r) {
  T d0 = r.dir[0], d1 = r.dir[1], d2 = r.dir[2];
  L.d0 = d0;
  L.d1 = d1;
  L.d2 = d2;
  L.org0 = r.org[0];
  L.org1 = r.org[1];
  L.org2 = r.org[2];
  L.min_t = r.min_t;
  L.max_t = r.max_t;
  L.hit_t = r.max_t; // nanort.h:2494, 2501
  L.prim = kInvalid;
  L.cap = 0u;
  L.u = T(0);
  L.v = T(0);
  // PrepareTraversal (nanort.h:1170-1193)
  int kz = 0;
  T a = Const<T>::abs(d0);
  if (a < Const<T>::abs(d1)) {
    kz = 1;
    a = Const<T>::abs(d1);
  }
  if (a < Const<T>::abs(d2)) {
    kz = 2;
    a = Const<T>::abs(d2);
  }
  int kx = kz + 1;
  if (kx == 3) kx = 0;
  int ky = kx + 1;
  if (ky == 3) ky = 0;
  T dz = sel3(d0, d1, d2, kz);
  if (dz < T(0)) {
    int t = kx;
    kx = ky;
    ky = t;
  }
  uint32_t pk = ((uint32_t)kx << 3) | ((uint32_t)ky << 5) | ((uint32_t)kz << 7);
  L.Sx = sel3(d0, d1, d2, kx) / dz;
  L.Sy = sel3(d0, d1, d2, ky) / dz;
  L.Sz = T(1.0) / dz;
  // Traverse prologue (nanort.h:2505-2516)
  pk |= (d0 < T(0) ? 1u : 0u) | (d1 < T(0) ? 2u : 0u) | (d2 < T(0) ? 4u : 0u);
  L.pk = pk;
  L.so0 = d0 < T(0) ? 48u : 0u;
  L.so1 = d1 < T(0) ? 48u : 0u;
  L.so2 = d2 < T(0) ? 48u : 0u;
  L.inv0 = safe_inverse<T>(d0);
  L.inv1 = safe_inverse<T>(d1);
  L.inv2 = safe_inverse<T>(d2);
}

// One axis of IntersectRayAABB (nanort.h:2285-2370): the near plane `lo` and the far plane `hi` (chosen by the ray's direction
// sign) narrow the interval.  safemax(t0, tmin) / safemin(t1, tmax) (nanort.h:1236-1243): a NaN first operand is dropped and the
// running value is never NaN, which is exactly maxNum/minNum (v_max_f32 / v_min_f32); the only difference, the sign of a zero
// result, cannot change `tmin <= tmax`.  (The packed two-box forms of walk_dev.h write the same operations over register pairs.)
template <typename T>
__device__ __forceinline__ void slab_axis(T lo, T hi, T org, T inv, T &tmin, T &tmax) {
  const T t0 = (lo - org) * inv;
  const T t1 = ((hi - org) * inv) * Const<T>::maxmult();
  tmin = Const<T>::fmax(t0, tmin);
  tmax = Const<T>::fmin(t1, tmax);
}

// IntersectRayAABB (nanort.h:2285-2370) over a box given as {bmin[3], bmax[3]}; `tmin_out`: where the ray enters it.
template <typename T>
__device__ __forceinline__ bool slab_test_tmin(const Lane<T> &L, const T bmin[3], const T bmax[3], T &tmin_out) {
  T tmin = L.min_t, tmax = L.hit_t;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int sg = L.sign(k);
    slab_axis<T>(sg ? bmax[k] : bmin[k], sg ? bmin[k] : bmax[k], L.org(k), L.inv(k), tmin, tmax);
  }
  tmin_out = tmin;
  return tmin <= tmax;
}
template <typename T>
__device__ __forceinline__ bool slab_test(const Lane<T> &L, const T bmin[3], const T bmax[3]) {
  T tmin;
  return slab_test_tmin<T>(L, bmin, bmax, tmin);
}

// TriangleIntersector::Intersect (nanort.h:1054-1150) against one leaf record, up to the hit distance and the barycentrics: every
// reject of the reference in its own order, the accept rule (nanort.h:1133-1139) left to the caller.  The ray constants come as
// VALUES — a lane's own (tri_test) or another lane's, fetched across the wave (leaf items, the tail of a launch): THE one
// statement of this arithmetic.  Written as one running predicate with select-style updates: all loads of the record are issued
// together, and the lane state stays in the same registers on every path.  PLAIN: trace options that cannot reject a primitive.
template <typename T>
struct TriSolve {
  bool ok;      // the record passed every reject; tt, uu, vv are 0 otherwise
  T tt, uu, vv; // hit distance, barycentrics
};
template <typename T, bool PLAIN = false>
__device__ __forceinline__ TriSolve<T> tri_solve(const LeafTri<T> &tri, bool active, T org0, T org1, T org2, T Sx, T Sy, T Sz, int kx, int ky,
                                                 int kz, uint32_t range0, uint32_t range1, uint32_t skip, bool cull) {
  const uint32_t prim = tri.prim_id;
  bool ok = PLAIN ? active : (active & (prim >= range0) & (prim < range1) & (prim != skip)); // nanort.h:2387-2395
  if (PLAIN) cull = false;
  const T A0 = tri.p0[0] - org0, A1 = tri.p0[1] - org1, A2 = tri.p0[2] - org2;
  const T B0 = tri.p1[0] - org0, B1 = tri.p1[1] - org1, B2 = tri.p1[2] - org2;
  const T C0 = tri.p2[0] - org0, C1 = tri.p2[1] - org1, C2 = tri.p2[2] - org2;
  const T Akz = sel3(A0, A1, A2, kz), Bkz = sel3(B0, B1, B2, kz), Ckz = sel3(C0, C1, C2, kz);
  const T Ax = sel3(A0, A1, A2, kx) - Sx * Akz;
  const T Ay = sel3(A0, A1, A2, ky) - Sy * Akz;
  const T Bx = sel3(B0, B1, B2, kx) - Sx * Bkz;
  const T By = sel3(B0, B1, B2, ky) - Sy * Bkz;
  const T Cx = sel3(C0, C1, C2, kx) - Sx * Ckz;
  const T Cy = sel3(C0, C1, C2, ky) - Sy * Ckz;
  T U = Cx * By - Cy * Bx;
  T V = Ax * Cy - Ay * Cx;
  T W = Bx * Ay - By * Ax;
  if (ok && (U == T(0) || V == T(0) || W == T(0))) { // nanort.h:1094-1107 (rare: a wave-level branch)
    const double CxBy = double(Cx) * double(By), CyBx = double(Cy) * double(Bx);
    const double AxCy = double(Ax) * double(Cy), AyCx = double(Ay) * double(Cx);
    const double BxAy = double(Bx) * double(Ay), ByAx = double(By) * double(Ax);
    U = T(CxBy - CyBx);
    V = T(AxCy - AyCx);
    W = T(BxAy - ByAx);
  }
  const bool neg = (U < T(0)) | (V < T(0)) | (W < T(0)); // nanort.h:1109-1116
  const bool pos = (U > T(0)) | (V > T(0)) | (W > T(0));
  ok = ok & !(neg & (cull | pos));
  const T det = U + V + W;
  ok = ok & !(det == T(0));
  TriSolve<T> r = {ok, T(0), T(0), T(0)};
  if (ok) { // skipped by the whole wave when no lane got this far
    const T Az = Sz * Akz, Bz = Sz * Bkz, Cz = Sz * Ckz;
    const T D = U * Az + V * Bz + W * Cz;
    const T rcp = T(1.0) / det;
    r.tt = D * rcp;
    r.uu = V * rcp;
    r.vv = W * rcp;
  }
  return r;
}

// ... against a lane's own ray, with the reference's accept rule.
template <typename T, bool PLAIN = false>
__device__ __forceinline__ void tri_test(Lane<T> &L, const LeafTri<T> &tri, bool active, uint32_t range0,
                                         uint32_t range1, uint32_t skip, bool cull) {
  const TriSolve<T> s = tri_solve<T, PLAIN>(tri, active, L.org0, L.org1, L.org2, L.Sx, L.Sy, L.Sz, L.kx(), L.ky(), L.kz(), range0, range1, skip, cull);
  if (s.ok) {
    // `if (tt > t) return; if (tt < min_t) return;` — equality (and NaN) accepted (nanort.h:1133-1139)
    const bool acc = !(s.tt > L.hit_t) & !(s.tt < L.min_t);
    L.hit_t = acc ? s.tt : L.hit_t;
    L.u = acc ? s.uu : L.u;
    L.v = acc ? s.vv : L.v;
    L.prim = acc ? tri.prim_id : L.prim;
  }
}

// SphereIntersector::Intersect (examples/particle_primitive/main.cc:161-236) against one leaf record: the
// quadratic in the reference's own operation order (vdot = (x*x + y*y) + z*z, nanort.h:410-412), IEEE sqrt and
// divisions, no contraction.  No min_t test and no skip_prim_id in that intersector; equality with the best t
// is accepted (`if (t > *t_inout) return false`).
template <typename T>
__device__ __forceinline__ void sphere_test(Lane<T> &L, const LeafSphere<T> &sp, bool active, uint32_t range0,
                                            uint32_t range1) {
  const uint32_t prim = sp.prim_id;
  bool ok = active & (prim >= range0) & (prim < range1);
  const T oc0 = L.org0 - sp.c[0], oc1 = L.org1 - sp.c[1], oc2 = L.org2 - sp.c[2];
  const T a = (L.d0 * L.d0 + L.d1 * L.d1) + L.d2 * L.d2;
  const T b = T(2.0) * ((L.d0 * oc0 + L.d1 * oc1) + L.d2 * oc2);
  const T c = ((oc0 * oc0 + oc1 * oc1) + oc2 * oc2) - sp.r * sp.r;
  const T disc = b * b - T(4.0) * a * c;
  ok = ok & !(disc < T(0));
  if (ok) {
    T t0, t1;
    if (Const<T>::abs(disc) < Const<T>::eps()) {
      t0 = t1 = T(-0.5) * (b / a);
    } else {
      const T ds = Const<T>::sqrt(disc);
      const T q = (b < T(0)) ? (-b - ds) / T(2.0) : (-b + ds) / T(2.0);
      t0 = q / a;
      t1 = c / q;
    }
    if (t0 > t1) {
      const T tmp = t0;
      t0 = t1;
      t1 = tmp;
    }
    const T t = (t0 < T(0)) ? t1 : t0;
    const bool acc = ok & !(t1 < T(0)) & !(t > L.hit_t);
    L.hit_t = acc ? t : L.hit_t;
    L.prim = acc ? prim : L.prim;
  }
}

// CylinderIntersector::Intersect (examples/cylinder_primitive/main.cc:237-343) with solve2e (:61-90) against one leaf
// record, as one running predicate (the reference's early returns in the same order, every comparison in the
// reference's own form so that NaNs take the same side).  The intersector's mutable members hit_cap_, u_param_,
// v_param_ are the lane's cap, u, v: as there, they change exactly when the primitive is accepted.
template <typename T>
__device__ __forceinline__ void cyl_normalize(const T a[3], T o[3]) { // vnormalize, nanort.h:383-398
  const T len = Const<T>::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  o[0] = a[0];
  o[1] = a[1];
  o[2] = a[2];
  if (Const<T>::abs(len) > Const<T>::eps()) {
    const T inv_len = T(1.0) / len;
    o[0] *= inv_len;
    o[1] *= inv_len;
    o[2] *= inv_len;
  }
}
template <typename T>
__device__ __forceinline__ T cyl_dot(const T a[3], const T b[3]) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

template <typename T>
__device__ __forceinline__ void cylinder_test(Lane<T> &L, const LeafCylinder<T> &cy, bool active, uint32_t range0,
                                              uint32_t range1, bool test_cap) {
  const uint32_t prim = cy.prim_id;
  const bool ok = active & (prim >= range0) & (prim < range1);
  const T kEPS = T(1.0e-6f);
  const T org[3] = {L.org0, L.org1, L.org2}, dir[3] = {L.d0, L.d1, L.d2};
  const T tmax = L.hit_t;
  const T rr = (cy.r0 < cy.r1) ? cy.r1 : cy.r0; // std::max(r0, r1)
  T d[3], m[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    d[k] = cy.p1[k] - cy.p0[k];
    m[k] = org[k] - cy.p0[k];
  }
  const T md = cyl_dot(m, d), nd = cyl_dot(dir, d), dd = cyl_dot(d, d);
  bool hitCap = false;
  T capT = Const<T>::fltmax();
  T t_new = tmax, u_new = L.u, v_new = L.v;
  uint32_t cap_new = L.cap;
  if (test_cap) {
    T t01[3], dN0[3], dN1[3], rd[3];
#pragma unroll
    for (int k = 0; k < 3; k++) t01[k] = cy.p0[k] - cy.p1[k];
    cyl_normalize<T>(t01, dN0);
#pragma unroll
    for (int k = 0; k < 3; k++) dN1[k] = -dN0[k];
    cyl_normalize<T>(dir, rd);
    const bool facing = Const<T>::abs(cyl_dot(dir, dN0)) > kEPS;
    const T p0D = -cyl_dot(cy.p0, dN0), p1D = -cyl_dot(cy.p1, dN1);
    const T p0T = -(cyl_dot(org, dN0) + p0D) / cyl_dot(rd, dN0);
    const T p1T = -(cyl_dot(org, dN1) + p1D) / cyl_dot(rd, dN1);
    T e0[3], e1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      e0[k] = (org[k] + rd[k] * p0T) - cy.p0[k];
      e1[k] = (org[k] + rd[k] * p1T) - cy.p1[k];
    }
    const T qp0Sqr = cyl_dot(e0, e0), qp1Sqr = cyl_dot(e1, e1);
    const bool c0 = facing & (p0T > T(0)) & (p0T < tmax) & (qp0Sqr < rr * rr);
    hitCap = c0;
    capT = c0 ? p0T : capT;
    t_new = c0 ? p0T : t_new;
    u_new = c0 ? Const<T>::sqrt(qp0Sqr) : u_new;
    v_new = c0 ? T(0) : v_new;
    const bool c1 = facing & (p1T > T(0)) & (p1T < tmax) & (p1T < capT) & (qp1Sqr < rr * rr);
    hitCap = hitCap | c1;
    capT = c1 ? p1T : capT;
    t_new = c1 ? p1T : t_new;
    u_new = c1 ? Const<T>::sqrt(qp1Sqr) : u_new;
    v_new = c1 ? T(1.0) : v_new;
    cap_new = hitCap ? 1u : cap_new;
  }
  bool accept = hitCap;
  const bool outside = ((md <= T(0)) & (nd <= T(0))) | ((md >= dd) & (nd >= T(0)));
  {
    const T nn = cyl_dot(dir, dir), mn = cyl_dot(m, dir);
    const T A = dd * nn - nd * nd;
    const T kk = cyl_dot(m, m) - rr * rr;
    const T C = dd * kk - md * md;
    const T B = dd * mn - nd * md;
    // solve2e: the smaller root (root[0]) and whether there is one
    T root;
    bool have;
    if (Const<T>::abs(A) <= kEPS) {
      root = -C / B;
      have = true;
    } else {
      const T D = B * B - A * C;
      if (D < T(0)) {
        root = T(0);
        have = false;
      } else if (D == T(0)) {
        root = -B / A;
        have = true;
      } else {
        T x1 = (Const<T>::abs(B) + Const<T>::sqrt(D)) / A;
        if (B >= T(0)) x1 = -x1;
        const T x2 = C / (A * x1);
        root = (x1 > x2) ? x2 : x1;
        have = true;
      }
    }
    const T t = root;
    T sv = md + t * nd;
    sv = sv / dd;
    const bool side = !outside & have & (T(0) <= t) & (t <= tmax) & (t <= capT) & (T(0) <= sv) & (sv <= T(1));
    accept = accept | side;
    t_new = side ? t : t_new;
    u_new = side ? T(0) : u_new;
    v_new = side ? sv : v_new;
    cap_new = side ? 0u : cap_new;
  }
  accept = accept & ok;
  L.hit_t = accept ? t_new : L.hit_t;
  L.u = accept ? u_new : L.u;
  L.v = accept ? v_new : L.v;
  L.cap = accept ? cap_new : L.cap;
  L.prim = accept ? prim : L.prim;
}

// CurveIntersector::Intersect (examples/curves_primitive/main.cc:637-759) against one leaf record: the curve as `n` line
// segments in a frame whose z axis is the ray (GetZAlign :382-417, Xform :419-430), de Casteljau (:432-454) at s / n, every
// sum in the reference's association and every comparison in its own form so that NaNs take the same side.  There is no min_t
// test, no t >= 0 test and no skip_prim_id in that intersector; `t < current` is strict.  u_param / v_param of the accepted
// segment are the lane's u, v: as there, they change exactly when a segment is accepted, and later segments see the lowered t.
//
// The frame (9 + 3 floats) depends on the ray alone.  It is RECOMPUTED here, at each leaf record, not carried in the lane across
// the walk.  By register count: with the frame recomputed the two instantiations of this kind hold 121 (two levels per step) and
// 117 (one level) VGPRs (111 and 107 before the occlusion copy of the record loop, traverse.hip), no scratch, four waves per SIMD;
// twelve more registers live through the inner-node loop would not fit the 128 that four waves allow, with nothing left before scratch or three waves.  The recomputation is one sqrt,
// three divisions and a dozen multiplies in front of a test of 9 * (n + 1) interpolations, and the compiler is free to hoist it
// out of a leaf's record loop.  It is a pure function of the ray and contraction is off: the values are those a stored frame holds.
struct CurveFrame {
  float m00, m01, m02, m10, m11, m12, m20, m21, m22, t0, t1, t2;
};
__device__ __forceinline__ CurveFrame curve_frame(float ox, float oy, float oz, float lx, float ly, float lz) {
  CurveFrame f;
  const float dxz = __builtin_sqrtf(lx * lx + lz * lz);
  if (dxz > 0.0f) {
    const float lxdxz = lx / dxz, lydxz = ly / dxz, lzdxz = lz / dxz;
    f.m00 = lzdxz;
    f.m01 = -lxdxz * ly;
    f.m02 = lx;
    f.m10 = 0.0f;
    f.m11 = dxz;
    f.m12 = ly;
    f.m20 = -lxdxz;
    f.m21 = -lydxz * lz;
    f.m22 = lz;
  } else { // the ray runs along y (or its direction is zero / NaN)
    f.m00 = 1.0f;
    f.m01 = 0.0f;
    f.m02 = 0.0f;
    f.m10 = 0.0f;
    f.m11 = 0.0f;
    f.m12 = (ly > 0.0f) ? -1.0f : 1.0f;
    f.m20 = 0.0f;
    f.m21 = (ly > 0.0f) ? 1.0f : -1.0f;
    f.m22 = 0.0f;
  }
  f.t0 = -((ox * f.m00 + oy * f.m10) + oz * f.m20);
  f.t1 = -((ox * f.m01 + oy * f.m11) + oz * f.m21);
  f.t2 = -((ox * f.m02 + oy * f.m12) + oz * f.m22);
  return f;
}
// EvaluateBezier on one component: three, two, one linear interpolations
__device__ __forceinline__ float curve_bezier1(float v0, float v1, float v2, float v3, float t) {
  const float u = 1.0f - t;
  const float a0 = v0 * u + v1 * t, a1 = v1 * u + v2 * t, a2 = v2 * u + v3 * t;
  const float b0 = a0 * u + a1 * t, b1 = a1 * u + a2 * t;
  return b0 * u + b1 * t;
}

// `anyhit` (wave-uniform; occlusion queries, traverse.hip "SETTLED"): the segment loop of a lane ends at its first accepted segment —
// later segments could only lower t, and `t < current` with current <= max_t has settled the ray — and neither sqrt(d2) nor the u
// parameter is computed: u, v and prim of such a launch are never read.  The closest-hit loop is the one it always was.
template <typename T>
__device__ __forceinline__ void curve_test(Lane<T> &L, const LeafCurve &cv, bool active, uint32_t range0, uint32_t range1,
                                           uint32_t subdiv, bool anyhit = false) {
  const uint32_t prim = cv.prim_id;
  bool ok = active & (prim >= range0) & (prim < range1);
  const CurveFrame f = curve_frame(L.org0, L.org1, L.org2, L.d0, L.d1, L.d2);
  float x[4], y[4], z[4];
  float t_z = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float px = cv.cp[3 * i + 0], py = cv.cp[3 * i + 1], pz = cv.cp[3 * i + 2];
    x[i] = ((px * f.m00 + py * f.m10) + pz * f.m20) + f.t0;
    y[i] = ((px * f.m01 + py * f.m11) + pz * f.m21) + f.t1;
    z[i] = ((px * f.m02 + py * f.m12) + pz * f.m22) + f.t2;
    t_z = (t_z < z[i]) ? z[i] : t_z;
  }
  const float uw = ((cv.r0 < cv.r3) ? cv.r3 : cv.r0) / 2.0f; // std::max(r0, r3) / 2
  ok = ok & !(t_z < 4.0f * uw);
  if (ok) { // (skipped by the whole wave when no lane got this far)
    const float fn = (float)(int)subdiv, inv_n = 1.0f / fn;
    const float w0 = 0.5f * cv.r0, w1 = 0.5f * cv.r3, bw = w1 - w0;
    float cur = L.hit_t, up = L.u, vp = L.v;
    bool hit = false;
    // (segment s ends where segment s + 1 begins: (s + 1) / n is evaluated once)
    float p1x = curve_bezier1(x[0], x[1], x[2], x[3], 0.0f / fn), p1y = curve_bezier1(y[0], y[1], y[2], y[3], 0.0f / fn),
          p1z = curve_bezier1(z[0], z[1], z[2], z[3], 0.0f / fn);
    if (anyhit) {
      for (uint32_t s = 0; s < subdiv && !hit; s++) { // (the same segments in the same order, up to the first accepted one)
        const float p0x = p1x, p0y = p1y, p0z = p1z;
        const float t1 = (float)(int)(s + 1u) / fn;
        p1x = curve_bezier1(x[0], x[1], x[2], x[3], t1);
        p1y = curve_bezier1(y[0], y[1], y[2], y[3], t1);
        p1z = curve_bezier1(z[0], z[1], z[2], z[3], t1);
        const float ax = 0.0f - p0x, ay = 0.0f - p0y;
        const float bx = p1x - p0x, by = p1y - p0y, bz = p1z - p0z;
        const float d0 = (ax * bx) + (ay * by), d1 = (bx * bx) + (by * by);
        float u = d0 / d1;
        u = (u < 1.0f) ? u : 1.0f;
        u = (0.0f < u) ? u : 0.0f;
        const float qx = p0x + (u * bx), qy = p0y + (u * by), t = p0z + (u * bz), r = w0 + (u * bw);
        const float r2 = r * r, d2 = (qx * qx) + (qy * qy);
        hit = (d2 <= r2) & (t < cur);
        cur = hit ? t : cur;
      }
      L.hit_t = cur;
      return;
    }
    for (uint32_t s = 0; s < subdiv; s++) {
      const float p0x = p1x, p0y = p1y, p0z = p1z;
      const float t1 = (float)(int)(s + 1u) / fn;
      p1x = curve_bezier1(x[0], x[1], x[2], x[3], t1);
      p1y = curve_bezier1(y[0], y[1], y[2], y[3], t1);
      p1z = curve_bezier1(z[0], z[1], z[2], z[3], t1);
      const float ax = 0.0f - p0x, ay = 0.0f - p0y; // the origin projected onto the segment, in the frame's xy plane
      const float bx = p1x - p0x, by = p1y - p0y, bz = p1z - p0z;
      const float d0 = (ax * bx) + (ay * by), d1 = (bx * bx) + (by * by);
      float u = d0 / d1;
      u = (u < 1.0f) ? u : 1.0f; // std::min(1.0f, u): NaN -> 1
      u = (0.0f < u) ? u : 0.0f; // std::max(0.0f, .)
      const float qx = p0x + (u * bx), qy = p0y + (u * by), t = p0z + (u * bz), r = w0 + (u * bw);
      const float r2 = r * r, d2 = (qx * qx) + (qy * qy);
      const bool acc = (d2 <= r2) & (t < cur);
      up = acc ? (u + (float)(int)s) * inv_n : up;
      vp = acc ? __builtin_sqrtf(d2) : vp;
      cur = acc ? t : cur;
      hit = hit | acc;
    }
    L.hit_t = cur; // (unchanged unless a segment was accepted)
    L.u = up;
    L.v = vp;
    L.prim = hit ? prim : L.prim;
  }
}

__device__ __forceinline__ unsigned lane_id() {
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// Which batch a virtual ray index lies in (multi-batch launches: common.h BatchPtrs; the ends are wave-uniform scalars).
template <typename T>
__device__ __forceinline__ uint32_t batch_of(const TraverseArgs<T> &a, uint32_t rid) {
  uint32_t b = 0;
#pragma unroll
  for (int k = 0; k + 1 < kMaxBatches; k++) b += ((uint32_t)(k + 1) < a.num_batches && rid >= a.batch_end[k]) ? 1u : 0u;
  return b;
}
// ... and the batch table copied from the kernel arguments into LDS once per block, so that lanes can index it by their own batch.
#define NRT_BATCH_TABLE_SETUP()                                                                        \
  __shared__ BatchPtrs s_tbl[sizeof(T) == 4 ? kMaxBatches : 1];                                        \
  const bool multi = sizeof(T) == 4 && a.num_batches > 1u; /* (wave-uniform) */                        \
  if (multi) {                                                                                         \
    _Pragma("unroll") for (int k_ = 0; k_ < kMaxBatches; k_++)                                         \
      if (threadIdx.x == (unsigned)k_) s_tbl[sizeof(T) == 4 ? k_ : 0] = a.batches[k_];                 \
    __syncthreads();                                                                                   \
  }

// Work distribution of the persistent kernels.
//  * The batch is cut into `static_bands` equal bands (+ a short tail).  The first part of every band is handed out
//    STATICALLY, without any atomic: slice `rank` of band b, rays [b * band_len + rank * static_per_wave, +static_per_wave),
//    belongs to wave `rank`.  Ranks are XCD-major (the dispatcher places block b on XCD b % 8 — used for L2 affinity only,
//    never for correctness), so at any moment the waves of an XCD walk neighbouring slices of one band and its L2 keeps one
//    part of the tree.  Every wave samples every band: an image whose cost per ray varies from region to region (C2: 40 %
//    sky) does not leave one XCD with the expensive rows.
//  * The rest of every band (and the tail) is claimed DYNAMICALLY, `chunk` rays per atomicAdd.  These rays form one virtual
//    array (band 0's dynamic part, band 1's, ..., the tail) that is cut into `num_parts` ranges with one cursor each (4 KiB
//    apart); a wave drains its home range first and then steals from the others.  Band parts and ranges are whole chunks, so a
//    chunk never straddles two bands.  Because the dynamic rays come from all over the batch too (round 2: the last quarter
//    of the array — for a camera wave the bottom of the image), what is left to balance the end of a launch is a sample of the
//    whole batch, not its cheapest corner.
//    (Device-scope atomics on one word saturate near 100 per microsecond on this part, hence the static share and the modest
//    chunk count.  Round 2 re-measured static share 0-75 %, chunks of 16-128 rays, claims issued one chunk ahead of need:
//    nothing beats 75 % / 128; profiles/r02d_scheduling_sweep.txt.  Round 6, with finer steps: the static share is 16 % — ONE
//    64-ray group per wave at 1080p, enough to start every wave without an atomic — because whatever a wave owns nobody can take
//    from it when the cost per ray is uneven over the image: C2 +7 %, C3 +2.8 %, profiles/r06y_distribution_static_share.txt.)
//  * A batch too small for a static group per wave has no static share at all; its waves then own the FIRST chunk of their home
//    range (chunk `wave index`, no atomic: claim_init) and the cursors count from the range's wave count.
struct Claim {
  uint32_t next, end; // claimed, not yet handed out: [next, end)
  uint32_t part, tried;
  uint32_t rank, band; // static share: this wave's rank, the band its current slice lies in
  bool exhausted;
};

// Chunk `idx` of cursor range `part`: where it starts in the virtual array of dynamic rays and how many rays it holds (false: past
// the range's end).  The cursor counts CHUNKS: the first `main_chunks` are whole ones, the rest of the range goes out in half chunks
// (tunable chunk_tail_pct) — the last rays of a launch in finer portions; half chunks subdivide whole ones, so no chunk straddles two
// bands.
template <typename T>
__device__ __forceinline__ bool chunk_of(const TraverseArgs<T> &a, uint32_t part, uint32_t idx, uint32_t &v, uint32_t &cnt) {
  const uint32_t lo = part * a.dyn_per_part; // range of this part in the virtual array of dynamic rays
  const uint32_t len = (part + 1u == a.num_parts) ? a.dyn_total - lo : a.dyn_per_part;
  const uint32_t main_chunks = (uint32_t)(((unsigned long long)(len / a.chunk) * (100u - a.chunk_tail_pct)) / 100u), half = a.chunk >> 1;
  const uint32_t base = idx < main_chunks ? idx * a.chunk : main_chunks * a.chunk + (idx - main_chunks) * half;
  const uint32_t want = idx < main_chunks ? a.chunk : half;
  if (!(idx < 0x1000000u && base < len)) return false;
  v = lo + base;
  cnt = (len - base < want) ? len - base : want;
  return true;
}
// ... and where those rays lie in the batch
template <typename T>
__device__ __forceinline__ uint32_t dyn_to_real(const TraverseArgs<T> &a, uint32_t v) {
  if (v < a.dyn_banded) { // inside band b's dynamic part
    const uint32_t b = v / a.dyn_per_band;
    return b * a.band_len + a.band_static + (v - b * a.dyn_per_band);
  }
  return a.tail_begin + (v - a.dyn_banded); // the tail behind the last band
}

template <typename T>
__device__ __forceinline__ void claim_init(const TraverseArgs<T> &a, Claim &c) {
  const uint32_t part = blockIdx.x % a.num_parts;
  // (readfirstlane: the compiler cannot see that threadIdx.x / 64 is the same in every lane; told so, it keeps the whole
  // claim state in scalar registers)
  const uint32_t rank = (part * a.blocks_per_part + blockIdx.x / a.num_parts) * (kTraverseBlock / kWave) +
                        (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  c.rank = rank;
  c.band = 0;
  c.next = rank * a.static_per_wave;
  c.end = c.next + a.static_per_wave; // (static_per_wave == 0: nothing is owned statically)
  c.part = part;
  c.tried = 0;
  c.exhausted = false;
  if (a.dyn_head != 0u && a.static_per_wave == 0u) {
    // A batch too small for a static group per wave (fewer than ~400 rays per wave at the default share): no static share, but no
    // start-up burst on the cursors either — chunk `wi` of the wave's HOME range belongs to wave `wi` of that partition without an
    // atomic (the cursors then count from the partition's wave count: claim_chunk), so the launch starts inside every XCD's own
    // strip of the batch and everything after a wave's first chunk is balanced dynamically.  (C3's mesh at 1600x960 +3 %, C2 +2.5 %
    // through its 1.24 M-ray bounce wave: profiles/r06z_dyn_head_small.txt.)
    const uint32_t wi = rank - part * a.blocks_per_part * (uint32_t)(kTraverseBlock / kWave);
    uint32_t v, cnt;
    if (chunk_of<T>(a, part, wi, v, cnt)) {
      c.next = dyn_to_real<T>(a, v);
      c.end = c.next + cnt;
    } else {
      c.next = c.end = 0u;
    }
  }
}

// All lanes of the wave call this (uniform control flow); `leader` is any active lane index.
template <typename T>
__device__ __forceinline__ bool claim_chunk(const TraverseArgs<T> &a, Claim &c, unsigned lane, int leader) {
  if (a.static_per_wave != 0u && c.band + 1u < a.static_bands) { // the wave's slice of the next band (no atomic)
    c.band++;
    c.next = c.band * a.band_len + c.rank * a.static_per_wave;
    c.end = c.next + a.static_per_wave;
    return true;
  }
  while (c.tried < a.num_parts) {
    uint32_t idx = 0;
    if (lane == (unsigned)leader) idx = atomicAdd(a.ray_cursor + kCursorStrideWords * c.part, 1u);
    idx = __builtin_amdgcn_readfirstlane(__shfl(idx, leader));
    if (a.dyn_head != 0u && a.static_per_wave == 0u) idx += a.blocks_per_part * (uint32_t)(kTraverseBlock / kWave); // (the first chunks of every range have owners: claim_init)
    uint32_t v, cnt;
    if (chunk_of<T>(a, c.part, idx, v, cnt)) {
      c.next = dyn_to_real<T>(a, v);
      c.end = c.next + cnt;
      return true;
    }
    c.part = (c.part + 1 == a.num_parts) ? 0 : c.part + 1;
    c.tried++;
  }
  c.exhausted = true;
  return false;
}

// Streaming accesses (each ray is read once, each hit written once): keep them out of the
// way of the tree data in L2 with the non-temporal hint.  (The hit stores of every walk; the ray loads of the multi-hit walk only:
// k_traverse and k_traverse_wide measured slower with it — load_ray below.)
template <typename T>
__device__ __forceinline__ typename Wire<T>::Ray load_ray_nt(const typename Wire<T>::Ray *p) {
  typename Wire<T>::Ray r;
  const uint32_t *src = reinterpret_cast<const uint32_t *>(p);
  uint32_t *dst = reinterpret_cast<uint32_t *>(&r);
#pragma unroll
  for (unsigned k = 0; k < sizeof(r) / 4; k++) dst[k] = __builtin_nontemporal_load(src + k);
  return r;
}
template <typename T>
__device__ __forceinline__ void store_hit_nt(typename Wire<T>::Hit *p, const typename Wire<T>::Hit &h) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 *src = reinterpret_cast<const u32x4 *>(&h);
  u32x4 *dst = reinterpret_cast<u32x4 *>(p);
#pragma unroll
  for (unsigned k = 0; k < sizeof(h) / 16; k++) __builtin_nontemporal_store(src[k], dst + k);
}

// A launch's own streams — rays in; hit records, flags and per-ray skip ids by the ray's index — lie in device memory, whether their
// pointer is a kernel argument or comes out of the multi-batch table in LDS (BatchPtrs).  A pointer read from memory is a generic one
// as far as the compiler can tell, and one selected between the two stays generic: every access through it is a flat_ instruction,
// which also takes a slot of the LDS queue and is waited for on both counters.  The walks therefore hold these pointers as
// global-address-space ones (as walk_dev.h's load_global_record does for the scene kernels' records) and the accesses are global_.
#define NRT_GLOBAL __attribute__((address_space(1)))
template <typename R>
__device__ __forceinline__ R NRT_GLOBAL *as_global(R *p) {
  return (R NRT_GLOBAL *)p;
}
// The same for a pointer INTO THE BLOCK'S LDS that reaches a function as an argument (a row of a __shared__ array): generic there,
// so a volatile access through it is a flat_ instruction with `sc0 sc1`, waited for on its own before the next one is issued.
// Held as a local-address-space pointer the access is a ds_ instruction.
#define NRT_LDS __attribute__((address_space(3)))
template <typename R>
__device__ __forceinline__ R NRT_LDS *as_lds(R *p) {
  return (R NRT_LDS *)p;
}
template <typename T>
__device__ __forceinline__ void store_hit_nt(typename Wire<T>::Hit NRT_GLOBAL *p, const typename Wire<T>::Hit &h) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 *src = reinterpret_cast<const u32x4 *>(&h);
  u32x4 NRT_GLOBAL *dst = (u32x4 NRT_GLOBAL *)p;
#pragma unroll
  for (unsigned k = 0; k < sizeof(h) / 16; k++) __builtin_nontemporal_store(src[k], dst + k);
}
// The ray a lane takes at a refill of the walks (k_traverse, k_traverse_wide): loaded with the DEFAULT cache policy.  The walks used
// to read `(debug & 4) ? plain load : load_ray_nt` of one address, which the compiler merged into one plain load — so the plain load
// is what every launch ran for as long as the select stood there.  With the hint really in the binary (nt on every piece, bypassing the vector L1)
// C3's step is 3.8 % SLOWER (profiles/r11a_ray_streams.txt): the lanes of a wave take neighbouring 36-byte records, so the pieces
// of a wave's rays share their 128-byte lines, and the L1 is what merges them.  Probe bit 4 of `debug` now selects the non-temporal
// load, in the profiling library only (the address goes through an empty asm, so that the two loads stay two in the binary).
template <typename T>
__device__ __forceinline__ typename Wire<T>::Ray load_ray(const typename Wire<T>::Ray NRT_GLOBAL *p, uint32_t debug_flags) {
  typename Wire<T>::Ray r;
  const uint32_t NRT_GLOBAL *src = (const uint32_t NRT_GLOBAL *)p;
  uint32_t *dst = reinterpret_cast<uint32_t *>(&r);
#ifdef NRT_PROF
  if (debug_flags & 4u) { // (wave-uniform)
    asm volatile("" : "+v"(src));
#pragma unroll
    for (unsigned k = 0; k < sizeof(r) / 4; k++) dst[k] = __builtin_nontemporal_load(src + k);
    asm volatile("" : "+v"(dst[0])); // (... and nothing like it ends the other arm: the loads are not sunk into one behind the branch)
    return r;
  }
#endif
  (void)debug_flags;
#pragma unroll
  for (unsigned k = 0; k < sizeof(r) / 4; k++) dst[k] = src[k]; // (neighbouring words: merged into the widest loads the 4-byte alignment allows)
  return r;
}

// Completion record of a launch (common.h, DoneRec): no event is recorded in the stream for it.  Start — one thread of each
// of the first eight blocks stamps the time; end — every wave counts itself out of its block's group (blockIdx % 8: eight
// counters, so that the exit atomics of ~5000 waves do not queue on one word), a group's last wave counts the group out,
// and the last group publishes the two stamps and then the launch's sequence number to the page-locked record.  No LDS
// (the fp64 variants use all of it for their stacks), no barrier, nothing fenced: a waiter learns that every wave has
// stopped READING the tree and the slot's scratch (what a rebuild or the slot's next launch must know), not that the hit
// records have landed — for that the caller synchronises its stream as usual.  Every word a later launch depends on is
// handed on by an atomic (performed at the memory side, visible to every XCD), not left dirty in one XCD's L2.
template <typename T>
__device__ __forceinline__ void done_begin(const TraverseArgs<T> &a) {
  if (a.done_rec != nullptr && threadIdx.x == 0u && blockIdx.x < 8u)
    atomicMin(&a.done_count->t_begin, (unsigned long long)__builtin_amdgcn_s_memrealtime());
}
// The same hand-off at the end of an ordinary (non-persistent) grid — the post passes of the sphere and cylinder kinds, which
// then close the launch's record in place of the traversal kernel: every block counts itself out once all its threads are
// past their reads.
__device__ __forceinline__ void done_end_blocks(DoneRec *rec, DoneCount *cnt, uint32_t seq) {
  if (rec == nullptr) return; // (uniform)
  __syncthreads();
  if (threadIdx.x != 0u) return;
  const uint32_t groups = gridDim.x < 8u ? gridDim.x : 8u, g = blockIdx.x % 8u;
  const uint32_t group_blocks = (gridDim.x - g + 7u) / 8u;
  if (atomicAdd(&cnt->group[g], 1u) != group_blocks - 1u) return;
  (void)atomicExch(&cnt->group[g], 0u);
  if (atomicAdd(&cnt->exited, 1u) != groups - 1u) return;
  (void)atomicExch(&cnt->exited, 0u);
  const unsigned long long t0 = atomicExch(&cnt->t_begin, ~0ull);
  __hip_atomic_store(&rec->t_begin, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&rec->t_end, (unsigned long long)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&rec->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
template <typename T>
__device__ __forceinline__ void done_end(const TraverseArgs<T> &a, unsigned lane) {
  if (a.done_rec == nullptr || !a.done_publish || lane != 0u) return; // (done_publish == 0: a post pass closes the record)
  const uint32_t groups = gridDim.x < 8u ? gridDim.x : 8u, g = blockIdx.x % 8u;
  const uint32_t group_waves = ((gridDim.x - g + 7u) / 8u) * (uint32_t)(kTraverseBlock / kWave);
  DoneCount *cnt = a.done_count;
  if (atomicAdd(&cnt->group[g], 1u) != group_waves - 1u) return; // not the group's last wave
  (void)atomicExch(&cnt->group[g], 0u); // (handed on clean to the slot's next launch)
  if (atomicAdd(&cnt->exited, 1u) != groups - 1u) return; // not the launch's last group
  (void)atomicExch(&cnt->exited, 0u);
  const unsigned long long t0 = atomicExch(&cnt->t_begin, ~0ull);
  DoneRec *r = a.done_rec;
  __hip_atomic_store(&r->t_begin, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&r->t_end, (unsigned long long)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&r->seq, a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// A lane's traversal stack.  Entry i lies in the block's LDS array, lds[i][col], below STACK, and from there on in the launch's
// global overflow arrays at (i - STACK) * spill_stride + gcol.  `col` / `gcol` name the column on both sides: a lane's own
// (threadIdx.x, its global thread index) or, in the tail of a launch, the column of the lane whose ray a quad has taken over.
// SE says what an entry is: StackRef here, StackEntry<T> (reference + t_min; the t_min half lies in spill_tmin) in walk_dev.h;
// A is the launch's argument block (spill, spill_stride and, for StackEntry, spill_tmin).  THE one statement of "entry i": every
// guarded push and every pop of every walk goes through load / store.
// (The block's LDS array is an argument of load / store, not a member: a pointer to LDS held in a struct reaches the code
// generator as a generic pointer, and the pop becomes a flat load whose address is selected between LDS and global memory.)
struct StackRef { // a bare node reference (the binary walk, binary_walk_dev.h: k_traverse, k_traverse_multihit, k_traverse_motion)
  typedef uint32_t type;
  static constexpr bool kHasTmin = false;
};
template <typename SE, int STACK, typename A>
struct LaneStack {
  typedef typename SE::type Entry;
  const A &a;
  unsigned col, gcol;
  // where entry i >= STACK lies in the overflow arrays
  __device__ __forceinline__ size_t spill_at(int i) const { return (size_t)(i - STACK) * a.spill_stride + gcol; }
  // Entry i >= 0.  The LDS read is unconditional (of the last LDS entry when i lies beyond); the rare entry in the overflow arrays
  // replaces it.  `live` false: the caller will not use the value (its stack is empty) and nothing beyond LDS is read.
  __device__ __forceinline__ void load(const Entry (&lds)[STACK][kTraverseBlock], int i, Entry &e, bool live = true) const {
    e = lds[i > STACK - 1 ? STACK - 1 : i][col];
    if (live && i >= STACK) {
      const size_t o = spill_at(i);
      if constexpr (SE::kHasTmin)
        e = SE::make(a.spill[o], a.spill_tmin[o]);
      else
        e = a.spill[o];
    }
  }
  // (StackRef entries; a StackEntry is stored by walk_dev.h's NRT_STACK_STORE, which says why it is a macro)
  __device__ __forceinline__ void store(Entry (&lds)[STACK][kTraverseBlock], int i, uint32_t ref) const {
    if (i < STACK) {
      lds[i][col] = ref;
    } else {
      a.spill[spill_at(i)] = ref;
    }
  }
};

// Lane states of the while-while loop (binary_walk_dev.h).
enum : int { LANE_IDLE = 0, LANE_TRAV = 1, LANE_LEAF = 2 };

// The host side of every persistent launch of the walks: the kernel is picked once, as a pointer, and the launch and the
// occupancy query that sizes its grid go through that pointer.
template <typename A>
static void launch_persistent(const void *kernel, unsigned grid, const A &args, hipStream_t s) {
  void *params[] = {(void *)&args};
  (void)hipLaunchKernel(kernel, dim3(grid), dim3(kTraverseBlock), params, 0, s); // (the callers return hipGetLastError())
}
// Resident blocks per CU of `kernel`, 8 at the most; `fallback` where the runtime cannot say.
static int resident_blocks(const void *kernel, int fallback) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, kTraverseBlock, 0) != hipSuccess || n < 1) n = fallback;
  return n > 8 ? 8 : n;
}

} // namespace nrt

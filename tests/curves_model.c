/* tests/curves_model.c — TEST INFRASTRUCTURE: the CPU model of the curve primitive (include/nanort_hip.h, nrtSetCurves_f32 /
 * nrtTraverseBatchCurves*_f32): a plain-C restatement of the arithmetic of the reference's curve example
 * (examples/curves_primitive/main.cc: GetZAlign, Xform, EvaluateBezier, EvaluateBezierTangent, CurveIntersector) under
 * BVHAccel::Traverse's binary loop (nanort.h:2487-2556), in the reference's own evaluation order.  Deliberately literal: both
 * ends of every segment are evaluated, the frame is computed per (ray, curve) — the GPU kernel shares and hoists; the bits
 * must not care.  Compile with -ffp-contract=off -fno-fast-math.
 *
 *   cvm_traverse   rays x Traverse over a given node / index array -> 40-byte records + 0/1 mask
 *   cvm_boxes      the example's per-curve box and SAH position (BoundingBoxAndCenter)
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef struct {
  float bmin[3], bmax[3];
  int32_t flag, axis;
  uint32_t data[2];
} cvm_node;
typedef struct {
  float org[3], dir[3], min_t, max_t;
  uint32_t type;
} cvm_ray;
typedef struct {
  float t;
  uint32_t prim_id;
  float u, v, tangent[3], normal[3];
} cvm_hit;

static float cvm_safe_inv(float v) {
  if (fabsf(v) < FLT_EPSILON) return INFINITY * ((v < 0.0f) ? -1.0f : 1.0f);
  return 1.0f / v;
}

static int cvm_slab(float min_t, float max_t, const float bmin[3], const float bmax[3], const float org[3], const float inv[3],
                    const int sign[3]) {
  float tmn[3], tmx[3], tmin, tmax;
  int k;
  for (k = 0; k < 3; k++) {
    const float mn = sign[k] ? bmax[k] : bmin[k], mx = sign[k] ? bmin[k] : bmax[k];
    tmn[k] = (mn - org[k]) * inv[k];
    tmx[k] = (mx - org[k]) * inv[k] * 1.00000024f;
  }
  tmin = (tmn[0] > min_t) ? tmn[0] : min_t;
  tmin = (tmn[1] > tmin) ? tmn[1] : tmin;
  tmin = (tmn[2] > tmin) ? tmn[2] : tmin;
  tmax = (tmx[0] < max_t) ? tmx[0] : max_t;
  tmax = (tmx[1] < tmax) ? tmx[1] : tmax;
  tmax = (tmx[2] < tmax) ? tmx[2] : tmax;
  return tmin <= tmax;
}

static void cvm_zalign(const float o[3], const float l[3], float m[3][3], float tr[3]) {
  const float dxz = sqrtf(l[0] * l[0] + l[2] * l[2]);
  if (dxz > 0) {
    const float lxdxz = l[0] / dxz, lydxz = l[1] / dxz, lzdxz = l[2] / dxz;
    m[0][0] = lzdxz;
    m[0][1] = -lxdxz * l[1];
    m[0][2] = l[0];
    m[1][0] = 0;
    m[1][1] = dxz;
    m[1][2] = l[1];
    m[2][0] = -lxdxz;
    m[2][1] = -lydxz * l[2];
    m[2][2] = l[2];
  } else {
    m[0][0] = 1;
    m[0][1] = 0;
    m[0][2] = 0;
    m[1][0] = 0;
    m[1][1] = 0;
    m[1][2] = (l[1] > 0) ? -1 : 1;
    m[2][0] = 0;
    m[2][1] = (l[1] > 0) ? 1 : -1;
    m[2][2] = 0;
  }
  tr[0] = -(o[0] * m[0][0] + o[1] * m[1][0] + o[2] * m[2][0]);
  tr[1] = -(o[0] * m[0][1] + o[1] * m[1][1] + o[2] * m[2][1]);
  tr[2] = -(o[0] * m[0][2] + o[1] * m[1][2] + o[2] * m[2][2]);
}

static void cvm_xform(const float p[3], float m[3][3], const float tr[3], float q[3]) {
  q[0] = p[0] * m[0][0] + p[1] * m[1][0] + p[2] * m[2][0] + tr[0];
  q[1] = p[0] * m[0][1] + p[1] * m[1][1] + p[2] * m[2][1] + tr[1];
  q[2] = p[0] * m[0][2] + p[1] * m[1][2] + p[2] * m[2][2] + tr[2];
}

static void cvm_bezier(float v[4][3], float t, float p[3]) {
  const float u = 1 - t;
  int k;
  for (k = 0; k < 3; k++) {
    const float a0 = v[0][k] * u + v[1][k] * t, a1 = v[1][k] * u + v[2][k] * t, a2 = v[2][k] * u + v[3][k] * t;
    const float b0 = a0 * u + a1 * t, b1 = a1 * u + a2 * t;
    p[k] = b0 * u + b1 * t;
  }
}

typedef struct { /* the intersector's mutable members */
  float t, u, v, u_param, v_param;
  uint32_t prim;
} cvm_state;

/* CurveIntersector::Intersect: 1 and *t lowered when a segment is accepted */
static int cvm_intersect(const float *cps, const float *radii, int n, const float org[3], const float dir[3], const uint32_t range[2],
                         cvm_state *st, float *t_inout, uint32_t prim) {
  float R[3][3], T[3], c[4][3], radius[2], t_z = 0.0f, uw, inv_n;
  int i, s, has_hit = 0;
  if (prim < range[0] || prim >= range[1]) return 0;
  cvm_zalign(org, dir, R, T);
  radius[0] = radii[4 * (size_t)prim + 0];
  radius[1] = radii[4 * (size_t)prim + 3];
  for (i = 0; i < 4; i++) {
    cvm_xform(cps + 12 * (size_t)prim + 3 * i, R, T, c[i]);
    if (t_z < c[i][2]) t_z = c[i][2];
  }
  uw = ((radius[0] < radius[1]) ? radius[1] : radius[0]) / 2.0f;
  if (t_z < 4.0f * uw) return 0;
  inv_n = 1.0f / (float)n;
  for (s = 0; s < n; s++) {
    float p0[3], p1[3], P0w, P1w, Ax, Ay, Bx, By, Bz, Bw, d0, d1, u, Px, Py, Pz, Pw, t, r2, d2;
    const float t0 = s / (float)n, t1 = (s + 1) / (float)n;
    cvm_bezier(c, t0, p0);
    cvm_bezier(c, t1, p1);
    P0w = (float)(0.5 * radius[0]);
    P1w = (float)(0.5 * radius[1]);
    Ax = 0.0f - p0[0];
    Ay = 0.0f - p0[1];
    Bx = p1[0] - p0[0];
    By = p1[1] - p0[1];
    Bz = p1[2] - p0[2];
    Bw = P1w - P0w;
    d0 = (Ax * Bx) + (Ay * By);
    d1 = (Bx * Bx) + (By * By);
    u = d0 / d1;
    u = (u < 1.0f) ? u : 1.0f; /* std::min(1.0f, u) */
    u = (0.0f < u) ? u : 0.0f; /* std::max(0.0f, .) */
    Px = p0[0] + (u * Bx);
    Py = p0[1] + (u * By);
    Pz = p0[2] + (u * Bz);
    Pw = P0w + (u * Bw);
    t = Pz;
    r2 = Pw * Pw;
    d2 = (Px * Px) + (Py * Py);
    if ((d2 <= r2) && (t < (*t_inout))) {
      st->u_param = (u + (float)s) * inv_n;
      st->v_param = sqrtf(d2);
      *t_inout = t;
      has_hit = 1;
    }
  }
  return has_hit;
}

static void cvm_normalize(float v[3]) { /* vnormalize, nanort.h:388-398 */
  const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (fabsf(len) > FLT_EPSILON) {
    const float inv_len = 1.0f / len;
    v[0] *= inv_len;
    v[1] *= inv_len;
    v[2] *= inv_len;
  }
}
static void cvm_cross(const float a[3], const float b[3], float c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

static int cvm_one(const cvm_node *nodes, const uint32_t *indices, const float *cps, const float *radii, int n, const cvm_ray *ray,
                   const uint32_t range[2], cvm_hit *out) {
  uint32_t stack[512];
  int sp = 0, sign[3], k, hit;
  float inv[3], hit_t = ray->max_t;
  cvm_state st;
  memset(&st, 0, sizeof(st));
  st.t = hit_t; /* Traverse: intersector.Update(ray.max_t, -1) */
  st.prim = 0xFFFFFFFFu;
  stack[0] = 0;
  for (k = 0; k < 3; k++) {
    sign[k] = ray->dir[k] < 0.0f ? 1 : 0;
    inv[k] = cvm_safe_inv(ray->dir[k]);
  }
  while (sp >= 0) {
    const cvm_node *node = &nodes[stack[sp]];
    sp--;
    if (!cvm_slab(ray->min_t, hit_t, node->bmin, node->bmax, ray->org, inv, sign)) continue;
    if (node->flag == 0) {
      const int near = sign[node->axis];
      stack[++sp] = node->data[1 - near];
      stack[++sp] = node->data[near];
    } else { /* TestLeafNode */
      uint32_t i;
      float t = st.t;
      int any = 0;
      for (i = 0; i < node->data[0]; i++) {
        const uint32_t prim = indices[node->data[1] + i];
        float local_t = t;
        if (cvm_intersect(cps, radii, n, ray->org, ray->dir, range, &st, &local_t, prim)) {
          t = local_t;
          st.t = t; /* Update */
          st.prim = prim;
          st.u = st.u_param;
          st.v = st.v_param;
          any = 1;
        }
      }
      if (any) hit_t = st.t;
    }
  }
  hit = st.t < ray->max_t;
  memset(out, 0, sizeof(*out));
  if (hit) { /* PostTraversal */
    const float *v = cps + 12 * (size_t)st.prim;
    float dv[3], c1[3], c2[3];
    for (k = 0; k < 3; k++) {
      const float C1 = v[9 + k] - (3.0f * v[6 + k]) + (3.0f * v[3 + k]) - v[k];
      const float C2 = (3.0f * v[6 + k]) - (6.0f * v[3 + k]) + (3.0f * v[k]);
      const float C3 = (3.0f * v[3 + k]) - (3.0f * v[k]);
      dv[k] = (3.0f * C1 * st.u * st.u) + (2.0f * C2 * st.u) + C3;
    }
    cvm_normalize(dv);
    cvm_cross(ray->dir, dv, c1);
    cvm_cross(c1, dv, c2);
    cvm_normalize(c2);
    out->t = st.t;
    out->prim_id = st.prim;
    out->u = st.u;
    out->v = st.v;
    memcpy(out->tangent, dv, sizeof(dv));
    memcpy(out->normal, c2, sizeof(c2));
  } else {
    out->t = ray->max_t;
    out->prim_id = 0xFFFFFFFFu;
  }
  return hit;
}

void cvm_traverse(const void *nodes, const uint32_t *indices, const float *cps, const float *radii, int num_subdivisions, const void *rays,
                  uint64_t num_rays, const uint32_t *range, void *hits, uint8_t *mask) {
  static const uint32_t all[2] = {0u, 0x7FFFFFFFu};
  uint64_t i;
  for (i = 0; i < num_rays; i++)
    mask[i] = (uint8_t)cvm_one((const cvm_node *)nodes, indices, cps, radii, num_subdivisions, (const cvm_ray *)rays + i, range ? range : all,
                               (cvm_hit *)hits + i);
}

/* CurveGeometry::BoundingBoxAndCenter: bmin / bmax / centre, 3 floats each per curve */
void cvm_boxes(const float *cps, const float *radii, uint32_t n, float *bmin, float *bmax, float *center) {
  uint32_t p;
  int i, k;
  for (p = 0; p < n; p++) {
    const float *v = cps + 12 * (size_t)p, *r = radii + 4 * (size_t)p;
    for (k = 0; k < 3; k++) {
      float lo = v[k] - r[0], hi = v[k] + r[0];
      for (i = 1; i < 4; i++) {
        const float a = v[3 * i + k] - r[i], b = v[3 * i + k] + r[i];
        lo = (lo < a) ? lo : a; /* std::min(a, lo) */
        hi = (b < hi) ? hi : b; /* std::max(b, hi) */
      }
      bmin[3 * (size_t)p + k] = lo;
      bmax[3 * (size_t)p + k] = hi;
      center[3 * (size_t)p + k] = (v[k] + v[3 + k] + v[6 + k] + v[9 + k]) / 4.0f;
    }
  }
}

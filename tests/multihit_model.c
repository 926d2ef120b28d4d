/* tests/multihit_model.c — TEST INFRASTRUCTURE: the CPU model of multi-hit traversal (include/nanort_hip.h,
 * nrtMultiHitTraverseBatch*), over the oracle's plain-C restatement of the reference's slab and triangle tests
 * (oracle/nanort_oracle_body.inc, included here per precision exactly as oracle/nanort_oracle.c does; compiled with
 * -I oracle).
 *
 *   mh_traverse_*  the contract's walk: the binary loop over a node array (pop, slab test on [min_t, B], near child first),
 *                  B = max_t while fewer than K hits are held, else the t of the worst held hit; a candidate (accepted
 *                  against B, t < max_t) enters when fewer than K are held or its (t, prim_id) key is below the worst;
 *                  the row is kept sorted by insertion, the worst held hit dropped.
 *   mh_brute_*     every primitive against B = max_t, candidates sorted by key, the first K kept.
 * Output as the library's: hits[ray * K + j] (sorted hits, then miss records {0, 0, max_t, 0xFFFFFFFF}), counts[ray].
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MH_PRECISION_BODY                                                                                              \
  static int FN(key_greater)(REAL t, uint32_t p, REAL bt, uint32_t bp) { return t > bt || (t == bt && p > bp); }     \
                                                                                                                       \
  /* candidate (t, u, v, prim) into the sorted row of `*held` hits; returns the new bound */                          \
  static REAL FN(mh_insert)(FN(orc_hit) * row, uint32_t K, uint32_t *held, REAL t, REAL u, REAL v, uint32_t prim,       \
                            REAL max_t) {                                                                              \
    uint32_t j = *held < K ? *held : K - 1u;                                                                           \
    while (j > 0u && FN(key_greater)(row[j - 1u].t, row[j - 1u].prim_id, t, prim)) {                                   \
      row[j] = row[j - 1u];                                                                                            \
      j--;                                                                                                             \
    }                                                                                                                  \
    row[j].u = u;                                                                                                      \
    row[j].v = v;                                                                                                      \
    row[j].t = t;                                                                                                      \
    row[j].prim_id = prim;                                                                                             \
    if (*held < K) (*held)++;                                                                                          \
    return *held == K ? row[K - 1u].t : max_t;                                                                         \
  }                                                                                                                    \
                                                                                                                       \
  static void FN(mh_finish)(FN(orc_hit) * row, uint32_t K, uint32_t held, REAL max_t) {                                \
    uint32_t j;                                                                                                        \
    for (j = held; j < K; j++) {                                                                                       \
      memset(&row[j], 0, sizeof(row[j]));                                                                              \
      row[j].t = max_t;                                                                                                \
      row[j].prim_id = 0xFFFFFFFFu;                                                                                    \
    }                                                                                                                  \
  }                                                                                                                    \
                                                                                                                       \
  static uint32_t FN(mh_one)(const FN(orc_node) * nodes, const uint32_t *indices, const FN(orc_mesh) * m,             \
                             const FN(orc_ray) * ray, const uint32_t opt[4], uint32_t K, FN(orc_hit) * row) {          \
    FN(orc_isector) s;                                                                                                 \
    uint32_t stack[512], held = 0, worst_prim = 0xFFFFFFFFu;                                                           \
    int sp = 0, sign[3], k;                                                                                            \
    REAL inv[3], B = ray->max_t;                                                                                       \
    stack[0] = 0;                                                                                                      \
    FN(prepare)(&s, ray, opt);                                                                                         \
    for (k = 0; k < 3; k++) {                                                                                          \
      sign[k] = ray->dir[k] < (REAL)0.0 ? 1 : 0;                                                                       \
      inv[k] = FN(safe_inv)(ray->dir[k]);                                                                              \
    }                                                                                                                  \
    while (sp >= 0) {                                                                                                  \
      const FN(orc_node) *node = &nodes[stack[sp]];                                                                    \
      sp--;                                                                                                            \
      if (!FN(slab)(ray->min_t, B, node->bmin, node->bmax, ray->org, inv, sign)) continue;                             \
      if (node->flag == 0) {                                                                                           \
        int near = sign[node->axis];                                                                                   \
        stack[++sp] = node->data[1 - near];                                                                            \
        stack[++sp] = node->data[near];                                                                                \
      } else {                                                                                                         \
        uint32_t i;                                                                                                    \
        for (i = 0; i < node->data[0]; i++) {                                                                          \
          uint32_t prim = indices[node->data[1] + i];                                                                  \
          REAL t = B;                                                                                                  \
          if (!FN(intersect)(&s, m, &t, prim)) continue;                                                               \
          if (!(t < ray->max_t)) continue; /* (NaN too) */                                                             \
          if (held == K && !(t < B || prim < worst_prim)) continue; /* accepted: t <= B */                            \
          B = FN(mh_insert)(row, K, &held, t, s.u, s.v, prim, ray->max_t);                                             \
          worst_prim = row[held - 1u].prim_id;                                                                         \
        }                                                                                                              \
      }                                                                                                                \
    }                                                                                                                  \
    FN(mh_finish)(row, K, held, ray->max_t);                                                                           \
    return held;                                                                                                       \
  }                                                                                                                    \
                                                                                                                       \
  void FN(mh_traverse)(const void *nodes, const uint32_t *indices, const void *verts, size_t stride,                    \
                       const uint32_t *faces, const void *rays, uint64_t n, const uint32_t *trace_opt, uint32_t K,     \
                       void *hits, uint32_t *counts) {                                                                 \
    static const uint32_t defaults[4] = {0u, 0x7FFFFFFFu, 0xFFFFFFFFu, 0u};                                            \
    const uint32_t *opt = trace_opt ? trace_opt : defaults;                                                            \
    FN(orc_mesh) mesh;                                                                                                 \
    uint64_t i;                                                                                                        \
    mesh.verts = (const unsigned char *)verts;                                                                         \
    mesh.stride = stride;                                                                                              \
    mesh.faces = faces;                                                                                                \
    for (i = 0; i < n; i++)                                                                                            \
      counts[i] = FN(mh_one)((const FN(orc_node) *)nodes, indices, &mesh, (const FN(orc_ray) *)rays + i, opt, K,      \
                             (FN(orc_hit) *)hits + i * K);                                                             \
  }                                                                                                                    \
                                                                                                                       \
  void FN(mh_brute)(uint32_t num_faces, const void *verts, size_t stride, const uint32_t *faces, const void *rays,     \
                    uint64_t n, const uint32_t *trace_opt, uint32_t K, void *hits, uint32_t *counts) {                 \
    static const uint32_t defaults[4] = {0u, 0x7FFFFFFFu, 0xFFFFFFFFu, 0u};                                            \
    const uint32_t *opt = trace_opt ? trace_opt : defaults;                                                            \
    FN(orc_mesh) mesh;                                                                                                 \
    uint64_t i;                                                                                                        \
    uint32_t prim;                                                                                                     \
    mesh.verts = (const unsigned char *)verts;                                                                         \
    mesh.stride = stride;                                                                                              \
    mesh.faces = faces;                                                                                                \
    for (i = 0; i < n; i++) {                                                                                          \
      const FN(orc_ray) *ray = (const FN(orc_ray) *)rays + i;                                                          \
      FN(orc_hit) *row = (FN(orc_hit) *)hits + i * K;                                                                  \
      FN(orc_isector) s;                                                                                               \
      uint32_t held = 0;                                                                                               \
      FN(prepare)(&s, ray, opt);                                                                                       \
      for (prim = 0; prim < num_faces; prim++) {                                                                       \
        REAL t = ray->max_t;                                                                                           \
        if (!FN(intersect)(&s, &mesh, &t, prim) || !(t < ray->max_t)) continue;                                        \
        /* a full row keeps the K smallest keys seen so far: enter only below the worst */                             \
        if (held == K && !FN(key_greater)(row[K - 1u].t, row[K - 1u].prim_id, t, prim)) continue;                      \
        (void)FN(mh_insert)(row, K, &held, t, s.u, s.v, prim, ray->max_t);                                             \
      }                                                                                                                \
      FN(mh_finish)(row, K, held, ray->max_t);                                                                         \
      counts[i] = held;                                                                                                \
    }                                                                                                                  \
  }

#define REAL float
#define SUF f32
#define REAL_EPS FLT_EPSILON
#define REAL_MAX FLT_MAX
#define REAL_INF ((float)INFINITY)
#define MAXMULT 1.00000024f
#define FABS fabsf
#include "nanort_oracle_body.inc"
#define CAT2(a, b) a##_##b
#define CAT(a, b) CAT2(a, b)
#define FN(name) CAT(name, SUF)
MH_PRECISION_BODY
#undef FN
#undef CAT
#undef CAT2
#undef REAL
#undef SUF
#undef REAL_EPS
#undef REAL_MAX
#undef REAL_INF
#undef MAXMULT
#undef FABS

#define REAL double
#define SUF f64
#define REAL_EPS DBL_EPSILON
#define REAL_MAX DBL_MAX
#define REAL_INF ((double)INFINITY)
#define MAXMULT 1.0000000000000004
#define FABS fabs
#include "nanort_oracle_body.inc"
#define CAT2(a, b) a##_##b
#define CAT(a, b) CAT2(a, b)
#define FN(name) CAT(name, SUF)
MH_PRECISION_BODY

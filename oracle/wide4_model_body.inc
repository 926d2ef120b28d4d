/* oracle/wide4_model_body.inc — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A sequential MODEL of the traversal kernel's two-levels-per-step walk (nanort_amd/csrc/walk_dev.h,
 * NRT_STEP_NODE4 / NRT_POP_ENTRY; DESIGN.md §3.1), used by tests/test_wide4_model.py to check, on the CPU and on
 * hostile inputs, that it visits the same leaves in the same order as the restated reference loop above
 * (nanort.h:2526-2548):
 *
 *   A step at branch node X tests the boxes of X's (up to) four GRANDCHILDREN at once — slots 0,1 the children of
 *   X.data[0], slots 2,3 those of X.data[1]; a child that is a leaf is tested itself in the first slot of its half —
 *   with the hit distance of that moment, ranks the slots as the binary loop would reach them (near half by X's
 *   axis, inside a half the near slot by the child's axis), enters the first hit and pushes the others, each with
 *   its entry distance, in reverse rank order.  A popped entry is entered iff its entry distance still beats the
 *   hit distance.  The child's own box is never tested: on a tree whose child boxes lie inside their parents' it
 *   is implied by the grandchild's (monotone slab arithmetic).
 *
 * Every visited leaf is appended to `trail` (when given) so that the test can compare SEQUENCES, not just records;
 * `counters` = {steps, leaves tested, triangle tests, max stack depth}.
 */

/* slab test that also returns the entry distance (the running maximum, as IntersectRayAABB computes it, nanort.h:2285-2370) */
static inline int FN(slab_tmin)(REAL min_t, REAL max_t, const REAL bmin[3], const REAL bmax[3], const REAL org[3],
                                const REAL inv[3], const int sign[3], REAL *tmin_out) {
  REAL mn[3], mx[3], tmn[3], tmx[3], tmin, tmax;
  int k;
  for (k = 0; k < 3; k++) {
    mn[k] = sign[k] ? bmax[k] : bmin[k];
    mx[k] = sign[k] ? bmin[k] : bmax[k];
    tmn[k] = (mn[k] - org[k]) * inv[k];
    tmx[k] = (mx[k] - org[k]) * inv[k] * MAXMULT;
  }
  tmin = (tmn[0] > min_t) ? tmn[0] : min_t;
  tmin = (tmn[1] > tmin) ? tmn[1] : tmin;
  tmin = (tmn[2] > tmin) ? tmn[2] : tmin;
  tmax = (tmx[0] < max_t) ? tmx[0] : max_t;
  tmax = (tmx[1] < tmax) ? tmx[1] : tmax;
  tmax = (tmx[2] < tmax) ? tmx[2] : tmax;
  *tmin_out = tmin;
  return tmin <= tmax;
}

typedef struct {
  uint32_t node;
  REAL tmin;
} FN(w4_entry);

static int FN(traverse_one_wide4)(const FN(orc_node) * nodes, const uint32_t *indices, const FN(orc_mesh) * m,
                                  const FN(orc_ray) * ray, const uint32_t opt[4], FN(orc_hit) * out,
                                  uint64_t *counters, uint32_t *trail, uint64_t trail_cap, uint64_t *trail_len) {
  FN(orc_isector) s;
  FN(w4_entry) stack[1024];
  int sp = 0, sign[3], k, hit;
  REAL inv[3], hit_t = ray->max_t;
  uint64_t c_steps = 0, c_leaves = 0, c_tris = 0, c_stack = 0;
  uint32_t cur = 0;
  int have = 1; /* a node to enter */

  s.t = hit_t;
  s.prim = 0xFFFFFFFFu;
  FN(prepare)(&s, ray, opt);
  for (k = 0; k < 3; k++) {
    sign[k] = ray->dir[k] < (REAL)0.0 ? 1 : 0;
    inv[k] = FN(safe_inv)(ray->dir[k]);
  }
  /* node 0: a leaf root is tested as the reference does; a branch root is entered without its own test (a ray that
   * misses it misses every grandchild: the first step then ends in an empty stack) */
  if (nodes[0].flag != 0) {
    REAL t0;
    have = FN(slab_tmin)(ray->min_t, hit_t, nodes[0].bmin, nodes[0].bmax, ray->org, inv, sign, &t0);
  }
  for (;;) {
    if (!have) { /* pop */
      if (sp == 0) break;
      sp--;
      if (!(stack[sp].tmin <= hit_t)) continue;
      cur = stack[sp].node;
    }
    have = 0;
    if (nodes[cur].flag != 0) { /* leaf: TestLeafNode, nanort.h:2374-2407 */
      uint32_t i, cnt = nodes[cur].data[0], off = nodes[cur].data[1];
      REAL t = s.t;
      int any = 0;
      c_leaves++;
      if (trail && *trail_len < trail_cap) trail[*trail_len] = cur;
      if (trail_len) (*trail_len)++;
      for (i = 0; i < cnt; i++) {
        uint32_t prim = indices[off + i];
        REAL local_t = t;
        c_tris++;
        if (FN(intersect)(&s, m, &local_t, prim)) {
          t = local_t;
          s.t = t;
          s.prim = prim;
          any = 1;
        }
      }
      if (any) hit_t = s.t;
      continue;
    }
    { /* one step over the four grandchild slots of branch `cur` */
      const FN(orc_node) *X = &nodes[cur];
      uint32_t slot_node[4];
      int slot_valid[4], slot_hit[4], rank_slot[4], h, j, r, first = -1, half_near[2];
      REAL slot_tmin[4];
      c_steps++;
      for (h = 0; h < 2; h++) {
        const uint32_t ci = X->data[h];
        const FN(orc_node) *ch = &nodes[ci];
        if (ch->flag == 0) {
          slot_node[2 * h] = ch->data[0];
          slot_node[2 * h + 1] = ch->data[1];
          slot_valid[2 * h] = slot_valid[2 * h + 1] = 1;
          half_near[h] = sign[ch->axis];
        } else {
          slot_node[2 * h] = ci;
          slot_node[2 * h + 1] = 0;
          slot_valid[2 * h] = 1;
          slot_valid[2 * h + 1] = 0;
          half_near[h] = 0;
        }
      }
      for (j = 0; j < 4; j++) {
        slot_hit[j] = 0;
        slot_tmin[j] = 0;
        if (slot_valid[j])
          slot_hit[j] = FN(slab_tmin)(ray->min_t, hit_t, nodes[slot_node[j]].bmin, nodes[slot_node[j]].bmax, ray->org,
                                      inv, sign, &slot_tmin[j]);
      }
      { /* visiting order: near half by X's axis, inside a half the near slot by the child's axis */
        const int hn = sign[X->axis], hf = 1 - hn;
        rank_slot[0] = 2 * hn + half_near[hn];
        rank_slot[1] = 2 * hn + (1 - half_near[hn]);
        rank_slot[2] = 2 * hf + half_near[hf];
        rank_slot[3] = 2 * hf + (1 - half_near[hf]);
      }
      for (r = 0; r < 4; r++)
        if (slot_hit[rank_slot[r]]) {
          first = r;
          break;
        }
      if (first < 0) continue; /* nothing hit: pop */
      for (r = 3; r > first; r--)
        if (slot_hit[rank_slot[r]]) {
          stack[sp].node = slot_node[rank_slot[r]];
          stack[sp].tmin = slot_tmin[rank_slot[r]];
          sp++;
          if ((uint64_t)sp > c_stack) c_stack = (uint64_t)sp;
        }
      cur = slot_node[rank_slot[first]];
      have = 1;
    }
  }
  hit = s.t < ray->max_t;
  if (hit) {
    out->t = s.t;
    out->u = s.u;
    out->v = s.v;
    out->prim_id = s.prim;
  } else {
    out->t = ray->max_t;
    out->u = 0;
    out->v = 0;
    out->prim_id = 0xFFFFFFFFu;
  }
  if (counters) {
    counters[0] += c_steps;
    counters[1] += c_leaves;
    counters[2] += c_tris;
    if (c_stack > counters[3]) counters[3] = c_stack;
  }
  return hit;
}

/* The reference loop's own leaf sequence, for the comparison (same walk as traverse_one above, recording leaves). */
static void FN(leaf_trail_reference)(const FN(orc_node) * nodes, const uint32_t *indices, const FN(orc_mesh) * m,
                                     const FN(orc_ray) * ray, const uint32_t opt[4], uint32_t *trail, uint64_t trail_cap,
                                     uint64_t *trail_len) {
  FN(orc_isector) s;
  uint32_t stack[512];
  int sp = 0, sign[3], k;
  REAL inv[3], hit_t = ray->max_t;
  stack[0] = 0;
  s.t = hit_t;
  s.prim = 0xFFFFFFFFu;
  FN(prepare)(&s, ray, opt);
  for (k = 0; k < 3; k++) {
    sign[k] = ray->dir[k] < (REAL)0.0 ? 1 : 0;
    inv[k] = FN(safe_inv)(ray->dir[k]);
  }
  while (sp >= 0) {
    const uint32_t ni = stack[sp];
    const FN(orc_node) *node = &nodes[ni];
    sp--;
    if (FN(slab)(ray->min_t, hit_t, node->bmin, node->bmax, ray->org, inv, sign)) {
      if (node->flag == 0) {
        int near = sign[node->axis];
        stack[++sp] = node->data[1 - near];
        stack[++sp] = node->data[near];
      } else {
        uint32_t i, cnt = node->data[0], off = node->data[1];
        REAL t = s.t;
        int any = 0;
        if (*trail_len < trail_cap) trail[*trail_len] = ni;
        (*trail_len)++;
        for (i = 0; i < cnt; i++) {
          uint32_t prim = indices[off + i];
          REAL local_t = t;
          if (FN(intersect)(&s, m, &local_t, prim)) {
            t = local_t;
            s.t = t;
            s.prim = prim;
            any = 1;
          }
        }
        if (any) hit_t = s.t;
      }
    }
  }
}

/* Batched driver.  trail_ref / trail_w4 (optional, each `trail_cap` entries) receive the concatenated leaf sequences of
 * all rays as visited by the reference loop / by the two-level walk; trail_len[0..1] their total lengths. */
void FN(orc_traverse_wide4_model)(const void *nodes, const uint32_t *indices, const void *verts, size_t stride,
                                  const uint32_t *faces, const void *rays, uint64_t n, const uint32_t *trace_opt,
                                  void *hits, uint8_t *mask, uint64_t *counters, uint32_t *trail_ref, uint32_t *trail_w4,
                                  uint64_t trail_cap, uint64_t *trail_len) {
  static const uint32_t defaults[4] = {0u, 0x7FFFFFFFu, 0xFFFFFFFFu, 0u};
  const uint32_t *opt = trace_opt ? trace_opt : defaults;
  FN(orc_mesh) mesh;
  uint64_t i, len_ref = 0, len_w4 = 0;
  mesh.verts = (const unsigned char *)verts;
  mesh.stride = stride;
  mesh.faces = faces;
  for (i = 0; i < n; i++) {
    const FN(orc_ray) *ray = (const FN(orc_ray) *)rays + i;
    int h = FN(traverse_one_wide4)((const FN(orc_node) *)nodes, indices, &mesh, ray, opt, (FN(orc_hit) *)hits + i, counters,
                                   trail_w4, trail_cap, &len_w4);
    if (trail_ref) FN(leaf_trail_reference)((const FN(orc_node) *)nodes, indices, &mesh, ray, opt, trail_ref, trail_cap, &len_ref);
    if (mask) mask[i] = (uint8_t)h;
  }
  if (trail_len) {
    trail_len[0] = len_ref;
    trail_len[1] = len_w4;
  }
}

"""Per-ray skip (node, primitive) pairs on scenes (nrtSceneQueryBatch*, Scene.QueryBatch*): what such a query must return, stated
with the restatement alone (oracle/nanosg_oracle.c through oracle.bindings.SceneOracle), and the waves the tests trace.

The rule: the query answers exactly as the unskipped query, except that in the per-node Traverse of node n the trace options carry
skip_prim_id = p for a ray whose pair is (p, n): the intersector returns false for that one primitive of that one instance without
touching the ray's state.  The restatement has no skip id, but its intersector rejects a triangle whose three vertices coincide
(det == 0) at the same place, before anything of the ray is touched.  So, per distinct pair (p, n): node n's `faces` pointer is
aimed at a copy in which face p is collapsed onto its first vertex, the rays that carry the pair are traced, and the pointer is put
back.  Node boxes and trees do not depend on the faces, so nothing is committed again.  With MASKED, one committed SceneOracle per
distinct ray word over the visible nodes, as scene_masks_fixture.expect_masked builds them, and the skip on top."""
import numpy as np

from nanort_amd.wire import RAY_F32
from oracle import bindings as ob
from scene_masks_fixture import ALL, MAX_WORDS, miss_records

INVALID_PAIR = np.array([ALL, ALL], dtype=np.uint32)


def pairs_of(hits):
    """The (n, 2) uint32 pairs {prim_id, node_id} of a wave's records: what the next wave skips."""
    return np.ascontiguousarray(np.stack([hits["prim_id"], hits["node_id"]], axis=1).astype(np.uint32))


def _trace_with_pairs(O, kept, faces_of, rays, pairs):
    """Rays through the committed SceneOracle `O` of the nodes `kept` (ids in the whole scene), each with its pair."""
    n = rays.shape[0]
    hits = miss_records(rays)
    flags = np.zeros(n, dtype=np.uint8)
    local = {int(k): j for j, k in enumerate(kept)}
    prim, node = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    nfaces = np.array([faces_of[int(k)].shape[0] for k in kept], dtype=np.int64)
    slot = np.array([local.get(int(x), -1) for x in node], dtype=np.int64)  # hidden or out of range: skips nothing
    valid = (slot >= 0) & (prim != ALL)
    valid[valid] &= prim[valid] < nfaces[slot[valid]]
    plain = np.nonzero(~valid)[0]
    if len(plain):
        hits[plain], flags[plain] = O.traverse(rays[plain])
    if valid.any():
        key = slot * (1 << 32) + prim
        order = np.nonzero(valid)[0]
        order = order[np.argsort(key[order], kind="stable")]
        cuts = np.nonzero(np.diff(key[order]))[0] + 1
        for sel in np.split(order, cuts):
            j, p = int(slot[sel[0]]), int(prim[sel[0]])
            faces = faces_of[int(kept[j])].copy()
            faces[p, :] = faces[p, 0]
            saved = O.arr[j].faces
            O.arr[j].faces = faces.ctypes.data
            try:
                hits[sel], flags[sel] = O.traverse(rays[sel])
            finally:
                O.arr[j].faces = saved
    return hits, flags


def expect_query(oracle, nodes, rays, pairs=None, node_masks=None, ray_words=None, committed=None):
    """(hits, flags) a query must return.  `nodes`: scene_masks_fixture.scene_nodes(...) of the whole scene, or such a list;
    `pairs`: (n, 2) uint32 {prim_id, node_id} or None (no SKIP); `node_masks` / `ray_words`: None = the query is not MASKED.
    `committed`: a committed SceneOracle of ALL the nodes, reused for the unmasked case."""
    n = rays.shape[0]
    pairs = np.tile(INVALID_PAIR, (n, 1)) if pairs is None else np.asarray(pairs, dtype=np.uint32)
    assert pairs.shape == (n, 2)
    faces_of = [np.ascontiguousarray(f, dtype=np.uint32) for _, f, _, _ in nodes]
    if node_masks is None and ray_words is None:
        O = committed
        if O is None:
            O = ob.SceneOracle(oracle)
            for v, f, x, tree in nodes:
                O.add_node(v, f, x, tree=tree)
            assert O.commit()
        return _trace_with_pairs(O, np.arange(len(nodes)), faces_of, rays, pairs)
    node_masks = np.full(len(nodes), ALL, dtype=np.uint32) if node_masks is None else np.asarray(node_masks, dtype=np.uint32)
    ray_words = np.full(n, ALL, dtype=np.uint32) if ray_words is None else np.asarray(ray_words, dtype=np.uint32)
    words = np.unique(ray_words)
    assert len(words) <= MAX_WORDS, "keep the CPU side in seconds"
    hits = miss_records(rays)
    flags = np.zeros(n, dtype=np.uint8)
    for w in words:
        sel = np.nonzero(ray_words == w)[0]
        kept = np.nonzero((node_masks & w) != 0)[0]
        if len(kept) == 0:
            continue
        O = ob.SceneOracle(oracle)
        for k in kept:
            v, f, x, tree = nodes[k]
            O.add_node(v, f, x, tree=tree)
        assert O.commit()
        h, m = _trace_with_pairs(O, kept, faces_of, rays[sel], pairs[sel])
        named = h["node_id"] != ALL
        h["node_id"][named] = kept[h["node_id"][named]].astype(np.uint32)
        hits[sel] = h
        flags[sel] = m
    return hits, flags


def bounce_wave(rays, hits, flags, rng, dir_scale=1.0, limit=None):
    """The next wave of a path tracer without an epsilon: one ray per primary hit, started AT the hit point (org + t * dir / |dir|,
    rounded to float32) in a random direction of length `dir_scale`, with the pair of the triangle it starts on.  Returns
    (rays, pairs, records): `records` are the primary wave's records of those rays — `&records[0].prim_id` at stride 20 is `pairs`."""
    sel = np.nonzero(flags)[0]
    if limit is not None and len(sel) > limit:
        sel = np.sort(rng.choice(sel, size=limit, replace=False))
    d = rays["dir"][sel].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = np.zeros(len(sel), dtype=RAY_F32)
    out["org"] = (rays["org"][sel].astype(np.float64) + hits["t"][sel].astype(np.float64)[:, None] * d).astype(np.float32)
    nd = rng.normal(size=(len(sel), 3))
    nd /= np.linalg.norm(nd, axis=1, keepdims=True)
    out["dir"] = (nd * dir_scale).astype(np.float32)
    out["min_t"] = 0.0
    out["max_t"] = 3.0e38
    records = np.ascontiguousarray(hits[sel])
    return out, pairs_of(records), records


def own_pair_share(hits, flags, pairs):
    """Share of the rays whose record names the pair they carry: the triangle they started on."""
    own = (flags == 1) & (hits["prim_id"] == pairs[:, 0]) & (hits["node_id"] == pairs[:, 1])
    return float(own.mean())


def stacked_planes(rng, count=600):
    """One plane mesh instanced three times, translated by 0, 3 and 6 along z; `count` rays from random interior points of random
    faces p of node 0, straight up (+z), with the pair (p, 0).  Skipped, every ray must name (p, 1): an implementation that compares
    the primitive id alone rejects face p of every copy and misses (or names node 2 where the planes' lumps let a neighbour in)."""
    from nanort_amd import scenes
    from scene_fixture import xform

    pv, pf = scenes.plane(12, 6)
    xs = [xform(trans=(0, 0, 3.0 * k)) for k in range(3)]
    p = rng.integers(0, pf.shape[0], size=count)
    b = rng.uniform(0.15, 0.7, size=(count, 2))
    b[:, 1] *= (1.0 - b[:, 0])  # barycentrics well inside the face
    tri = pv[pf[p]].astype(np.float64)
    pts = tri[:, 0] + b[:, :1] * (tri[:, 1] - tri[:, 0]) + b[:, 1:] * (tri[:, 2] - tri[:, 0])
    rays = np.zeros(count, dtype=RAY_F32)
    rays["org"] = pts.astype(np.float32)
    rays["dir"][:, 2] = 1.0
    rays["max_t"] = 3.0e38
    pairs = np.ascontiguousarray(np.stack([p, np.zeros(count)], axis=1).astype(np.uint32))
    return (pv, pf), xs, rays, pairs

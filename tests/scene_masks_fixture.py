"""Instance visibility masks on scenes (nrtSceneSetNodeMasks, nrtScene*BatchMasked*): what a masked query must return, stated
with the restatement alone (oracle/nanosg_oracle.c through oracle.bindings.SceneOracle), and the bit layout of the line fixture.

The rule: an instance exists for a ray iff (node word & ray word) != 0, and a masked query answers exactly as the unmasked query
would on a scene committed from the visible nodes alone, with the node ids kept.  So, per distinct ray word: a SceneOracle of the
visible nodes (same meshes, same trees, same transforms, in node order), the rays that carry the word traced through it, node_id
mapped back through the list of kept ids.  A word that leaves no node visible gives the miss record of the unmasked call."""
import numpy as np

from oracle import bindings as ob

ALL = 0xFFFFFFFF
MAX_WORDS = 8  # distinct ray words per expectation: each costs one CPU scene


def scene_nodes(O):
    """(verts, faces, xform, (nodes, indices)) of every node of a SceneOracle, in node-id order."""
    out = []
    for (v, f, nodes, idx), n in zip(O.keep, O.nodes):
        out.append((v, f, np.array(list(n.local_xform), dtype=np.float32).reshape(4, 4), (nodes, idx)))
    return out


def miss_records(rays):
    h = np.zeros(rays.shape[0], dtype=ob.SCENE_HIT)
    h["t"] = rays["max_t"]
    h["prim_id"] = ALL
    h["node_id"] = ALL
    return h


def expect_masked(oracle, nodes, node_masks, rays, ray_words=None):
    """(hits, flags) a masked query must return.  `nodes`: scene_nodes(...) of the whole scene; `node_masks`: one word per node or
    None (all ones); `ray_words`: one word per ray or None (all ones)."""
    n = rays.shape[0]
    node_masks = np.full(len(nodes), ALL, dtype=np.uint32) if node_masks is None else np.asarray(node_masks, dtype=np.uint32)
    ray_words = np.full(n, ALL, dtype=np.uint32) if ray_words is None else np.asarray(ray_words, dtype=np.uint32)
    assert node_masks.shape == (len(nodes),) and ray_words.shape == (n,)
    words = np.unique(ray_words)
    assert len(words) <= MAX_WORDS, "keep the CPU side in seconds"
    hits = miss_records(rays)
    flags = np.zeros(n, dtype=np.uint8)
    for w in words:
        sel = np.nonzero(ray_words == w)[0]
        kept = np.nonzero((node_masks & w) != 0)[0]
        if len(kept) == 0:
            continue  # nothing exists for these rays: the miss record
        O = ob.SceneOracle(oracle)
        for k in kept:
            v, f, x, tree = nodes[k]
            O.add_node(v, f, x, tree=tree)
        assert O.commit()
        h, m = O.traverse(rays[sel])
        named = h["node_id"] != ALL
        h["node_id"][named] = kept[h["node_id"][named]].astype(np.uint32)
        hits[sel] = h
        flags[sel] = m
    return hits, flags


# ---- the line fixture (tests/test_gpu_scene_occlusion.py line_fixture: 70 A boxes along x, then B, then 10 more A) ----------------
# bit 0 is absent from A[0..9], bit 1 from A[0..5], bit 2 from A[0..6], bit 3 from B alone; every other bit is set everywhere.
LINE_B = 70


def line_node_masks():
    m = np.full(81, ALL, dtype=np.uint32)
    m[0:10] &= ~np.uint32(1)
    m[0:6] &= ~np.uint32(2)
    m[0:7] &= ~np.uint32(4)
    m[LINE_B] &= ~np.uint32(8)
    return m


# What the `front` rays (they enter all 81 boxes; unmasked, B ranks 71st) and the `mid` rays (60 boxes, then B, 61st) must
# return per ray word: (word, flag on front or None, flag on mid or None).
LINE_TABLE = [
    (ALL, 0, None),  # B ranks 71st
    (1, 1, None),    # ten A hidden: 61st
    (4, 1, None),    # seven A hidden: exactly 64th
    (2, 0, None),    # six A hidden: 65th
    (8, None, 0),    # the blocker itself hidden
    (0, 0, 0),
]


def line_ray_words(num_rays, front, mid):
    """One word per ray of the line fixture, interleaved by ray index so that every wave mixes visible sets: the front rays cycle
    through the table's front words, the mid rays through its mid words, the rest through all six."""
    fw = np.array([w for w, a, _ in LINE_TABLE if a is not None], dtype=np.uint32)
    mw = np.array([w for w, _, b in LINE_TABLE if b is not None], dtype=np.uint32)
    aw = np.array([w for w, _, _ in LINE_TABLE], dtype=np.uint32)
    idx = np.arange(num_rays)
    words = aw[idx % len(aw)]
    words[front] = fw[idx[front] % len(fw)]
    words[mid] = mw[idx[mid] % len(mw)]
    return words


def check_line_table(flags, words, front, mid):
    """Every class of LINE_TABLE is non-empty and uniform in `flags`."""
    for w, on_front, on_mid in LINE_TABLE:
        for sl, want in ((front, on_front), (mid, on_mid)):
            if want is None:
                continue
            got = flags[sl][words[sl] == w]
            assert len(got) >= 50, (w, len(got))
            assert (got == want).all(), (hex(w), want, float(got.mean()))

"""Fixtures of the combined ray query (include/nanort_hip.h, "one descriptor for every triangle ray query"), shared by
tests/test_query_model.py on the CPU and tests/test_gpu_query.py on the GPU: the expectation, and two worlds on which a per-ray time,
a per-ray visibility word and a per-ray skip id all matter on the same ray.

The expectation needs no oracle of its own.  The rays are grouped by (bits of the clamped time, word, skip id); each group is traced
by oracle.traverse — the project's pinned restatement of the reference — over the context's own nodes and indices, with the vertices
interpolated to the group's time (motion_fixture.lerp) when MOTION is set, the faces the group does not see collapsed to a point
(masks_fixture.hidden_faces) when MASKED is set, and skip_prim_id = the group's id.  All three are "the intersector returns false
before it touches the ray's state" (the collapsed face is rejected at det == 0: masks_fixture), so every field is bit-exact."""
import numpy as np

import masks_fixture as kf
import motion_fixture as mf
import own_walks_fixture as ow
from helpers import trace_options
from nanort_amd import scenes
from nanort_amd.wire import TRACE_OPTIONS, default_trace_options, hit_dtype, ray_dtype, widen_rays

NO_ID = 0xFFFFFFFF

SHELL_SCALES = (1.0, 1.25, 1.5, 1.75)
SHELL_CENTRE = (0.0, 5.0, 0.0)
SHELL_RAYS = 4099
SHELL_ORIGIN = (3.0, 6.0, 1.0)
SHELL_MIN_ALL_THREE = 0.10  # share of the rays whose record differs from the record without ids, without masks AND at time 0

PILE_MIN_ALL_THREE = 150    # the same on the pile, in rays (of own_walks_fixture.PILE_RAYS)


def expected(oracle, nodes, idx, v0, v1, f, prim_masks, rays, times=None, ray_masks=None, skip_ids=None, motion=False, masked=False, opts=None,
             count=False):
    """(hits, mask[, max stack over the whole query]) a query must return.  times / ray_masks / skip_ids None: every ray at time 0 /
    with 0xFFFFFFFF / with the options' skip_prim_id.  motion / masked: the query's flags (an array whose flag is off is not read)."""
    real = v0.dtype
    n = rays.shape[0]
    f = np.ascontiguousarray(f, dtype=np.uint32)
    base = np.asarray(default_trace_options() if opts is None else opts, dtype=TRACE_OPTIONS).reshape(-1)[:1].copy()  # one record
    s = mf.clamp_times(np.zeros(n) if (times is None or not motion) else times, real)
    sbits = s.view(np.uint32 if real == np.float32 else np.uint64).astype(np.uint64)
    words = np.full(n, 0xFFFFFFFF, dtype=np.uint32) if (ray_masks is None or not masked) else np.asarray(ray_masks, dtype=np.uint32)
    ids = np.full(n, int(base["skip_prim_id"][0]), dtype=np.uint32) if skip_ids is None else np.asarray(skip_ids, dtype=np.uint32)
    keys = np.stack([sbits, words.astype(np.uint64), ids.astype(np.uint64)], axis=1)
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(inverse, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(inverse, minlength=first.shape[0]))])
    hits = np.zeros(n, dtype=hit_dtype(real))
    mask = np.zeros(n, dtype=np.uint8)
    depth = 0
    lerped, hidden = {}, {}
    for g in range(first.shape[0]):
        sel = order[bounds[g]:bounds[g + 1]]
        i = first[g]
        v = v0
        if motion:
            b = int(sbits[i])
            if b not in lerped:
                lerped[b] = mf.lerp(v0, v1, s[i])
            v = lerped[b]
        fg = f
        if masked:
            w = int(words[i])
            if w not in hidden:
                hidden[w] = kf.hidden_faces(f, prim_masks, w)
            fg = hidden[w]
        o = base.copy()
        o["skip_prim_id"] = ids[i]
        out = oracle.traverse(nodes, idx, v, fg, np.ascontiguousarray(rays[sel]), o, count=count)
        hits[sel], mask[sel] = out[0], out[1]
        if count:
            depth = max(depth, int(out[2][3]))
    return (hits, mask, depth) if count else (hits, mask)


def num_groups(real, times, ray_masks, skip_ids):
    s = mf.clamp_times(times, real)
    keys = np.stack([s.view(np.uint32 if real == np.float32 else np.uint64).astype(np.uint64), np.asarray(ray_masks, dtype=np.uint64),
                     np.asarray(skip_ids, dtype=np.uint64)], axis=1)
    return np.unique(keys, axis=0).shape[0]


def ids_of(hits, mask):
    """The skip id of every ray: the primitive its record names, NO_ID on a miss (the ray leaves the triangle it would hit)."""
    return np.ascontiguousarray(np.where(mask != 0, hits["prim_id"], NO_ID).astype(np.uint32))


class World:
    """A mesh with a second keyframe, random prim words, the reference's tree with union boxes, rays with a time, a word and a skip id
    each — the id is the primitive the MOTION+MASKED record of the same ray names.  figures(): the expectation of the all-three
    query and the per-ray 'every feature matters' predicate."""

    def __init__(self, oracle, real, v, v1, f, rays, times, words):
        self.real = np.dtype(real).type
        self.v, self.v1, self.f = v, v1, np.ascontiguousarray(f, dtype=np.uint32)
        self.rays, self.times, self.words = rays, times, words
        self.nodes, self.idx, self.stats = ow.motion_tree(oracle, v, v1, self.f)
        self.pm = kf.random_prim_masks(self.f.shape[0])
        h, m = self.expected(oracle, ids=False)
        self.ids = ids_of(h, m)

    def expected(self, oracle, motion=True, masked=True, ids=True, opts=None, count=False, times=None):
        return expected(oracle, self.nodes, self.idx, self.v, self.v1, self.f, self.pm, self.rays, self.times if times is None else times, self.words,
                        self.ids if ids else None, motion=motion, masked=masked, opts=opts, count=count)

    def figures(self, oracle):
        """(hits, mask, max stack, all_three): all_three[i] — ray i's record differs from the record of the query without ids, of the
        query without masks and of the query at time 0, all at once."""
        h, m, depth = self.expected(oracle, count=True)
        no_ids = self.expected(oracle, ids=False)
        no_masks = self.expected(oracle, masked=False)
        at_zero = self.expected(oracle, times=np.zeros(self.rays.shape[0], dtype=self.real))
        all_three = mf.differs(h, m, *no_ids) & mf.differs(h, m, *no_masks) & mf.differs(h, m, *at_zero)
        return h, m, depth, all_three


def shells(oracle, real):
    """Four concentric copies of scenes.sphere(32, 17) about SHELL_CENTRE, keyframe 1 the wave deformation, 4099 rays from a point
    between the shells in random directions: every ray crosses several layers, so hiding or skipping its first hit leaves another."""
    sv, sf = scenes.sphere(32, 17)
    c = np.asarray(SHELL_CENTRE, dtype=np.float64)
    vs, fs = [], []
    for k, scale in enumerate(SHELL_SCALES):
        vs.append((sv.astype(np.float64) - c) * scale + c)
        fs.append(sf + np.uint32(k * sv.shape[0]))
    v = np.ascontiguousarray(np.concatenate(vs).astype(real))
    f = np.ascontiguousarray(np.concatenate(fs), dtype=np.uint32)
    v1 = mf.deformations(v)["wave"]
    rng = np.random.default_rng(5)
    rays = np.zeros(SHELL_RAYS, dtype=ray_dtype(np.float32))
    rays["org"] = SHELL_ORIGIN
    rays["dir"] = rng.normal(size=(SHELL_RAYS, 3))
    rays["min_t"] = 0.0
    rays["max_t"] = 1e30
    if np.dtype(real) == np.float64:
        rays = widen_rays(rays)
    return World(oracle, real, v, v1, f, np.ascontiguousarray(rays), mf.assign_times(SHELL_RAYS, real), kf.assign_ray_masks(SHELL_RAYS))


def pile(oracle, real):
    """own_walks_fixture's pile with its second keyframe: the reference's tree is deeper than the walks' 32 LDS stack entries."""
    v, f, rays, words = ow.pile(real)
    return World(oracle, real, v, ow.pile_keyframe1(v), f, rays, mf.assign_times(ow.PILE_RAYS, real, seed=ow.PILE_RAY_SEED), words)


SHELL_OPTIONS = dict(range_=(50, 900), cull=True)  # the arm with trace options (the skip id is per ray)


def shell_options():
    return trace_options(**SHELL_OPTIONS)

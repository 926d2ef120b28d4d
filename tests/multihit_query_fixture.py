"""Fixtures of multi-hit with per-ray skip ids, visibility words and motion times (include/nanort_hip.h, nrtMultiHitQueryBatch*;
DESIGN.md 3.16), shared by tests/test_multihit_query_model.py on the CPU and tests/test_gpu_multihit_query.py on the GPU.

The expectation needs no oracle of its own.  As in tests/query_fixture.py::expected the rays are grouped by (bits of the clamped time,
word, skip id); each group is walked by multihit_fixture.model — the restatement of the multi-hit contract over the pinned triangle
and slab tests — over the context's own nodes and indices, with the vertices interpolated to the group's time (motion_fixture.lerp)
when MOTION is set, the faces the group does not see collapsed to a point (masks_fixture.hidden_faces) when MASKED is set, and
skip_prim_id = the group's id.  All three are "the intersector returns false before it touches the ray's state", so every byte of
every row is exact.  The worlds are query_fixture's shells and pile as they are."""
import os
import re

import numpy as np

import masks_fixture as kf
import motion_fixture as mf
import multihit_fixture as mhf
import query_fixture as qf
from nanort_amd.wire import TRACE_OPTIONS, default_trace_options, hit_dtype

COMBOS = {"ids": (False, False, True), "motion+ids": (True, False, True), "masked+ids": (False, True, True), "motion+masked": (True, True, False),
          "all": (True, True, True)}

_WORLDS, _EXPECTED = {}, {}


def staged_rows_cap():
    """The bytes of rows one launch of the staged host path holds, as nanort_amd/csrc/api_query.hip names them."""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nanort_amd", "csrc", "api_query.hip")).read()
    found = re.findall(r"const\s+uint64_t\s+kMultiHitStagedBytes\s*=\s*(\d+)ull\s*<<\s*(\d+)\s*;", text)
    assert len(found) == 1, "kMultiHitStagedBytes: %d statements in api_query.hip" % len(found)
    return int(found[0][0]) << int(found[0][1])


def expected(nodes, idx, v0, v1, f, prim_masks, rays, K, times=None, ray_masks=None, skip_ids=None, motion=False, masked=False, opts=None):
    """(hits[n, K], counts[n]) a multi-hit query must return.  times / ray_masks / skip_ids None: every ray at time 0 / with 0xFFFFFFFF /
    with the options' skip_prim_id.  motion / masked: the query's flags (an array whose flag is off is not read)."""
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
    hits = np.zeros((n, K), dtype=hit_dtype(real))
    counts = np.zeros(n, dtype=np.uint32)
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
        hits[sel], counts[sel] = mhf.model(nodes, idx, v, fg, np.ascontiguousarray(rays[sel]), K, o)
    return hits, counts


def world(oracle, name, real):
    """query_fixture's shells or pile of one precision, built once per process."""
    key = (name, np.dtype(real).name)
    if key not in _WORLDS:
        _WORLDS[key] = (qf.shells if name == "shells" else qf.pile)(oracle, real)
    return _WORLDS[key]


def expect(oracle, name, real, K, motion=True, masked=True, ids=True, opts=None, times=None, prim_masks=None):
    """The expectation of one (world, precision, K, combination[, options]), computed once per process and never changed."""
    w = world(oracle, name, real)
    key = (name, np.dtype(real).name, int(K), bool(motion), bool(masked), bool(ids), None if opts is None else np.asarray(opts).tobytes(),
           None if times is None else np.asarray(times).tobytes(), None if prim_masks is None else np.asarray(prim_masks).tobytes())
    if key not in _EXPECTED:
        h, c = expected(w.nodes, w.idx, w.v, w.v1, w.f, w.pm if prim_masks is None else prim_masks, w.rays, K, w.times if times is None else times,
                        w.words, w.ids if ids else None, motion=motion, masked=masked, opts=opts)
        h.setflags(write=False)
        c.setflags(write=False)
        _EXPECTED[key] = (h, c)
    return _EXPECTED[key]


def rows_bytes(h):
    """Every field of every record, row by row: [n] byte strings (fp64 records: the padding left out)."""
    n = h.shape[0]
    parts = [np.ascontiguousarray(h[k]).view(np.uint8).reshape(n, -1) for k in h.dtype.names]
    return np.concatenate(parts, axis=1)


def rows_differ(h, c, h2, c2):
    """[n] bool: ray i's row or count differs between two results."""
    return (rows_bytes(h) != rows_bytes(h2)).any(axis=1) | (c != c2)


def assert_rows_identical(eh, ec, h, c):
    """Rows and counts byte for byte; on a mismatch the first differing ray is named."""
    h = np.asarray(h).reshape(eh.shape)
    bad = rows_differ(eh, ec, h, np.asarray(c))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError("%d of %d rays differ; ray %d: want count %d %s, got count %d %s" % (int(bad.sum()), bad.shape[0], i, int(ec[i]), eh[i], int(c[i]), h[i]))


def all_three(oracle, name, real, K):
    """[n] bool: ray i's row differs from the row of the query without ids, of the query without masks and of the query at time 0, all
    at once."""
    w = world(oracle, name, real)
    h, c = expect(oracle, name, real, K)
    out = np.ones(w.rays.shape[0], dtype=bool)
    for kw in (dict(ids=False), dict(masked=False), dict(times=np.zeros(w.rays.shape[0], dtype=w.real))):
        out &= rows_differ(h, c, *expect(oracle, name, real, K, **kw))
    return out

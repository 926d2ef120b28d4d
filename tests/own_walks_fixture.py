"""Fixtures of tests/test_gpu_own_walks.py, shared with tests/test_masks_model.py and tests/test_motion_model.py, which assert their
conditions on the CPU (they need the oracle only): the pile whose reference tree is deeper than the own walks' 32 LDS stack entries
(helpers.deep_stack_case at a size that keeps every test at a few seconds), and the random soup with its hostile rays
(multihit_fixture) dressed with visibility words and with a second keyframe.

The bounds are those the GPU tests rest on; they hold for the reference alone and none of them comes from what a kernel returns."""
import numpy as np

import masks_fixture as kf
import motion_fixture as mf
import multihit_fixture as hf
import refit_model
from helpers import deep_stack_case
from nanort_amd.wire import widen_rays

PILE_RAYS = 1500
PILE_RAY_SEED = 5      # assign_ray_masks
PILE_MIN_STACK = 33    # the oracle's max-stack counter must pass this for every ray word: the walk is past its 32 LDS entries
PILE_MIN_OTHER = 375   # rays (a quarter) whose masked record is a hit on another primitive than the unmasked record

SOUP_RAYS = 6000
SOUP_RAY_SEED = 9
SOUP_MIN_OTHER = 150   # as PILE_MIN_OTHER
SOUP_MOTION_MIN_HITS = 100
SOUP_MOTION_MIN_DIFFER = 50  # records that differ from the keyframe-0 record
SOUP_JITTER = 2e-2


def pile(real):
    """(v, f, rays, ray words): 1536 large triangles across the z axis and 512 exact duplicates, 1500 rays along the axis."""
    v, f, _, _, rays = deep_stack_case(n_rays=PILE_RAYS, nt=1536, ndup=512)
    v = np.ascontiguousarray(v.astype(real))
    if np.dtype(real) == np.float64:
        rays = widen_rays(rays)
    return v, np.ascontiguousarray(f, dtype=np.uint32), np.ascontiguousarray(rays), kf.assign_ray_masks(PILE_RAYS, seed=PILE_RAY_SEED)


def pile_keyframe1(v):
    """Keyframe 1 of the pile: every vertex moved along z (the triangles tilt; the rays, along z, still cross all of them)."""
    rng = np.random.default_rng(23)
    v1 = v.copy()
    v1[:, 2] += rng.normal(scale=0.05, size=v.shape[0]).astype(v.dtype)
    return np.ascontiguousarray(v1)


def motion_tree(oracle, v0, v1, f):
    """The reference's tree over keyframe 0 with every box the union over the two keyframes (what a motion context holds)."""
    nodes, idx, st = oracle.build(v0, f)
    return mf.motion_boxes(refit_model.refit, nodes, idx, v0, v1, f), idx, st


def soup_masked(real):
    """(vbuf, f, stride, rays, ray words, prim words): the soup with strided vertices, its hostile rays, random prim words."""
    vbuf, f, stride = hf.soup(real)
    f = np.ascontiguousarray(f, dtype=np.uint32)
    return vbuf, f, stride, hf.hostile_rays(real, SOUP_RAYS), kf.assign_ray_masks(SOUP_RAYS, seed=SOUP_RAY_SEED), kf.random_prim_masks(f.shape[0])


def soup_motion(real):
    """(v0, v1, f, rays, times): the same soup as tight xyz rows (the keyframe setter reads both keyframes with one stride), keyframe 1
    a jitter of it, the same hostile rays, one time per ray."""
    vbuf, f, _ = hf.soup(real)
    v0 = np.ascontiguousarray(vbuf[:, :3])
    rng = np.random.default_rng(11)
    v1 = np.ascontiguousarray((v0 + rng.normal(scale=SOUP_JITTER, size=v0.shape)).astype(real))
    return v0, v1, np.ascontiguousarray(f, dtype=np.uint32), hf.hostile_rays(real, SOUP_RAYS), mf.assign_times(SOUP_RAYS, real)


def masked_figures(oracle, nodes, idx, v, f, pm, rays, words, stride=None):
    """(expected hits, expected flags, {word: max stack}, rays that hit, rays whose record is another primitive than the unmasked one)."""
    eh, em, depth = kf.expected(oracle, nodes, idx, v, f, pm, rays, words, stride=stride, count=True)
    ph, pmask = oracle.traverse(nodes, idx, v, f, rays, stride=stride)
    return eh, em, depth, int(em.sum()), int(kf.other_primitive(eh, em, ph, pmask).sum())


def motion_figures(oracle, nodes, idx, v0, v1, f, rays, times):
    """(expected hits, expected flags, rays that hit, records that differ from the keyframe-0 record)."""
    eh, em = mf.expected(oracle, nodes, idx, v0, v1, f, rays, times)
    h0, m0 = oracle.traverse(nodes, idx, v0, f, rays)
    return eh, em, int(em.sum()), int(mf.differs(eh, em, h0, m0).sum())

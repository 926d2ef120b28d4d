"""Visibility-mask test fixtures (include/nanort_hip.h, "visibility masks"), shared by tests/test_masks_model.py on
the CPU and tests/test_gpu_masks.py on the GPU: the per-primitive mask patterns, a per-ray assignment in which neighbouring rays
never share a mask, and the expectation.

The expectation needs no oracle of its own.  For the rays that share one mask word m the expected records are oracle.traverse — the
project's pinned restatement of the reference — over the context's own tree and the faces f_m, which are f with every face the
rays do not see replaced by (f[i, 0], f[i, 0], f[i, 0]).  For finite vertices such a triangle has A == B == C, so the edge functions
U = Cx * By - Cy * Bx, V, W subtract the same product from itself and are exactly 0 (no contraction: -ffp-contract=off), in the
double-precision recomputation too; the intersector rejects it at `det == 0`, before it touches the ray's state.  The boxes are
never read from the faces.  That is "the intersector returns false for this primitive", bit for bit."""
import numpy as np

from nanort_amd.wire import hit_dtype

# The words a ray may carry: everything, nothing, single low bits, the top bit (a sign bit in a signed comparison), a middle bit,
# two bits, everything but the top bit.
RAY_MASK_VALUES = (0xFFFFFFFF, 0, 1, 2, 0x80000000, 0x00010000, 3, 0x7FFFFFFF)

# Seed of the random prim masks: tests/test_masks_model.py asserts the fixture condition for it (with ray mask 1 at least a tenth of
# through_rays get a record that is neither the unmasked record nor a miss: 16.9 % with this seed).
SEED = 16


def random_prim_masks(nf, seed=SEED):
    """One uniformly random 32-bit word per face: every bit hides about half of the mesh."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, size=nf, dtype=np.uint64).astype(np.uint32)


def prim_patterns(nf, seed=SEED):
    """name -> uint32[nf].  `mod3` (bit = prim_id % 3) is not invariant under the builder's permutation of the faces: a walk that
    indexed prim-order words by leaf position, or the reverse, fails on it."""
    ids = np.arange(nf, dtype=np.uint32)
    return {
        "random": random_prim_masks(nf, seed),
        "zeros": np.zeros(nf, dtype=np.uint32),
        "ones": np.full(nf, 0xFFFFFFFF, dtype=np.uint32),
        "bit31": np.full(nf, 0x80000000, dtype=np.uint32),
        "mod3": (np.uint32(1) << (ids % np.uint32(3))).astype(np.uint32),
    }


def assign_ray_masks(n, seed=3):
    """One of RAY_MASK_VALUES per ray, pseudo-random, consecutive rays always different: the lanes of a wave differ, and a lane
    refilled with the next ray of its chunk must pick up that ray's own word."""
    rng = np.random.default_rng(seed)
    k = len(RAY_MASK_VALUES)
    step = rng.integers(1, k, size=n)  # 1 .. k - 1: never the predecessor's value
    step[0] = rng.integers(0, k)
    which = np.cumsum(step) % k
    assert n < 2 or (which[1:] != which[:-1]).all()
    return np.ascontiguousarray(np.asarray(RAY_MASK_VALUES, dtype=np.uint32)[which])


def through_rays(cam):
    """`cam` (scenes.camera_rays: a pinhole at (0, 5, 20) looking down -z into C1's open box) turned a quarter about the vertical axis
    through the box: a pinhole at (-20, 5, 0) looking down +x, THROUGH the box's closed side walls.  A ray of the camera set meets one
    layer of geometry nearly everywhere (the box is open towards the camera; only the 4 % of the rays that cross the small mesh inside
    meet more), so hiding its first hit leaves a miss: over 64 seeds at most 1.7 % of the camera rays get a masked record that is
    neither the unmasked record nor a miss.  These rays cross two walls and whatever stands between them."""
    r = cam.copy()
    r["org"][:, 0], r["org"][:, 2] = -cam["org"][:, 2], cam["org"][:, 0]
    r["dir"][:, 0], r["dir"][:, 2] = -cam["dir"][:, 2], cam["dir"][:, 0]
    return np.ascontiguousarray(r)


def visible(prim_masks, m):
    return (np.asarray(prim_masks, dtype=np.uint32) & np.uint32(m)) != 0


def hidden_faces(f, prim_masks, m):
    """f with every face invisible under the ray mask m collapsed to its first corner."""
    f_m = np.ascontiguousarray(f, dtype=np.uint32).copy()
    hide = ~visible(prim_masks, m)
    f_m[hide] = f_m[hide, :1]
    return f_m


def expected(oracle, nodes, idx, v, f, prim_masks, rays, ray_masks, opts=None, stride=None, count=False):
    """(hits, mask) a masked query must return.  ray_masks None: every ray 0xFFFFFFFF.  `stride`: the vertex rows' stride in bytes
    (None: tight xyz).  count: also {word: the oracle's max-stack counter over the rays that carry it}."""
    n = rays.shape[0]
    hits = np.zeros(n, dtype=hit_dtype(v.dtype))
    mask = np.zeros(n, dtype=np.uint8)
    words = np.full(n, 0xFFFFFFFF, dtype=np.uint32) if ray_masks is None else np.asarray(ray_masks, dtype=np.uint32)
    depth = {}
    for m in np.unique(words):
        sel = np.nonzero(words == m)[0]
        out = oracle.traverse(nodes, idx, v, hidden_faces(f, prim_masks, m), np.ascontiguousarray(rays[sel]), opts, stride=stride, count=count)
        hits[sel], mask[sel] = out[0], out[1]
        if count:
            depth[int(m)] = int(out[2][3])
    return (hits, mask, depth) if count else (hits, mask)


def other_primitive(eh, em, ph, pm):
    """Per ray: the masked record (eh, em) is a hit on another primitive than the unmasked record (ph, pm) names (which may be a
    miss): the ray went on walking past what it does not see."""
    return (em != 0) & ((pm == 0) | (eh["prim_id"] != ph["prim_id"]))


def miss_records(rays, real):
    """The miss record of every ray: {0, 0, max_t, 0xFFFFFFFF}, flag 0."""
    h = np.zeros(rays.shape[0], dtype=hit_dtype(real))
    h["t"] = rays["max_t"]
    h["prim_id"] = 0xFFFFFFFF
    return h, np.zeros(rays.shape[0], dtype=np.uint8)

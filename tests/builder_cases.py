"""The inputs at which GPU builds are compared with the model of the builder's rule (builder_model.py), shared by
test_builder_model.py (CPU: the model's trees are valid and its decisions cover every path of the rule) and
test_gpu_builder_model.py (GPU: byte equality).  A case is (id, kind, precision, input arrays, (min_leaf, bin_size, max_depth));
the model's tree of a case is computed once per process."""
import functools

import numpy as np

import builder_model as bm
from bvh_check import validate_bvh

SIZES = (2, 5, 255, 256, 257, 2049, 4097)
OPTIONS = ((4, 64, 256), (1, 8, 256), (16, 200, 12), (2, 5, 9), (4, 2, 256))
DEFAULT = (4, 64, 256)
# (precision, n, ratio, min_leaf) of test_the_two_subtree_kernels_agree_on_chains_of_lopsided_splits (test_gpu_build.py)
CHAINS = ((np.float64, 256, 0.3, 1), (np.float64, 256, 0.5, 1), (np.float64, 200, 0.2, 2), (np.float32, 100, 0.45, 1), (np.float64, 5000, 0.97, 1))


def soup(n):
    """test_rebuilds_of_one_context_hand_their_bins_on_clean's geometry: small triangles about centres uniform in a cube."""
    rng = np.random.default_rng(77)
    tri = rng.uniform(-1, 1, (n, 1, 3)) + rng.normal(0, 0.03, (n, 3, 3))
    return tri.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def coincident():
    """test_coincident_centroids_use_the_median_fallback's mesh: 1000 copies of one triangle and 3 of another."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [6, 5, 5], [5, 6, 5]], dtype=np.float32)
    return v, np.array([[0, 1, 2]] * 1000 + [[3, 4, 5]] * 3, dtype=np.uint32)


def sliver_chain(n, ratio):
    """test_gpu_build.py's _sliver_chain: tiny triangles whose centroids sit at ratio**i along x, a chain of lopsided splits."""
    x = ratio ** np.arange(n, dtype=np.float64)
    v = np.empty((3 * n, 3), dtype=np.float64)
    s = 1e-3 * x
    v[0::3] = np.stack([x, np.zeros(n), np.zeros(n)], 1)
    v[1::3] = np.stack([x + s, s, np.zeros(n)], 1)
    v[2::3] = np.stack([x, s, s], 1)
    return v, np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def copies(nx, ny, nz):
    """One small triangle copied to every point of an nx x ny x nz lattice away from the origin.  With an odd count along an
    axis the cuts come in mirrored pairs whose costs are equal in exact arithmetic and a few ulps apart as computed: which of
    the two wins is decided by the rounding of every operation of the rule, in the order the rule states them."""
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    p = np.stack([0.37 + 0.1 * i.ravel(), -1.21 + 0.13 * j.ravel(), 2.6 + 0.17 * k.ravel()], 1)
    t = np.array([[0, 0, 0], [0.03, 0.01, 0], [0.01, 0.03, 0.02]])
    v = (p[:, None, :] + t[None]).reshape(-1, 3)
    return v, np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)


def _name(real):
    return np.dtype(real).name


def _cases():
    out = {}

    def add(cid, kind, real, make, options):
        assert cid not in out
        out[cid] = (kind, real, make, options)

    both = (np.float32, np.float64)
    for n in SIZES:
        for o in OPTIONS:
            for real in both:
                add("soup%d-%s-%d_%d_%d" % ((n, _name(real)) + o), "triangles", real, functools.partial(soup, n), o)
    for o in ((4, 64, 256), (1, 8, 256)):
        for real in both:
            add("lattice9k-%s-%d_%d_%d" % ((_name(real),) + o), "triangles", real, lambda: bm.tree_hash_inputs()["grid9k"], o)
    for real in both:
        add("coincident-%s" % _name(real), "triangles", real, coincident, DEFAULT)
    for real, n, ratio, min_leaf in CHAINS:
        add("chain%d_%g_%d-%s" % (n, ratio, min_leaf, _name(real)), "triangles", real, functools.partial(sliver_chain, n, ratio), (min_leaf, 64, 256))
    for o in ((4, 64, 256), (1, 8, 256)):  # (not in the issue's list: the cases above hold no near tie, see test_builder_model.py)
        for real in both:
            add("copies1331-%s-%d_%d_%d" % ((_name(real),) + o), "triangles", real, functools.partial(copies, 11, 11, 11), o)
    add("soup20000-float32", "triangles", np.float32, functools.partial(soup, 20000), DEFAULT)

    def spheres():
        from nanort_amd import scenes
        return scenes.random_spheres(3000)

    def hair():
        import curves_fixture
        return curves_fixture.hair(3000)

    def cylinders():
        from nanort_amd import scenes
        return scenes.random_cylinders(257)

    add("spheres3000", "spheres", np.float32, spheres, DEFAULT)
    add("hair3000", "curves", np.float32, hair, DEFAULT)
    add("cylinders257", "cylinders", np.float32, cylinders, DEFAULT)
    return out


CASES = _cases()
IDS = list(CASES)


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(kind, precision, input arrays as the builder gets them, options) of a case."""
    kind, real, make, options = CASES[cid]
    a, b = make()
    if kind == "triangles":
        a = np.ascontiguousarray(a, dtype=real)
    return kind, real, (a, b), options


@functools.lru_cache(maxsize=None)
def model(cid):
    """(nodes, indices, decisions) of the model for a case."""
    kind, real, arrays, (min_leaf, bin_size, max_depth) = inputs(cid)
    return bm.build(*bm.records(kind, real, *arrays), real, min_leaf, max_depth, bin_size)


def validate(cid, nodes, idx):
    """bvh_check.validate_bvh(..., low_side_first=True) of a tree over a case's primitives.  The validator reads triangles; for
    the other kinds it is given the boxes as degenerate triangles (exact bounds) and then the centres (the low side first)."""
    kind, real, arrays, (min_leaf, bin_size, max_depth) = inputs(cid)
    if kind == "triangles":
        return validate_bvh(nodes, idx, arrays[0], arrays[1], min_leaf=min_leaf, max_depth=max_depth, low_side_first=True)
    bmin, bmax, centre = bm.records(kind, real, *arrays)
    n = centre.shape[0]
    i = np.arange(n)
    validate_bvh(nodes, idx, np.concatenate([bmin, bmax]), np.stack([i, n + i, n + i], 1), min_leaf=min_leaf, max_depth=max_depth)
    return validate_bvh(nodes, idx, centre, np.stack([i, i, i], 1), min_leaf=min_leaf, max_depth=max_depth, exact_bounds=False,
                        low_side_first=True)

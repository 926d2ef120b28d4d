"""Fingerprints of GPU-built trees (node array + index permutation) over a spread of meshes, precisions and build options:
a builder refactor that is meant to change nothing must reproduce every line.  Usage: python tools/tree_hash.py
(numpy_meshes() is imported by tests/builder_model.py, which rebuilds the soup60k and grid9k lines on the CPU.)"""
import hashlib, sys
import numpy as np
OPTIONS = ((4, 64, 256), (1, 8, 256), (16, 200, 12))  # (min_leaf_primitives, bin_size, max_tree_depth)


def numpy_meshes():
    """The two meshes that need nothing but numpy, {"soup60k": (v, f), "grid9k": (v, f)}: one generator, drawn in this order."""
    rng = np.random.default_rng(3)
    v = rng.normal(size=(20000, 3)).astype(np.float32); f = rng.integers(0, 20000, size=(60000, 3)).astype(np.uint32)
    g = rng.integers(-6, 7, size=(3000, 3)).astype(np.float32); gf = rng.integers(0, 3000, size=(9000, 3)).astype(np.uint32)
    return {"soup60k": (v, f), "grid9k": (g, gf)}


if __name__ == "__main__":
    sys.path.insert(0, '.')
    from nanort_amd import BVHAccel, TriangleMesh, SphereGeometry, scenes
    from nanort_amd.wire import default_build_options
    cases = [("plane1M", scenes.plane(1000, 500)), ("sphere70k", scenes.sphere()), ("plane300x150", scenes.plane(300, 150))]
    cases += list(numpy_meshes().items())
    for name, (v, f) in cases:
        for real in (np.float32, np.float64):
            for ml, bins, md in OPTIONS:
                if name == "plane1M" and (real is np.float64 or ml != 4):
                    continue
                bo = default_build_options(real); bo["min_leaf_primitives"] = ml; bo["bin_size"] = bins; bo["max_tree_depth"] = md
                a = BVHAccel(real); assert a.Build(f.shape[0], TriangleMesh(v.astype(real), f), bo)
                nodes, idx = a.GetTree()
                print(name, real.__name__, ml, bins, md, nodes.shape[0], hashlib.md5(nodes.tobytes() + idx.tobytes()).hexdigest(), flush=True)
    c, r = scenes.random_spheres(50000)
    a = BVHAccel(np.float32); assert a.Build(50000, SphereGeometry(c, r)); nodes, idx = a.GetTree()
    print("spheres50k", nodes.shape[0], hashlib.md5(nodes.tobytes() + idx.tobytes()).hexdigest())

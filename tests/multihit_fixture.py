"""Multi-hit test fixtures: the CPU model of tests/multihit_model.c (compiled into a temporary directory), its ray sets and
the tie check shared by tests/test_multihit_model.py and tests/test_gpu_multihit.py."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from oracle.bindings import hit_dtype, node_dtype, ray_dtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def model_lib():
    """gcc -O2 -ffp-contract=off -fno-fast-math -shared -fPIC tests/multihit_model.c -I oracle, once per process."""
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="nrt_multihit_model_")
        so = os.path.join(d, "libmultihit_model.so")
        r = subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-I", os.path.join(ROOT, "oracle"),
                            "-o", so, os.path.join(ROOT, "tests", "multihit_model.c"), "-lm"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        L = ctypes.CDLL(so)
        vp, u32, u64, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
        for s in ("f32", "f64"):
            f = getattr(L, "mh_traverse_" + s)
            f.argtypes = [vp, vp, vp, sz, vp, vp, u64, vp, u32, vp, vp]
            f.restype = None
            g = getattr(L, "mh_brute_" + s)
            g.argtypes = [u32, vp, sz, vp, vp, u64, vp, u32, vp, vp]
            g.restype = None
        _LIB = L
    return _LIB


def _suffix(real):
    return "f32" if np.dtype(real) == np.float32 else "f64"


def _opts(o):
    return None if o is None else np.ascontiguousarray(np.asarray(o).reshape(1)).view(np.uint32).copy()


def model(nodes, indices, verts, faces, rays, K, opts=None, stride=None):
    """The contract's walk over (nodes, indices): (hits[n, K], counts[n]) as the library returns them."""
    real = verts.dtype
    assert nodes.dtype == node_dtype(real) and rays.dtype == ray_dtype(real)
    nodes, rays = np.ascontiguousarray(nodes), np.ascontiguousarray(rays)
    indices, faces = np.ascontiguousarray(indices, dtype=np.uint32), np.ascontiguousarray(faces, dtype=np.uint32)
    n = rays.shape[0]
    hits = np.zeros((n, K), dtype=hit_dtype(real))
    counts = np.zeros((n,), dtype=np.uint32)
    o = _opts(opts)
    getattr(model_lib(), "mh_traverse_" + _suffix(real))(_p(nodes), _p(indices), _p(verts), stride or 3 * verts.dtype.itemsize, _p(faces),
                                                          _p(rays), n, _p(o), K, _p(hits), _p(counts))
    return hits, counts


def brute(verts, faces, rays, K, opts=None, stride=None):
    """Every primitive against B = max_t, candidates sorted by (t, prim_id), the first K."""
    real = verts.dtype
    rays = np.ascontiguousarray(rays)
    faces = np.ascontiguousarray(faces, dtype=np.uint32)
    n = rays.shape[0]
    hits = np.zeros((n, K), dtype=hit_dtype(real))
    counts = np.zeros((n,), dtype=np.uint32)
    o = _opts(opts)
    getattr(model_lib(), "mh_brute_" + _suffix(real))(faces.shape[0], _p(verts), stride or 3 * verts.dtype.itemsize, _p(faces), _p(rays), n,
                                                       _p(o), K, _p(hits), _p(counts))
    return hits, counts


def hits_bytes(h):
    """Every field of every record (fp64 records: the padding left out)."""
    return b"".join(np.ascontiguousarray(h[k]).tobytes() for k in h.dtype.names)


def soup(real, seed=7):
    """tests/test_gpu_traverse.py's random soup: lattice vertices (exact edge hits), degenerate triangles, strided vertices."""
    rng = np.random.default_rng(seed)
    nv, nf, se = 1500, 5000, 4
    vbuf = rng.uniform(-1, 1, size=(nv, se)).astype(real)
    vbuf[:50, :3] = np.round(vbuf[:50, :3] * 4) / 4
    faces = rng.integers(0, nv, size=(nf, 3), dtype=np.uint32)
    faces[:20, 1] = faces[:20, 0]
    return vbuf, faces, se * vbuf.dtype.itemsize


def hostile_rays(real, n, seed=7):
    """... and its rays: zero direction components, axis-aligned, lattice origins, tiny and short [min_t, max_t] windows."""
    rng = np.random.default_rng(seed + 1)
    rays = np.zeros((n,), dtype=ray_dtype(real))
    rays["org"] = rng.uniform(-2, 2, size=(n, 3))
    rays["org"][: n // 7] = np.round(rays["org"][: n // 7] * 4) / 4
    d = rng.normal(size=(n, 3))
    k = n // 20
    d[:k, 0] = 0.0
    d[k:2 * k, 1] = 0.0
    d[2 * k:3 * k, :2] = 0.0
    d[3 * k:4 * k] = np.round(d[3 * k:4 * k])
    d[np.all(d == 0, axis=1)] = (0, 0, 1)
    d[4 * k:5 * k, 2] = 1e-9
    rays["dir"] = d
    rays["max_t"] = rng.choice([1e30, 0.5, 3.0], size=n)
    rays["min_t"] = rng.choice([0.0, 1e-3, 0.4], size=n)
    return rays


def random_window_rays(rays, seed):
    """The same rays with random [min_t, max_t] windows."""
    rng = np.random.default_rng(seed)
    r = rays.copy()
    a = rng.uniform(0, 4, size=r.shape[0])
    b = a + rng.uniform(0, 8, size=r.shape[0])
    r["min_t"], r["max_t"] = a, b
    return r


def check_k1_against_closest(h1, c1, ch, cm, ties_ok):
    """K = 1 against a closest-hit result (records ch, flags cm): the flag equal and t bit-identical on every ray; prim / u / v
    equal except on rays where ties_ok confirms that another candidate has exactly the same t (there t is equal as a number: a
    tie of -0 and +0 names the sign of the primitive each side names).  Returns the number of such rays."""
    h1 = h1[:, 0]
    assert np.array_equal(c1.astype(np.uint8), cm.astype(np.uint8))
    same = h1["prim_id"] == ch["prim_id"]
    for k in ("t", "u", "v"):
        assert np.ascontiguousarray(h1[k][same]).tobytes() == np.ascontiguousarray(ch[k][same]).tobytes(), k
    diff = np.nonzero(~same)[0]
    if diff.size:
        assert np.array_equal(h1["t"][diff], ch["t"][diff])
        tz = h1["t"][diff] != 0
        assert np.ascontiguousarray(h1["t"][diff][tz]).tobytes() == np.ascontiguousarray(ch["t"][diff][tz]).tobytes()
        ties_ok(diff, h1[diff], ch[diff])
    return diff.size


def tie_checker(verts, faces, rays, opts=None, stride=None):
    """Rays whose K = 1 prim_id differs from closest hit's: the brute-force enumeration must show both primitives as candidates
    at exactly that t, with the multi-hit one the smaller id."""
    def check(idx, mh, ch):
        bh, bc = brute(verts, faces, rays[idx], 64, opts, stride)
        for j in range(idx.size):
            row = bh[j, : bc[j]]
            at_t = row["prim_id"][row["t"] == mh["t"][j]]
            assert mh["prim_id"][j] in at_t and ch["prim_id"][j] in at_t, (idx[j], mh[j], ch[j])
            assert mh["prim_id"][j] < ch["prim_id"][j] and mh["prim_id"][j] == at_t.min()
    return check


def header_check(tmp_dir, v, f, rays, K, backend=False):
    """tests/cpp/multihit_check.cc compiled against include/nanort.h (host build, or -DNANORT_USE_HIP_BACKEND) and run once:
    (counts, rows[n, K], nodes, indices[, batch counts, batch rows])."""
    from oracle.bindings import hit_dtype as hd, node_dtype as nd

    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "nanort_amd", "lib")
    exe = os.path.join(tmp_dir, "multihit_check" + ("_hip" if backend else ""))
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I", inc, os.path.join(ROOT, "tests", "cpp", "multihit_check.cc"), "-o", exe]
    if backend:
        cmd += ["-DNANORT_USE_HIP_BACKEND", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include", "-L", libdir, "-lnanort_hip",
                "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    mesh, rp, out = (os.path.join(tmp_dir, x) for x in ("mesh.bin", "rays.bin", "out.bin"))
    with open(mesh, "wb") as fp:
        fp.write(np.array([v.shape[0], f.shape[0]], dtype=np.uint32).tobytes())
        fp.write(np.ascontiguousarray(v, dtype=np.float32).tobytes())
        fp.write(np.ascontiguousarray(f, dtype=np.uint32).tobytes())
    with open(rp, "wb") as fp:
        fp.write(np.array([rays.shape[0]], dtype=np.uint64).tobytes())
        fp.write(np.ascontiguousarray(rays).tobytes())
    r = subprocess.run([exe, mesh, rp, str(K), out] + (["batch"] if backend else []), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    raw = open(out, "rb").read()
    n, H, N = rays.shape[0], hd(np.float32), nd(np.float32)
    o = 0
    counts = np.frombuffer(raw, dtype=np.uint32, count=n, offset=o)
    o += 4 * n
    rows = np.frombuffer(raw, dtype=H, count=n * K, offset=o).reshape(n, K)
    o += n * K * H.itemsize
    nn = int(np.frombuffer(raw, dtype=np.uint64, count=1, offset=o)[0])
    o += 8
    nodes = np.frombuffer(raw, dtype=N, count=nn, offset=o)
    o += nn * N.itemsize
    idx = np.frombuffer(raw, dtype=np.uint32, count=f.shape[0], offset=o)
    o += 4 * f.shape[0]
    if not backend:
        return counts, rows, nodes, idx
    bcounts = np.frombuffer(raw, dtype=np.uint32, count=n, offset=o)
    o += 4 * n
    brows = np.frombuffer(raw, dtype=H, count=n * K, offset=o).reshape(n, K)
    return counts, rows, nodes, idx, bcounts, brows

"""Motion-blur test fixtures (include/nanort_hip.h, "motion blur"), shared by tests/test_motion_model.py on the
CPU and tests/test_gpu_motion.py on the GPU: the vertex rule of include/nanort_motion.h restated in numpy (numpy rounds every
float32 / float64 operation on its own, as the device and the host header do), the expectation built from it — the project's pinned
restatement of the reference (oracle.traverse) over vertices interpolated to each distinct time — the keyframe-1 deformations, and a
per-ray time assignment in which neighbouring rays never share a time."""
import numpy as np

from nanort_amd.wire import hit_dtype

# The ten times of the contract's corners: the two keyframes, inner points (1/3 is inexact in both precisions), the largest value
# below 1, and everything the clamp folds: -0.0, a negative, a value above 1, NaN.
TIME_VALUES = (0.0, 1.0, 0.5, 0.25, 1.0 / 3.0, float(np.nextafter(np.float32(1.0), np.float32(0.0))), -0.0, -1.0, 2.0, float("nan"))


def clamp_times(times, real):
    """s = (time > 0) ? (time < 1 ? time : 1) : 0, elementwise, in `real`."""
    t = np.asarray(times, dtype=real)
    one, zero = np.asarray(1, dtype=real), np.asarray(0, dtype=real)
    with np.errstate(invalid="ignore"):
        return np.where(t > zero, np.where(t < one, t, one), zero).astype(real)


def lerp(v0, v1, s):
    """The vertices at shutter time `s` (one clamped value): x = (1 - s) * a + s * b, then clamped into [min(a, b), max(a, b)] per
    component; every operation in the arrays' own precision."""
    real = v0.dtype
    assert v1.dtype == real and v0.shape == v1.shape
    s = np.asarray(s, dtype=real)
    one = np.asarray(1, dtype=real)
    a, b = v0, v1
    lo = np.where(b < a, b, a)
    hi = np.where(a < b, b, a)
    x = ((one - s) * a).astype(real) + (s * b).astype(real)
    x = x.astype(real)
    return np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(real)


def expected(oracle, nodes, idx, v0, v1, f, rays, times, opts=None):
    """(hits, mask) a motion query must return: rays grouped by the bit pattern of their clamped time, each group traced by the
    oracle over (nodes, idx) and the vertices interpolated to that time.  times None: every ray at time 0."""
    real = v0.dtype
    n = rays.shape[0]
    hits = np.zeros(n, dtype=hit_dtype(real))
    mask = np.zeros(n, dtype=np.uint8)
    s = clamp_times(np.zeros(n) if times is None else times, real)
    bits = s.view(np.uint32 if real == np.float32 else np.uint64)
    for b in np.unique(bits):
        sel = np.nonzero(bits == b)[0]
        h, m = oracle.traverse(nodes, idx, lerp(v0, v1, s[sel[0]]), f, np.ascontiguousarray(rays[sel]), opts)
        hits[sel], mask[sel] = h, m
    return hits, mask


def assign_times(n, real, seed=3):
    """One of TIME_VALUES per ray, pseudo-random, consecutive rays always different: the lanes of a wave differ, and a lane refilled
    with the next ray of its chunk must pick up that ray's own time."""
    rng = np.random.default_rng(seed)
    k = len(TIME_VALUES)
    step = rng.integers(1, k, size=n)  # 1 .. k - 1: never the predecessor's value
    step[0] = rng.integers(0, k)
    which = np.cumsum(step) % k
    t = np.asarray(TIME_VALUES, dtype=real)[which]
    assert n < 2 or (which[1:] != which[:-1]).all()
    return np.ascontiguousarray(t)


# Amplitudes of the two deformations the fixture condition is asserted for (test_motion_model.py): chosen so that at time 0.5 well
# over a tenth of C1's camera rays see something that is neither keyframe (measured with the oracle: wave 39 %, which is every ray
# that hits; translate 95 %).  The translation is along the view axis, towards the camera at z = 20, by more than the mesh's depth
# (z in [-4.96, 4.79]): keyframe 1 lies wholly outside keyframe 0's bounds and is still in front of the camera.
TRANSLATE = (0.0, 0.0, 11.0)
WAVE_AMPLITUDE = 0.5


def deformations(v):
    """name -> keyframe 1: a small jitter, a rigid translation far outside the old bounds, a wave, a fifth of the vertices collapsed to
    a point, and keyframe 0 itself."""
    rng = np.random.default_rng(11)
    real = v.dtype
    c = v.mean(axis=0)
    out = {}
    out["jitter"] = (v + rng.normal(scale=1e-3, size=v.shape)).astype(real)
    out["translate"] = (v + np.array(TRANSLATE)).astype(real)
    w = v.astype(np.float64).copy()
    w[:, 1] += WAVE_AMPLITUDE * np.sin(3.0 * w[:, 0]) * np.cos(2.0 * w[:, 2])
    out["wave"] = w.astype(real)
    col = v.copy()
    k = rng.choice(v.shape[0], size=max(1, v.shape[0] // 5), replace=False)
    col[k] = c.astype(real)
    out["collapse"] = col
    out["same"] = v.copy()
    return {name: np.ascontiguousarray(a) for name, a in out.items()}


def differs(ha, ma, hb, mb):
    """Per ray: the two results differ in some bit of some field or in the flag."""
    d = ma != mb
    for k in ha.dtype.names:
        x, y = np.ascontiguousarray(ha[k]), np.ascontiguousarray(hb[k])
        bits = np.uint32 if x.dtype.itemsize == 4 else np.uint64
        d = d | (x.view(bits) != y.view(bits))
    return d


def time_matters_share(oracle, nodes, idx, v0, v1, f, rays, s=0.5):
    """Share of the rays whose record at time `s` differs from the record at time 0 AND from the record at time 1 (the fixture
    condition: a walk that ignored, truncated or mis-indexed the time would be seen)."""
    n = rays.shape[0]
    real = v0.dtype
    hs, ms = expected(oracle, nodes, idx, v0, v1, f, rays, np.full(n, s, dtype=real))
    h0, m0 = expected(oracle, nodes, idx, v0, v1, f, rays, np.zeros(n, dtype=real))
    h1, m1 = expected(oracle, nodes, idx, v0, v1, f, rays, np.ones(n, dtype=real))
    return float((differs(hs, ms, h0, m0) & differs(hs, ms, h1, m1)).mean())


def motion_boxes(refit, nodes, idx, v0, v1, f):
    """The node array with every box the elementwise min / max of tests/refit_model.py's refit over keyframe 0 and over keyframe 1."""
    a, b = refit(nodes, idx, v0, f), refit(nodes, idx, v1, f)
    out = a.copy()
    out["bmin"] = np.minimum(a["bmin"], b["bmin"])
    out["bmax"] = np.maximum(a["bmax"], b["bmax"])
    return out

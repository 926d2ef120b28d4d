"""The three "own walk" kernels — multi-hit, motion, masked (nanort_amd/csrc/own_walks.hip) — where the plain
walk is tested, and the launch path only they take (api_query.hip, own_walk()): 32 LDS stack entries and then the slot's spill array,
no completion record, the slot closed by an event, a taken-over slot waited for with hipStreamWaitEvent.

  a. the masked walk on a tree deeper than its LDS stack;
  b. the masked and the motion walk over the random soup and its hostile rays (zero direction components, axis-aligned rays, lattice
     origins and exact edge hits, degenerate faces, tiny windows);
  c. masks on a context that holds a motion keyframe, through a change of the keyframe that changes the leaf order;
  d. every kind of launch mixed on more streams than the context has launch slots, with ray counts that grow the slots' spill arrays
     while launches are in flight, and the setters right behind such a burst;
  e. the staged host forms of every kind from four threads.

a to c are exact against the oracle over the context's own node array (masks_fixture.expected, motion_fixture.expected): every field
of every record, no tolerance.  d and e compare with the serial host forms of the same queries, which a to c tie to the oracle.  The
fixture conditions (tests/own_walks_fixture.py) hold for the reference alone; tests/test_masks_model.py and tests/test_motion_model.py
assert them without a GPU."""
import faulthandler
import sys
import threading

import numpy as np
import pytest

import masks_fixture as kf
import motion_fixture as mf
import own_walks_fixture as ow
from helpers import assert_hits_identical, trace_options
from multihit_fixture import hits_bytes
from nanort_amd import BVHAccel, MotionTriangleMesh, TriangleMesh
from nanort_amd.capi import NRT_ERR_INVALID, NrtError
from nanort_amd.wire import hit_dtype

pytestmark = pytest.mark.gpu

REALS = [np.float32, np.float64]
IDS = ["f32", "f64"]
ALL_OPTIONS = dict(range_=(50, 900), skip=412, cull=True)  # (test_gpu_masks.py, OPTIONS["all"])
K = 3
FILE_TIME_LIMIT_S = 120  # the whole file runs in about ten seconds


@pytest.fixture(scope="module", autouse=True)
def file_time_limit():
    """The file mixes streams, launch slots, events and host threads: a wait that never ends among them would hang the suite.  Past
    the limit every thread's stack is written out and the process ends."""
    faulthandler.dump_traceback_later(FILE_TIME_LIMIT_S, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()


def _c(real):
    return "float" if np.dtype(real) == np.float32 else "double"


def check_masked(oracle, a, real, v, f, pm, rays, words, opts=None, stride=None):
    """Masked closest hit and occlusion against the expectation over the accel's own tree; returns the expected flags."""
    nodes, idx = a.GetTree()
    eh, em = kf.expected(oracle, nodes, idx, v, f, pm, rays, words, opts, stride=stride)
    h, m = a.TraverseBatchMasked(rays, words, opts)
    assert a.LastKernelName() == "nrt::k_traverse_masked<%s>" % _c(real)
    assert_hits_identical(eh, em, h, m)
    assert np.array_equal(a.OccludedBatchMasked(rays, words, opts), em)
    assert a.LastKernelName() == "nrt::k_traverse_masked<%s>" % _c(real)
    return em


def check_motion(oracle, a, real, v0, v1, f, rays, times, opts=None):
    nodes, idx = a.GetTree()
    eh, em = mf.expected(oracle, nodes, idx, v0, v1, f, rays, times, opts)
    h, m = a.TraverseBatchMotion(rays, times, opts)
    assert a.LastKernelName() == "nrt::k_traverse_motion<%s>" % _c(real)
    assert_hits_identical(eh, em, h, m)
    assert np.array_equal(a.OccludedBatchMotion(rays, times, opts), em)
    return em


def refused(call):
    with pytest.raises(NrtError) as e:
        call()
    assert e.value.status == NRT_ERR_INVALID, e.value


# ---- a. the masked walk past the LDS stack -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_masked_walk_past_the_lds_stack(oracle, real):
    """The reference's tree over the pile is 138 deep and every ray's walk holds 137 entries, whatever it sees: 105 past the LDS
    entries, in the slot's spill array.  A ray that does not see its first triangles walks on to one it sees."""
    v, f, rays, words = ow.pile(real)
    nodes, idx, _ = oracle.build(v, f)
    a = BVHAccel(real)
    a.SetMesh(TriangleMesh(v, f))
    a.SetTree(nodes, idx)
    pats = kf.prim_patterns(f.shape[0])
    for name in ("random", "mod3"):
        pm = pats[name]
        a.SetPrimMasks(pm)
        _, _, depth, hits, other = ow.masked_figures(oracle, nodes, idx, v, f, pm, rays, words)
        assert len(depth) == len(kf.RAY_MASK_VALUES) and min(depth.values()) > ow.PILE_MIN_STACK, depth
        assert hits > 0
        if name == "random":
            assert other >= ow.PILE_MIN_OTHER, other
        for o in (None, trace_options(**ALL_OPTIONS)):
            if o is not None:  # (the id range, the skip id and culling reject hits, never nodes: the stack is as deep)
                _, _, depth = kf.expected(oracle, nodes, idx, v, f, pm, rays, words, o, count=True)
                assert min(depth.values()) > ow.PILE_MIN_STACK, depth
            em = check_masked(oracle, a, real, v, f, pm, rays, words, o)
            assert em.sum() > 0
    a.close()


# ---- b. soup and hostile rays ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_masked_walk_over_the_soup_and_hostile_rays(oracle, real):
    vbuf, f, stride, rays, words, pm = ow.soup_masked(real)
    nodes, idx, _ = oracle.build(vbuf, f, stride=stride)
    _, _, _, hits, other = ow.masked_figures(oracle, nodes, idx, vbuf, f, pm, rays, words, stride)
    assert hits > 0 and other >= ow.SOUP_MIN_OTHER, (hits, other)
    a = BVHAccel(real)
    a.SetMesh(TriangleMesh(vbuf, f, stride))
    a.SetPrimMasks(pm)
    a.SetTree(nodes, idx)  # the reference's tree, adopted
    for o in (None, trace_options(cull=True)):
        check_masked(oracle, a, real, vbuf, f, pm, rays, words, o, stride)
    assert a.BuildCurrent()  # the builder's tree: another leaf order, the same words
    assert a.GetTree()[1].tobytes() != np.ascontiguousarray(idx).tobytes()
    for o in (None, trace_options(cull=True)):
        em = check_masked(oracle, a, real, vbuf, f, pm, rays, words, o, stride)
        assert em.sum() > 0
    a.close()


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_motion_walk_over_the_soup_and_hostile_rays(oracle, real):
    v0, v1, f, rays, times = ow.soup_motion(real)
    nodes, idx, _ = ow.motion_tree(oracle, v0, v1, f)
    _, _, hits, differ = ow.motion_figures(oracle, nodes, idx, v0, v1, f, rays, times)
    assert hits >= ow.SOUP_MOTION_MIN_HITS and differ >= ow.SOUP_MOTION_MIN_DIFFER, (hits, differ)
    a = BVHAccel(real)
    a.SetMesh(MotionTriangleMesh(v0, v1, f))
    a.SetTree(nodes, idx)
    for o in (None, trace_options(cull=True)):
        check_motion(oracle, a, real, v0, v1, f, rays, times, o)
    assert a.BuildCurrent()
    for o in (None, trace_options(cull=True)):
        em = check_motion(oracle, a, real, v0, v1, f, rays, times, o)
        assert em.sum() > 0
    a.close()


# ---- c. masks on a motion context --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_masks_on_a_motion_context_follow_its_leaf_order(oracle, real):
    """Masked queries on a context with a keyframe answer for keyframe 0 over the context's own (union-box) tree; the motion queries
    do not see the words; a new keyframe gives a new leaf order, and the words' leaf-order copy follows it with no call of the masks
    setter between; removing the keyframe keeps the masks; nrtSetMesh drops both."""
    v0, v1, f, rays, times = ow.soup_motion(real)
    words = kf.assign_ray_masks(rays.shape[0], seed=ow.SOUP_RAY_SEED)
    pm = kf.prim_patterns(f.shape[0])["mod3"]  # (not invariant under a permutation of the faces)
    a = BVHAccel(real)
    assert a.Build(f.shape[0], MotionTriangleMesh(v0, v1, f))
    bare = a.TraverseBatchMotion(rays, times), a.OccludedBatchMotion(rays, times)
    a.SetPrimMasks(pm)
    assert check_masked(oracle, a, real, v0, f, pm, rays, words).sum() > 0
    check_masked(oracle, a, real, v0, f, pm, rays, words, trace_options(cull=True))
    (h, m), occ = a.TraverseBatchMotion(rays, times), a.OccludedBatchMotion(rays, times)
    assert h.tobytes() == bare[0][0].tobytes() and m.tobytes() == bare[0][1].tobytes() and occ.tobytes() == bare[1].tobytes()
    assert m.sum() > 0
    idx_a = a.GetTree()[1]
    # another keyframe 1, far from the first: other union boxes, other splits, another leaf order
    rng = np.random.default_rng(31)
    v1b = np.ascontiguousarray((v0 + rng.uniform(-0.75, 0.75, size=v0.shape)).astype(real))
    a.SetMeshMotion(v1b)
    assert not a.IsValid()
    assert a.BuildCurrent()
    idx_b = a.GetTree()[1]
    assert idx_b.shape == idx_a.shape and idx_b.tobytes() != idx_a.tobytes(), "fixture: the new keyframe leaves the leaf order as it was"
    assert check_masked(oracle, a, real, v0, f, pm, rays, words).sum() > 0
    check_motion(oracle, a, real, v0, v1b, f, rays, times)
    # the keyframe removed: a plain tree, a third leaf order; the masks are still there
    a.SetMeshMotion(None)
    assert a.BuildCurrent()
    assert a.GetTree()[1].tobytes() != idx_b.tobytes()
    assert check_masked(oracle, a, real, v0, f, pm, rays, words).sum() > 0
    refused(lambda: a.TraverseBatchMotion(rays, times))
    # nrtSetMesh drops the keyframe and the masks
    a.SetMeshMotion(v1)
    a.SetMesh(TriangleMesh(v0, f))
    assert a.BuildCurrent()
    refused(lambda: a.TraverseBatchMasked(rays, words))
    refused(lambda: a.TraverseBatchMotion(rays, times))
    a.close()


# ---- d, e. one context, every kind ---------------------------------------------------------------------------------------------------
KINDS = ["closest", "occlusion", "multihit", "masked", "masked occlusion", "motion", "motion occlusion"]
OWN_KERNEL = {"multihit": "multihit", "masked": "masked", "masked occlusion": "masked", "motion": "motion", "motion occlusion": "motion"}


class Pile:
    """The pile of (a) with a second keyframe, the reference's tree with union boxes, random prim words: every own-walk launch goes
    past its LDS stack entries.  accel(): a context that holds all of it."""

    def __init__(self, oracle, real):
        self.real = real
        self.v, self.f, self.rays, self.words = ow.pile(real)
        self.v1 = ow.pile_keyframe1(self.v)
        self.nodes, self.idx, st = ow.motion_tree(oracle, self.v, self.v1, self.f)
        self.pm = kf.random_prim_masks(self.f.shape[0])
        self.times = mf.assign_times(self.rays.shape[0], real)
        _, _, cnt = oracle.traverse(self.nodes, self.idx, self.v, self.f, self.rays, count=True)
        assert st["max_tree_depth"] > ow.PILE_MIN_STACK and cnt[3] > ow.PILE_MIN_STACK

    def accel(self):
        a = BVHAccel(self.real)
        a.SetMesh(MotionTriangleMesh(self.v, self.v1, self.f))
        a.SetTree(self.nodes, self.idx)
        a.SetPrimMasks(self.pm)
        return a


def host_query(a, kind, rays, words, times, skip=None):
    """(records or None, flags / counts) of the host form."""
    if kind == "closest":
        return a.TraverseBatch(rays, skip_prim_ids=skip)
    if kind == "occlusion":
        return None, a.OccludedBatch(rays)
    if kind == "multihit":
        return a.MultiHitTraverseBatch(rays, K)
    if kind == "masked":
        return a.TraverseBatchMasked(rays, words)
    if kind == "masked occlusion":
        return None, a.OccludedBatchMasked(rays, words)
    if kind == "motion":
        return a.TraverseBatchMotion(rays, times)
    assert kind == "motion occlusion"
    return None, a.OccludedBatchMotion(rays, times)


def same_result(want, got, what):
    (wh, wf), (gh, gf) = want, got
    assert (wh is None) == (gh is None), what
    if wh is not None:
        assert gh.shape == wh.shape and hits_bytes(gh) == hits_bytes(wh), what  # (every field; fp64 records carry 4 padding bytes)
    assert gf.dtype == wf.dtype and gf.tobytes() == wf.tobytes(), what


class Burst:
    """24 Device launches on six streams, the kinds in rotation, ray counts ascending from 64 to all of the pile's rays.  Seven kinds
    over six streams over four slots: every slot is taken over from record-closed and from event-closed launches, and alternates
    between the two itself."""
    LAUNCHES, STREAMS = 24, 6

    def __init__(self, p):
        import torch

        self.torch, self.p = torch, p
        self.hit_t = hit_dtype(p.real)
        n_all = p.rays.shape[0]
        self.counts = [64 + (n_all - 64) * k // (self.LAUNCHES - 1) for k in range(self.LAUNCHES)]
        assert self.counts[0] == 64 and self.counts[-1] == n_all and all(a < b for a, b in zip(self.counts, self.counts[1:]))
        self.kinds = [KINDS[k % len(KINDS)] for k in range(self.LAUNCHES)]
        self.streams = [torch.cuda.Stream() for _ in range(self.STREAMS)]
        self.d_rays = torch.from_numpy(p.rays.view(np.uint8).copy()).cuda()
        self.d_words = torch.from_numpy(p.words.view(np.int32).copy()).cuda()
        self.d_times = torch.from_numpy(p.times.copy()).cuda()
        self.outs = []

    def expectation(self, a):
        """The serial host forms of the same queries."""
        p = self.p
        return [host_query(a, kind, p.rays[:n], p.words[:n], p.times[:n]) for kind, n in zip(self.kinds, self.counts)]

    def fill(self):
        """Fresh outputs, every byte a pattern no result holds: an unwritten record shows."""
        torch = self.torch
        self.outs = []
        for kind, n in zip(self.kinds, self.counts):
            per_ray = K if kind == "multihit" else 1
            d_h = None if kind.endswith("occlusion") else torch.full((n * per_ray * self.hit_t.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
            d_f = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if kind == "multihit" else torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
            self.outs.append((d_h, d_f))
        torch.cuda.synchronize()

    def issue(self, a):
        """Back to back, no host synchronisation between the launches."""
        p, rsz = self.p, self.p.rays.dtype.itemsize
        for k, (kind, n, (d_h, d_f)) in enumerate(zip(self.kinds, self.counts, self.outs)):
            s = self.streams[k % self.STREAMS]
            d_r, d_w, d_t = self.d_rays[: n * rsz], self.d_words[:n], self.d_times[:n]
            if kind == "closest":
                a.TraverseBatchDevice(d_r, d_h, d_f, stream=s)
            elif kind == "occlusion":
                a.OccludedBatchDevice(d_r, d_f, stream=s)
            elif kind == "multihit":
                a.MultiHitTraverseBatchDevice(d_r, K, d_h, d_f, stream=s)
            elif kind == "masked":
                a.TraverseBatchMaskedDevice(d_r, d_w, d_h, d_f, stream=s)
            elif kind == "masked occlusion":
                a.OccludedBatchMaskedDevice(d_r, d_w, d_f, stream=s)
            elif kind == "motion":
                a.TraverseBatchMotionDevice(d_r, d_t, d_h, d_f, stream=s)
            else:
                a.OccludedBatchMotionDevice(d_r, d_t, d_f, stream=s)
            if kind in OWN_KERNEL:
                assert a.LastKernelName() == "nrt::k_traverse_%s<%s>" % (OWN_KERNEL[kind], _c(p.real))

    def results(self):
        out = []
        for kind, n, (d_h, d_f) in zip(self.kinds, self.counts, self.outs):
            h = None
            if d_h is not None:
                h = np.frombuffer(d_h.cpu().numpy().tobytes(), dtype=self.hit_t)
                h = h.reshape(n, K) if kind == "multihit" else h
            fl = d_f.cpu().numpy()
            out.append((h, fl.view(np.uint32) if kind == "multihit" else fl))
        return out


@pytest.mark.parametrize("real", REALS, ids=IDS)
def test_mixed_kinds_on_more_streams_than_slots(oracle, real):
    import torch

    p = Pile(oracle, real)
    ref, a = p.accel(), p.accel()  # (the burst's context starts with fresh slots: its spill arrays grow during the burst)
    b = Burst(p)
    want = b.expectation(ref)
    for (wh, wf), kind in zip(want, b.kinds):
        assert wf.any(), kind  # (not vacuous: every launch has hits)
    b.fill()
    b.issue(a)
    torch.cuda.synchronize()
    for k, (w, g) in enumerate(zip(want, b.results())):
        same_result(w, g, "launch %d (%s, %d rays)" % (k, b.kinds[k], b.counts[k]))
    # the setters right behind a burst wait for it: new words, then the builder's tree (another leaf order, other boxes) — the
    # launches in flight read the words' leaf-order copy and the tree's arrays, all of which the two calls rewrite in place
    other = kf.prim_patterns(p.f.shape[0])["mod3"]
    b.fill()
    b.issue(a)
    a.SetPrimMasks(other)
    assert a.BuildCurrent()
    torch.cuda.synchronize()
    for k, (w, g) in enumerate(zip(want, b.results())):
        same_result(w, g, "second burst, launch %d (%s, %d rays)" % (k, b.kinds[k], b.counts[k]))
    assert a.GetTree()[1].tobytes() != np.ascontiguousarray(p.idx).tobytes()
    # ... and the context answers for the new words on the new tree
    assert check_masked(oracle, a, real, p.v, p.f, other, p.rays, p.words).sum() > 0
    ref.close()
    a.close()


def test_host_forms_of_every_kind_from_four_threads(oracle):
    """Four threads, three rounds each over the five host forms (plain, masked, motion, multi-hit, per-ray skip ids) on ONE context: they
    share st_rays / st_hits / st_mask and st_times, st_ray_masks, st_skip under host_mutex, regrown from round to round (257, 1500,
    4093 rays) and reused across the kinds.  Every result equals the single-threaded one."""
    p = Pile(oracle, np.float32)
    a = p.accel()
    rounds = (257, 1500, 4093)
    kinds = ("closest", "masked", "motion", "multihit", "skip")
    n_all = p.rays.shape[0]
    closest_ids = a.TraverseBatch(p.rays)[0]["prim_id"].copy()  # a ray's skip id is the triangle it would hit: it hits the next one

    def inputs(t, n):
        """Thread t's rays of a round: the pile's set from another start, so no two threads ask the same thing."""
        sel = (np.arange(n) + 97 * t) % n_all
        return np.ascontiguousarray(p.rays[sel]), np.ascontiguousarray(p.words[sel]), np.ascontiguousarray(p.times[sel]), np.ascontiguousarray(closest_ids[sel])

    def ask(kind, rays, words, times, skip):
        return host_query(a, "closest", rays, words, times, skip) if kind == "skip" else host_query(a, kind, rays, words, times)

    want = {(t, n, kind): ask(kind, *inputs(t, n)) for t in range(4) for n in rounds for kind in kinds}
    h0, m0 = want[(0, 1500, "closest")]
    hs, ms = want[(0, 1500, "skip")]
    assert m0.all() and (hs["prim_id"] != h0["prim_id"]).all()  # (the skip ids matter: no ray may report the triangle it skips)
    errors = []

    def work(t):
        try:
            for n in rounds:
                args = inputs(t, n)
                for kind in kinds:
                    same_result(want[(t, n, kind)], ask(kind, *args), "thread %d, %d rays, %s" % (t, n, kind))
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    a.close()

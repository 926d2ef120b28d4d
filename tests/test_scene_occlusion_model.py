"""CPU model of the occlusion form of the single-pass scene walk (nanort_amd/csrc/scene_kernels.hip, k_scene_walk<.., ANY = true>) and
of its certificate, plus the interface checks of nrtSceneOccludedBatch*.

What the reference's flag is: of the instances whose boxes a ray enters, the 64 of smallest (entry distance, id) are listed
(kMaxIntersections); the flag is 1 iff one of those has a local hit.  The walk meets the entered instances in an order of its
own, keeps no list, and decides per ray:
  searching — until the first hit every instance it meets is opened (nothing may be skipped: skipping needs a hit);
  counting  — after the first hit, in instance h: nothing is opened any more; B = (instances opened before h) + (instances met
              later that rank before h) bounds the number of entered instances in front of h from above.  The walk may skip an
              instance entered strictly beyond e_h (it ranks behind h and would not count).  B >= 64 at any time: redo.
  end       — no hit: certified 0.  Hit and B < 64: certified 1.  A scene of at most 64 instances: the first hit is certified 1.
The model below does exactly that on abstract per-ray sets (entry distance with ties, id, "local walk hits"), in random visiting
orders with random legal skipping, and every certified answer must be the reference rule's; what is not certified is exactly what
goes to redo."""
import ctypes
import os
import random

import pytest

CAP = 64  # kMaxIntersections


def reference_flag(insts):
    """insts: (entry, id, hits).  Flag = any hit among the CAP smallest (entry, id)."""
    return int(any(h for _, _, h in sorted(insts, key=lambda x: (x[0], x[1]))[:CAP]))


def walk_model(insts, rng, scene_size, skip_prob=0.5):
    """The stop rule and certificate as k_scene_walk<ANY> implements them.  Returns (flag or None, redo)."""
    order = list(insts)
    rng.shuffle(order)
    traced = 0
    hit = None  # (entry, id) of the instance of the first hit
    bound = 0
    for e, k, h in order:
        if hit is None:  # searching: every entered instance is opened
            traced += 1
            if h:
                before = traced - 1
                if before >= CAP:
                    return None, True
                if scene_size <= CAP:
                    return 1, False
                hit = (e, k)
                bound = before
            continue
        # counting: an instance entered strictly beyond the hit's entry may be skipped (a subtree cull); it would not count
        if e > hit[0] and rng.random() < skip_prob:
            continue
        if (e, k) < hit:
            bound += 1
            if bound >= CAP:
                return None, True
    if hit is None:
        return 0, False
    assert bound < CAP
    return 1, False


def run(insts, rng, scene_size=None, orders=6):
    ref = reference_flag(insts)
    scene_size = len(insts) + 100 if scene_size is None else scene_size
    out = []
    for _ in range(orders):
        flag, redo = walk_model(insts, rng, scene_size, skip_prob=rng.choice([0.0, 0.5, 1.0]))
        assert (flag is None) == redo  # uncertified rays are exactly those sent to redo
        if flag is not None:
            assert flag == ref, (flag, ref, len(insts))
        out.append(flag)
    return ref, out


def random_set(rng, n, p_hit):
    ids = rng.sample(range(10 * n + 10), n)
    # entry distances from a small pool: deliberate ties (the id then decides the rank)
    return [(float(rng.randrange(0, max(2, n // 3 + 1))), k, rng.random() < p_hit) for k in ids]


def test_random_sets_every_certified_answer_is_the_reference_rule():
    rng = random.Random(7)
    certified = redo = 0
    for trial in range(1500):
        n = rng.randrange(0, 201)
        insts = random_set(rng, n, rng.choice([0.0, 0.01, 0.05, 0.3, 1.0]))
        small = rng.random() < 0.2 and n <= CAP
        _, out = run(insts, rng, scene_size=n if small else None)
        certified += sum(f is not None for f in out)
        redo += sum(f is None for f in out)
    assert certified > 0 and redo > 0  # both outcomes occur on this material


def test_no_hit_is_zero_whatever_number_of_boxes_was_entered():
    rng = random.Random(8)
    for n in (0, 1, 63, 64, 65, 200):
        insts = [(float(i % 7), i, False) for i in range(n)]
        ref, out = run(insts, rng)
        assert ref == 0 and out == [0] * len(out)


def test_only_hitting_instances_rank_behind_the_list():
    """The only hits rank >= 64: the reference answers 0; the walk may never certify 1."""
    rng = random.Random(9)
    for extra in (1, 5, 40):
        insts = [(float(i), i, False) for i in range(CAP)] + [(1000.0 + i, 500 + i, True) for i in range(extra)]
        ref, out = run(insts, rng, orders=40)
        assert ref == 0
        assert all(f is None for f in out)  # a hit was found, it cannot be certified: redo (the listing path answers 0)
    # the same with ties at the boundary: the 64th and 65th share an entry distance, the hitter has the higher id
    insts = [(1.0, i, False) for i in range(CAP)] + [(1.0, CAP, True)]
    ref, out = run(insts, rng, orders=40)
    assert ref == 0 and all(f is None for f in out)


@pytest.mark.parametrize("front", [63, 64, 65])
def test_exactly_63_64_65_boxes_in_front_of_the_hit(front):
    rng = random.Random(100 + front)
    insts = [(float(i % 9), i, False) for i in range(front)] + [(50.0, 900, True)] + [(60.0 + i, 1000 + i, False) for i in range(30)]
    ref, out = run(insts, rng, orders=60)
    assert ref == (1 if front < CAP else 0)
    if front >= CAP:
        assert all(f is None for f in out)  # never certified: redo
    else:
        assert all(f in (1, None) for f in out)  # (None: an order that opened many boxes before the hit — the bound is conservative)
    # a visiting order that meets the hit FIRST counts exactly the boxes in front of it
    first = [insts[front]] + insts[:front] + insts[front + 1:]
    flag, redo = walk_model(first, _NoShuffle(), len(insts) + 100, skip_prob=1.0)
    assert (flag, redo) == ((1, False) if front < CAP else (None, True))


class _NoShuffle:
    """A stand-in for random.Random that keeps the given order and never skips by chance."""

    def shuffle(self, x):
        pass

    def random(self):
        return 0.0


def test_scene_of_at_most_64_instances_ends_at_the_first_hit():
    rng = random.Random(12)
    for n in (1, 2, 64):
        for _ in range(50):
            insts = random_set(rng, n, 0.2)
            ref, out = run(insts, rng, scene_size=n)
            assert out == [ref] * len(out)  # always certified: every entered box is listed


# ---- the interface: both entry points exist, from the library up to the Python class ---------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_both_occlusion_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, "nanort_amd", "lib", "libnanort_hip.so"))
    for name in ("nrtSceneOccludedBatch_f32", "nrtSceneOccludedBatchDevice_f32"):
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "nanort_hip.h")).read()
    assert "NRT_API nrt_status nrtSceneOccludedBatch_f32(nrt_scene *scene, const nrt_ray_f32 *rays, uint64_t num_rays, uint8_t *mask_out);" in header
    assert "NRT_API nrt_status nrtSceneOccludedBatchDevice_f32(nrt_scene *scene, const nrt_ray_f32 *d_rays, uint64_t num_rays, uint8_t *d_mask_out);" in header


def test_scene_class_has_both_methods():
    from nanort_amd import Scene

    assert callable(getattr(Scene, "OccludedBatch", None)) and callable(getattr(Scene, "OccludedBatchDevice", None))

"""Scenes and ray sets of the occlusion-query tests of the sphere, cylinder and curve kinds (tests/test_gpu_occluded_kinds.py):
what sphere_fixture and curves_fixture describe, and — where a fixture's own rays hit or miss almost everywhere, as under one
strand of hair — rays from the curve example's eye aimed at and closely past the primitives themselves (a grid over the scene's
box with a margin meets a thin strand with a few rays in a hundred: measured, and not kept).  A mask of all zeros or all ones would hide a
failure: every set here was kept because at least a tenth of its rays hit and at least a tenth miss (the CPU oracles say so, and
the GPU tests assert it again)."""
import numpy as np

import curves_fixture as cf
import sphere_fixture
from nanort_amd import scenes


def mixed(flags):
    """At least a tenth of the rays hit and at least a tenth miss."""
    flags = np.asarray(flags)
    return flags.size >= 10 and 0.1 <= float((flags != 0).mean()) <= 0.9


def aimed_at(points, rho, k=4, span=2.0):
    """Rays from the eye of curves_fixture.camera(): for every point p with its radius rho, a k x k grid of targets over
    p + [-span * rho, span * rho]^2 in x and y — some through the primitive, some closely past it."""
    points, rho = np.asarray(points, dtype=np.float64).reshape(-1, 3), np.asarray(rho, dtype=np.float64).reshape(-1)
    off = np.linspace(-span, span, k)
    ox, oy = (a.reshape(-1) for a in np.meshgrid(off, off))
    target = np.repeat(points, k * k, axis=0)
    target[:, 0] += np.tile(ox, points.shape[0]) * np.repeat(rho, k * k)
    target[:, 1] += np.tile(oy, points.shape[0]) * np.repeat(rho, k * k)
    rays = np.repeat(cf.camera(1, 1), target.shape[0])
    d = target - rays["org"].astype(np.float64)
    rays["dir"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return rays


def bezier_points(cps, samples):
    """`samples` points along each cubic Bezier curve of cps (n, 4, 3), in float64: (n * samples, 3)."""
    t = ((np.arange(samples) + 0.5) / samples)[None, :, None]
    p = cps.astype(np.float64)[:, :, None, :]
    return ((1 - t) ** 3 * p[:, 0] + 3 * (1 - t) ** 2 * t * p[:, 1] + 3 * (1 - t) * t ** 2 * p[:, 2] + t ** 3 * p[:, 3]).reshape(-1, 3)


def sphere_cases():
    """(name, centres, radii, rays)"""
    c, r = sphere_fixture.scene()
    dc, dr = sphere_fixture.degenerate_spheres(400)
    out = [("scene_rays", c, r, sphere_fixture.rays()), ("scene_hostile", c, r, sphere_fixture.hostile_rays()),
           ("degenerate", dc, dr, sphere_fixture.hostile_rays())]
    for n in (1, 3):  # the root is a leaf
        at = aimed_at(np.repeat(c[:n], 64, axis=0), np.repeat(r[:n], 64) * np.tile(np.linspace(0.25, 1.0, 64), n))  # (grids of several widths)
        out.append(("n%d" % n, c[:n], r[:n], np.concatenate([at, sphere_fixture.hostile_rays()[:200]])))
    return out


def cylinder_cases():
    """(name, end points, radii, rays)"""
    return [("random3000", *scenes.random_cylinders(3000), sphere_fixture.rays()),
            ("degenerate", *sphere_fixture.degenerate_cylinders(400), sphere_fixture.hostile_rays())]


CURVE_SCENES = ("1", "2", "5", "64", "fur")


def curve_rays(scene):
    """curves_fixture.all_rays() where they are a mixed set (the fur); for the strands of "1", "2", "5" and "64", which the example's
    64 x 64 grid all but misses, rays aimed at points along the strands (their half radius is the tube's), then the hostile rays."""
    if scene == "fur":
        return cf.all_rays()
    cps, radii = cf.scene(scene)
    samples = max(4, 256 // radii.shape[0])
    return np.concatenate([aimed_at(bezier_points(cps, samples), np.repeat(0.5 * radii.max(axis=1), samples)), cf.hostile_rays()])

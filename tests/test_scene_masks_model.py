"""The expectation of the masked scene queries (tests/scene_masks_fixture.py) and the line fixture's bit layout, checked on the CPU
against the restatement alone: with all-ones words the expectation IS the plain restatement, byte for byte, and the fixture yields
every class the GPU test relies on — a blocker that ranks 71st, 65th, exactly 64th and 61st among the boxes a ray sees, and a
hidden blocker.  These parts validate the fixture, not the feature; the last test asks the library for the feature's entry points."""
import os
import subprocess

import numpy as np

from nanort_amd import capi
from oracle import bindings as ob
from scene_fixture import instances
from scene_masks_fixture import ALL, LINE_B, check_line_table, expect_masked, line_node_masks, line_ray_words, scene_nodes
from test_gpu_scene_occlusion import line_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def line_oracle(oracle):
    (av, af), (bv, bf), nodes, rays, front, mid, _ = line_fixture()
    tree = {"A": oracle.build(av, af)[:2], "B": oracle.build(bv, bf)[:2]}
    mesh = {"A": (av, af), "B": (bv, bf)}
    O = ob.SceneOracle(oracle)
    for w, x in nodes:
        O.add_node(mesh[w][0], mesh[w][1], x, tree=tree[w])
    assert O.commit()
    return O, rays, front, mid


def test_all_ones_words_are_the_plain_restatement(oracle):
    O, rays, _, _ = line_oracle(oracle)
    oh, om = O.traverse(rays)
    nodes = scene_nodes(O)
    for node_masks, words in ((None, None), (np.full(len(nodes), ALL, dtype=np.uint32), np.full(rays.shape[0], ALL, dtype=np.uint32)),
                              (line_node_masks(), None)):  # (every node keeps some bit: all-ones RAYS see them all)
        h, m = expect_masked(oracle, nodes, node_masks, rays, words)
        assert h.tobytes() == oh.tobytes() and m.tobytes() == om.tobytes()
    assert 0 < om.mean() < 1


def test_all_ones_words_on_the_five_node_fixture(oracle):
    from nanort_amd import scenes

    O = ob.SceneOracle(oracle)
    for v, f, x in instances(sphere_res=(16, 8), plane_res=(12, 6)):
        O.add_node(v, f, x)
    assert O.commit()
    rays = scenes.camera_rays(64, 36)
    oh, om = O.traverse(rays)
    h, m = expect_masked(oracle, scene_nodes(O), None, rays, None)
    assert h.tobytes() == oh.tobytes() and m.tobytes() == om.tobytes()
    # the plane hidden from bit 0: rays with that bit alone lose exactly their plane hits; a zero word sees nothing
    masks = np.full(5, ALL, dtype=np.uint32)
    masks[0] &= ~np.uint32(1)
    words = np.array([ALL, 1, 0], dtype=np.uint32)[np.arange(rays.shape[0]) % 3]
    h, m = expect_masked(oracle, scene_nodes(O), masks, rays, words)
    assert h[words == ALL].tobytes() == oh[words == ALL].tobytes()
    assert (h["node_id"][words == 1] != 0).all() and (oh["node_id"][words == 1] == 0).any()
    assert (m[words == 0] == 0).all() and (h["node_id"][words == 0] == ALL).all()
    assert (h["t"][words == 0] == rays["max_t"][words == 0]).all()


def test_line_fixture_yields_every_class(oracle):
    """Hidden instances take no place among the 64 nearest: with ten, seven or six of the leading boxes hidden the blocker ranks
    61st, 64th or 65th, and the flag follows."""
    O, rays, front, mid = line_oracle(oracle)
    masks = line_node_masks()
    assert masks[LINE_B] == ALL & ~8 and (masks[71:] == ALL).all() and (masks[10:70] == ALL).all()
    words = line_ray_words(rays.shape[0], front, mid)
    assert len(np.unique(words)) == 6
    h, m = expect_masked(oracle, scene_nodes(O), masks, rays, words)
    check_line_table(m, words, front, mid)
    # a hit of a front ray names the blocker by ITS id in the whole scene
    hit = np.nonzero(m[front] == 1)[0]
    assert (h["node_id"][front][hit] == LINE_B).all()
    # and an implementation that lists a hidden instance and skips it when reached would differ: unmasked, the blocker is out of reach
    _, om = O.traverse(rays)
    assert (om[front] == 0).all() and (om[mid] == 1).all()


def test_the_library_exports_the_masked_scene_calls():
    names = ["nrtSceneSetNodeMasks", "nrtSceneTraverseBatchMasked_f32", "nrtSceneTraverseBatchMaskedDevice_f32",
             "nrtSceneOccludedBatchMasked_f32", "nrtSceneOccludedBatchMaskedDevice_f32"]
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert set(names) <= exported
    assert set(names) <= set(capi.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "nanort_hip.h")).read()
    for n in names:
        assert "NRT_API nrt_status %s(" % n in hdr, n
    from nanort_amd import Scene

    for meth in ("SetNodeMasks", "TraverseBatchMasked", "TraverseBatchMaskedDevice", "OccludedBatchMasked", "OccludedBatchMaskedDevice"):
        assert callable(getattr(Scene, meth, None)), meth


REFERENCE = os.environ.get("REFERENCE", "/root/reference")


def test_batch_tracer_masked_methods_fit_the_unmodified_nanosg(tmp_path):
    """include/nanosg_hip.h: BatchTracer::SetNodeMasks / TraverseMasked type-check against the reference's own nanosg.h (they
    only forward to the C ABI, whose behaviour tests/test_gpu_scene_masks.py covers)."""
    import pytest

    if not os.path.exists(os.path.join(REFERENCE, "nanort.h")):
        pytest.skip("reference tree not present")
    tu = tmp_path / "sgm.cc"
    tu.write_text(
        '#include "nanort.h"\n#include "nanosg.h"\n#include "nanosg_hip.h"\n'
        "struct Mesh { std::vector<float> vertices; std::vector<unsigned int> faces; size_t stride;\n"
        "  void GetNormal(float Ng[3], float Ns[3], unsigned int, float, float) const { Ng[0]=Ns[0]=0; Ng[1]=Ns[1]=0; Ng[2]=Ns[2]=1; } };\n"
        "int main() { Mesh m; nanosg::Node<float, Mesh> node(&m); nanosg::Scene<float, Mesh> scene; scene.AddNode(node); scene.Commit();\n"
        "  nanosg::BatchTracer<nanosg::Scene<float, Mesh> > tr(scene); std::vector<nanort::Ray<float> > rays(4);\n"
        "  std::vector<nanosg::Intersection<float> > is(4); std::vector<unsigned char> hit(4);\n"
        "  std::vector<uint32_t> node_words(1, 0xFFFFFFFEu), ray_words(4, 1u);\n"
        "  bool (nanosg::BatchTracer<nanosg::Scene<float, Mesh> >::*set)(const uint32_t *, size_t) = &nanosg::BatchTracer<nanosg::Scene<float, Mesh> >::SetNodeMasks;\n"
        "  (void)set;\n"
        "  if (!tr.SetNodeMasks(node_words.data(), node_words.size()) || !tr.SetNodeMasks(NULL, 0)) return 2;\n"
        "  if (!tr.TraverseMasked(rays.data(), NULL, 4, is.data())) return 3;\n"
        "  return tr.TraverseMasked(rays.data(), ray_words.data(), 4, is.data(), hit.data()) ? 0 : 1; }\n")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", "-DNANORT_USE_HIP_BACKEND", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(REFERENCE, "examples", "nanosg"), str(tu)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]

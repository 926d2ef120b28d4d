"""The expectation of the scene queries with per-ray skip pairs (tests/scene_query_fixture.py) and the two fixtures the GPU tests
rest on, checked on the CPU against the restatement alone: with every pair invalid the expectation IS the plain restatement, byte
for byte; a bounce wave started on the five-node fixture's triangles re-hits the triangle it starts on about half of the time and
never once the pair is skipped; and on three stacked copies of one plane a ray that skips (p, node 0) must name (p, node 1).  The
last tests ask the header, the library and the bindings for the feature's ABI."""
import ctypes
import os
import subprocess

import numpy as np

from nanort_amd import capi, scenes
from oracle import bindings as ob
from scene_fixture import instances
from scene_masks_fixture import ALL, expect_masked, miss_records, scene_nodes
from scene_query_fixture import bounce_wave, expect_query, own_pair_share, pairs_of, stacked_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")


def five_node_oracle(oracle):
    O = ob.SceneOracle(oracle)
    for v, f, x in instances(sphere_res=(16, 8), plane_res=(12, 6)):
        O.add_node(v, f, x)
    assert O.commit()
    return O


def test_invalid_pairs_are_the_plain_restatement(oracle):
    O = five_node_oracle(oracle)
    nodes = scene_nodes(O)
    rays = scenes.camera_rays(64, 36)
    n = rays.shape[0]
    oh, om = O.traverse(rays)
    assert 0 < om.mean() <= 1
    faces = [f.shape[0] for _, f, _, _ in nodes]
    k = np.arange(n)
    cases = {
        "no pairs": None,
        "all ones": np.full((n, 2), ALL, dtype=np.uint32),
        "node all ones": np.stack([k % 7, np.full(n, ALL)], axis=1).astype(np.uint32),
        "node >= count": np.stack([k % 7, 5 + k % 3], axis=1).astype(np.uint32),
        "prim all ones": np.stack([np.full(n, ALL), k % 5], axis=1).astype(np.uint32),
        "prim >= faces": np.stack([np.array(faces)[k % 5] + k % 2, k % 5], axis=1).astype(np.uint32),
        "the miss records of a wave that missed": pairs_of(miss_records(rays)),
    }
    for what, pairs in cases.items():
        h, m = expect_query(oracle, nodes, rays, pairs, committed=O)
        assert h.tobytes() == oh.tobytes() and m.tobytes() == om.tobytes(), what
    # ... and with MASKED on top, the masked expectation
    masks = np.array([ALL & ~1, ALL, ALL, 1, 2], dtype=np.uint32)
    words = np.array([ALL, 1, 0, 2], dtype=np.uint32)[k % 4]
    eh, em = expect_masked(oracle, nodes, masks, rays, words)
    h, m = expect_query(oracle, nodes, rays, cases["node >= count"], masks, words)
    assert h.tobytes() == eh.tobytes() and m.tobytes() == em.tobytes()
    # a pair that names a HIDDEN node skips nothing either (the node does not exist for the ray), a visible one does
    pairs = pairs_of(oh)
    h, m = expect_query(oracle, nodes, rays, pairs, masks, words)
    hidden = (oh["node_id"] != ALL) & ((masks[np.minimum(oh["node_id"], 4)] & words) == 0)
    assert hidden.any() and h[hidden].tobytes() == eh[hidden].tobytes()


def test_condition_a_bounce_rays_re_hit_their_own_triangle_until_it_is_skipped(oracle):
    O = five_node_oracle(oracle)
    nodes = scene_nodes(O)
    rays = scenes.camera_rays(64, 36)
    oh, om = O.traverse(rays)
    assert om.mean() > 0.9
    b, pairs, records = bounce_wave(rays, oh, om, np.random.default_rng(5))
    assert b.shape[0] > 2000 and np.array_equal(pairs, pairs_of(records))
    uh, um = O.traverse(b)
    own = own_pair_share(uh, um, pairs)
    print("bounce rays: %d, unskipped own-pair share %.3f" % (b.shape[0], own))
    assert own >= 0.40, own  # half of the directions point back through the surface the ray starts on
    sh, sm = expect_query(oracle, nodes, b, pairs, committed=O)
    own_s = own_pair_share(sh, sm, pairs)
    changed = float((sm != um).mean())
    print("skipped own-pair share %.3f, flags changed %.3f" % (own_s, changed))
    assert own_s == 0.0
    assert changed > 0.0  # (a ray that left the plane downwards through its own triangle now misses)
    # rays that did not name their own pair are untouched by the skip
    other = ~((um == 1) & (uh["prim_id"] == pairs[:, 0]) & (uh["node_id"] == pairs[:, 1]))
    assert sh[other].tobytes() == uh[other].tobytes()


def test_condition_b_stacked_planes_name_the_next_copy(oracle):
    (pv, pf), xs, rays, pairs = stacked_planes(np.random.default_rng(11))
    tree = oracle.build(pv, pf)[:2]
    O = ob.SceneOracle(oracle)
    for x in xs:
        O.add_node(pv, pf, x, tree=tree)
    assert O.commit()
    uh, um = O.traverse(rays)
    own = own_pair_share(uh, um, pairs)
    print("stacked planes: unskipped own-pair share %.3f" % own)
    assert own > 0.0
    sh, sm = expect_query(oracle, scene_nodes(O), rays, pairs, committed=O)
    assert sm.all()
    assert (sh["node_id"] == 1).all() and np.array_equal(sh["prim_id"], pairs[:, 0])
    # what comparing the primitive id alone would return: face p gone from EVERY copy
    faces_of_all = []
    for j in range(3):
        faces_of_all.append(O.arr[j].faces)
    wrong = 0
    for i in range(0, rays.shape[0], 60):
        f = pf.copy()
        f[pairs[i, 0], :] = f[pairs[i, 0], 0]
        for j in range(3):
            O.arr[j].faces = f.ctypes.data
        h, m = O.traverse(rays[i:i + 1])
        for j in range(3):
            O.arr[j].faces = faces_of_all[j]
        wrong += int(not (m[0] == 1 and h["node_id"][0] == 1 and h["prim_id"][0] == pairs[i, 0]))
    assert wrong == 10  # every sampled ray: a miss, or another node or face


C_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "nanort_hip.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(nrt_scene_query_f32, f), sizeof(((nrt_scene_query_f32 *)0)->f))
int main(void) {
  printf("sizeof %zu 0\n", sizeof(nrt_scene_query_f32));
  F(struct_size); F(flags); F(rays); F(num_rays); F(ray_masks); F(skip_pairs); F(skip_stride_bytes); F(reserved); F(hits_out); F(mask_out);
  printf("FLAGBITS %u %u\n", NRT_SCENE_QUERY_OCCLUSION | (NRT_SCENE_QUERY_MASKED << 8) | (NRT_SCENE_QUERY_SKIP << 16), 0u);
  printf("pair %zu %zu\n", offsetof(nrt_scene_hit_f32, prim_id), offsetof(nrt_scene_hit_f32, node_id));
  printf("record %zu 0\n", sizeof(nrt_scene_hit_f32));
  return 0;
}
"""


def test_descriptor_layout_in_c_and_in_python(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout
    got = {l.split()[0]: (int(l.split()[1]), int(l.split()[2])) for l in out.splitlines()}
    assert got.pop("sizeof") == (ctypes.sizeof(capi.SceneQuery), 0) == (64, 0)
    assert got.pop("FLAGBITS")[0] == capi.NRT_SCENE_QUERY_OCCLUSION | (capi.NRT_SCENE_QUERY_MASKED << 8) | (capi.NRT_SCENE_QUERY_SKIP << 16)
    from nanort_amd.wire import SCENE_HIT_F32

    # the pair is the tail of a record, prim_id first: a bounce wave passes &hits[0].prim_id at stride sizeof(record)
    assert got.pop("pair") == (SCENE_HIT_F32.fields["prim_id"][1], SCENE_HIT_F32.fields["node_id"][1]) == (12, 16)
    assert got.pop("record") == (SCENE_HIT_F32.itemsize, 0) == (20, 0)
    fields = [name for name, _ in capi.SceneQuery._fields_]
    assert sorted(got) == sorted(fields)
    for name in fields:
        d = getattr(capi.SceneQuery, name)
        assert got[name] == (d.offset, d.size), name


def test_the_library_exports_the_scene_query_calls():
    names = ["nrtSceneQueryBatch_f32", "nrtSceneQueryBatchDevice_f32"]
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert set(names) <= exported
    assert set(names) <= set(capi.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "nanort_hip.h")).read()
    for n in names:
        assert "NRT_API nrt_status %s(" % n in hdr, n
    assert "&hits[0].prim_id" in hdr and "sizeof(nrt_scene_hit_f32)" in hdr  # the reason for the pair's layout is stated
    from nanort_amd import Scene

    for meth in ("QueryBatch", "QueryBatchDevice"):
        assert callable(getattr(Scene, meth, None)), meth


def test_batch_tracer_query_method_fits_the_unmodified_nanosg(tmp_path):
    """include/nanosg_hip.h: BatchTracer::TraverseQuery type-checks against the reference's own nanosg.h (it only forwards to the
    C ABI, whose behaviour tests/test_gpu_scene_query.py covers)."""
    import pytest

    if not os.path.exists(os.path.join(REFERENCE, "nanort.h")):
        pytest.skip("reference tree not present")
    tu = tmp_path / "sgq.cc"
    tu.write_text(
        '#include "nanort.h"\n#include "nanosg.h"\n#include "nanosg_hip.h"\n'
        "struct Mesh { std::vector<float> vertices; std::vector<unsigned int> faces; size_t stride;\n"
        "  void GetNormal(float Ng[3], float Ns[3], unsigned int, float, float) const { Ng[0]=Ns[0]=0; Ng[1]=Ns[1]=0; Ng[2]=Ns[2]=1; } };\n"
        "int main() { Mesh m; nanosg::Node<float, Mesh> node(&m); nanosg::Scene<float, Mesh> scene; scene.AddNode(node); scene.Commit();\n"
        "  nanosg::BatchTracer<nanosg::Scene<float, Mesh> > tr(scene); std::vector<nanort::Ray<float> > rays(4);\n"
        "  std::vector<nanosg::Intersection<float> > is(4); std::vector<unsigned char> hit(4);\n"
        "  std::vector<uint32_t> ray_words(4, 1u), pairs(8, 0xFFFFFFFFu); std::vector<nrt_scene_hit_f32> prev(4);\n"
        "  if (!tr.TraverseQuery(rays.data(), 4, NULL, NULL, 0, false, is.data())) return 2;\n"
        "  if (!tr.TraverseQuery(rays.data(), 4, ray_words.data(), pairs.data(), 8, false, is.data(), hit.data())) return 3;\n"
        "  if (!tr.TraverseQuery(rays.data(), 4, NULL, &prev[0].prim_id, sizeof(nrt_scene_hit_f32), false, is.data(), hit.data())) return 4;\n"
        "  return tr.TraverseQuery(rays.data(), 4, NULL, &prev[0].prim_id, sizeof(prev[0]), true, static_cast<nanosg::Intersection<float> *>(NULL), hit.data()) ? 0 : 1; }\n")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", "-DNANORT_USE_HIP_BACKEND", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(REFERENCE, "examples", "nanosg"), str(tu)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]

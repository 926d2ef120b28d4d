// tests/ref_curves_shim.cc — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// C-ABI wrapper around the UNMODIFIED custom-primitive example examples/curves_primitive/main.cc (genFur, CurvePred,
// CurveGeometry, CurveIntersector) on top of the unmodified nanort.h; the example's translation unit is included where it
// lies with its main() renamed.  tests/curves_fixture.py compiles it into a temporary directory where the reference tree
// exists (-I$REFERENCE -I$REFERENCE/examples/common -I$REFERENCE/examples/curves_primitive, -ffp-contract=off); its answers
// are recorded under tests/golden/ for the machines where it does not.
#include <stdint.h>
#include <string.h>

#include <chrono>

#define main nrt_curves_example_main
#include "main.cc"
#undef main

extern "C" {

struct RefCurveAccel {
  std::vector<float> cps, radii;
  nanort::BVHAccel<float> accel;
};

// the example's own scene (main.cc:850-868): 400 curves on a sphere of radius 4 at the origin; `thickness` is its argv[1]
uint32_t refcv_fur(float *cps_out, float *radii_out, uint32_t capacity, float thickness) {
  std::vector<float> vertices, thicknesses;
  genFur(&vertices, &thicknesses, float3(0.0f, 0.0f, 0.0f), 4.0f, thickness);
  const uint32_t n = (uint32_t)(thicknesses.size() / 4);
  if (n > capacity) return n;
  memcpy(cps_out, vertices.data(), vertices.size() * sizeof(float));
  memcpy(radii_out, thicknesses.data(), thicknesses.size() * sizeof(float));
  return n;
}

void *refcv_build(const float *cps, const float *radii, uint32_t n, uint32_t min_leaf, uint32_t *num_nodes) {
  RefCurveAccel *a = new RefCurveAccel();
  a->cps.assign(cps, cps + 12 * (size_t)n);
  a->radii.assign(radii, radii + 4 * (size_t)n);
  nanort::BVHBuildOptions<float> options;  // the example's options (main.cc:858-859)
  options.cache_bbox = false;
  if (min_leaf) options.min_leaf_primitives = min_leaf;
  CurveGeometry geom(a->cps.data(), a->radii.data());
  CurvePred pred(a->cps.data());
  if (!a->accel.Build(n, geom, pred, options)) {
    delete a;
    return NULL;
  }
  *num_nodes = (uint32_t)a->accel.GetNodes().size();
  return a;
}

void refcv_get_tree(void *h, void *nodes_out, uint32_t *indices_out) {
  RefCurveAccel *a = static_cast<RefCurveAccel *>(h);
  memcpy(nodes_out, a->accel.GetNodes().data(), a->accel.GetNodes().size() * sizeof(nanort::BVHNode<float>));
  memcpy(indices_out, a->accel.GetIndices().data(), a->accel.GetIndices().size() * sizeof(unsigned int));
}

void refcv_destroy(void *h) { delete static_cast<RefCurveAccel *>(h); }

// hits: CurveIntersection[n] (40 B: t, prim_id, u, v, tangent[3], normal[3]).  A miss leaves
// {max_t, 0xFFFFFFFF, 0, 0, (0,0,0), (0,0,0)}.  The intersector's current distance is set through its public interface
// before each Traverse (which does the same itself, nanort.h:2501).  Returns the seconds the loop took.
double refcv_traverse(void *h, const void *rays, uint64_t n, uint32_t range0, uint32_t range1, int num_subdivisions, void *hits,
                      uint8_t *mask) {
  RefCurveAccel *a = static_cast<RefCurveAccel *>(h);
  const nanort::Ray<float> *r = static_cast<const nanort::Ray<float> *>(rays);
  static_assert(sizeof(CurveIntersection) == 40, "CurveIntersection");
  CurveIntersection *o = static_cast<CurveIntersection *>(hits);
  nanort::BVHTraceOptions opt;
  opt.prim_ids_range[0] = range0;
  opt.prim_ids_range[1] = range1;
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  for (uint64_t i = 0; i < n; i++) {
    CurveIntersector<CurveIntersection> isector(a->cps.data(), a->radii.data(), num_subdivisions);
    CurveIntersection isect;
    memset(&isect, 0, sizeof(isect));
    isect.t = r[i].max_t;
    isect.prim_id = 0xFFFFFFFFu;
    isector.Update(r[i].max_t, 0xFFFFFFFFu);
    const bool hit = a->accel.Traverse(r[i], isector, &isect, opt);
    memcpy(&o[i], &isect, sizeof(isect));
    if (mask) mask[i] = hit ? 1 : 0;
  }
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // extern "C"

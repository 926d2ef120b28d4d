// tests/cpp/occluded_kinds_check.cc — occlusion queries of the sphere, cylinder and curve primitives of include/nanort.h, on the
// host and, compiled with -DNANORT_USE_HIP_BACKEND, on the GPU.
//
//   occluded_kinds_check <spheres|cylinders|curves> <prims.bin> <rays.bin> <flags.bin>
//       prims.bin: u32 n, then n * {3, 6, 12} floats (centres / two end points / four control points) and n * {1, 2, 4} radii;
//       rays.bin: u64 m, m rays.  Build() over the primitives, then for every variant of the kind's intersector (cylinders:
//       test_cap on and off; curves: 4, 7 and 1 subdivisions) and two prim_ids_range settings (everything; the upper half of the
//       ids) the generic host OccludedBatch(rays, m, intersector, out) must give, ray by ray, the flag of Traverse().
//       flags.bin: the m flags of the first variant with the default options.
//   With the backend macro Build() runs on the GPU and the program first checks OccludedBatchSpheres / OccludedBatchCylinders /
//   OccludedBatchCurves and their Device forms against that host call — test_cap and num_subdivisions changing between calls,
//   on an accel that shares its device context with a copy, and on the copy afterwards — and the refusals of the wrong kind.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nanort.h"
#ifdef NANORT_USE_HIP_BACKEND
#include <hip/hip_runtime_api.h>  // device buffers for the *Device forms
#endif

typedef nanort::Ray<float> Ray;
typedef nanort::BVHAccel<float> Accel;

static bool read_all(const char *path, std::vector<char> *buf) {
  FILE *fp = fopen(path, "rb");
  if (!fp) return false;
  fseek(fp, 0, SEEK_END);
  const long n = ftell(fp);
  fseek(fp, 0, SEEK_SET);
  buf->resize(static_cast<size_t>(n));
  const bool ok = n == 0 || fread(&(*buf)[0], 1, static_cast<size_t>(n), fp) == static_cast<size_t>(n);
  fclose(fp);
  return ok;
}

static int g_failures = 0;
static void expect(bool ok, const std::string &what) {
  if (!ok) {
    fprintf(stderr, "FAILED: %s\n", what.c_str());
    g_failures++;
  }
}

// The generic OccludedBatch against the per-ray Traverse() loop; returns the flags.
template <class I, class H>
static std::vector<unsigned char> host_flags(const Accel &accel, const std::vector<Ray> &rays, const I &isector, const nanort::BVHTraceOptions &opt,
                                             const std::string &what) {
  const size_t m = rays.size();
  std::vector<unsigned char> batch(m, 7), loop(m, 0);
  expect((accel.template OccludedBatch<I, H>(m ? &rays[0] : NULL, m, isector, m ? &batch[0] : NULL, opt)), what + ": OccludedBatch returned false");
  for (size_t i = 0; i < m; i++) {
    const I ray_isector(isector);
    H isect;
    loop[i] = accel.Traverse(rays[i], ray_isector, &isect, opt) ? 1 : 0;
  }
  expect(batch == loop, what + ": the generic OccludedBatch differs from the per-ray Traverse() flags");
  return loop;
}

#ifdef NANORT_USE_HIP_BACKEND
struct DeviceRays {
  void *rays, *flags;
  size_t m;
  explicit DeviceRays(const std::vector<Ray> &r) : rays(NULL), flags(NULL), m(r.size()) {
    if (hipMalloc(&rays, m ? m * sizeof(Ray) : 1) != hipSuccess || hipMalloc(&flags, m ? m : 1) != hipSuccess ||
        (m && hipMemcpy(rays, &r[0], m * sizeof(Ray), hipMemcpyHostToDevice) != hipSuccess)) {
      fprintf(stderr, "device buffers for %zu rays failed\n", m);
      exit(3);
    }
  }
  ~DeviceRays() {
    (void)hipFree(rays);
    (void)hipFree(flags);
  }
  // (the call under test in between: asynchronous on `s`)
  void poison() const {
    if (hipMemset(flags, 0xCD, m ? m : 1) != hipSuccess || hipDeviceSynchronize() != hipSuccess) exit(3);
  }
  std::vector<unsigned char> fetch(hipStream_t s) const {
    std::vector<unsigned char> out(m, 9);
    if (hipStreamSynchronize(s) != hipSuccess || (m && hipMemcpy(&out[0], flags, m, hipMemcpyDeviceToHost) != hipSuccess)) exit(3);
    return out;
  }
};
#endif

static nanort::BVHTraceOptions upper_half(unsigned int n) {
  nanort::BVHTraceOptions o;
  o.prim_ids_range[0] = n / 2;
  o.prim_ids_range[1] = n;
  return o;
}

int main(int argc, char **argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: occluded_kinds_check <spheres|cylinders|curves> <prims.bin> <rays.bin> <flags.bin>\n");
    return 2;
  }
  const std::string kind = argv[1];
  const size_t per_prim = kind == "spheres" ? 3 : (kind == "cylinders" ? 6 : (kind == "curves" ? 12 : 0));
  std::vector<char> pb, rb;
  if (!per_prim || !read_all(argv[2], &pb) || !read_all(argv[3], &rb) || pb.size() < 4 || rb.size() < 8) {
    fprintf(stderr, "cannot read the inputs\n");
    return 2;
  }
  unsigned int n = 0;
  unsigned long long m64 = 0;
  std::memcpy(&n, &pb[0], 4);
  std::memcpy(&m64, &rb[0], 8);
  const size_t m = static_cast<size_t>(m64), radii_per_prim = per_prim / 3;
  if (pb.size() != 4 + static_cast<size_t>(n) * (per_prim + radii_per_prim) * 4 || rb.size() != 8 + m * sizeof(Ray)) {
    fprintf(stderr, "input sizes do not match their counts\n");
    return 2;
  }
  std::vector<float> pos(per_prim * n), radii(radii_per_prim * n);
  std::memcpy(pos.data(), &pb[4], pos.size() * 4);
  std::memcpy(radii.data(), &pb[4 + pos.size() * 4], radii.size() * 4);
  std::vector<Ray> rays(m);
  if (m) std::memcpy(static_cast<void *>(&rays[0]), &rb[8], m * sizeof(Ray));
  const Ray *rp = m ? &rays[0] : NULL;

  Accel accel;
  nanort::BVHBuildOptions<float> build_options;
  build_options.cache_bbox = false;
  bool built = false;
  if (kind == "spheres") built = accel.Build(n, nanort::SphereGeometry(pos.data(), radii.data()), nanort::SpherePred(pos.data()), build_options);
  if (kind == "cylinders") built = accel.Build(n, nanort::CylinderGeometry(pos.data(), radii.data()), nanort::CylinderPred(pos.data()), build_options);
  if (kind == "curves") built = accel.Build(n, nanort::BezierCurveGeometry(pos.data(), radii.data()), nanort::BezierCurvePred(pos.data()), build_options);
  if (!built) {
    fprintf(stderr, "Build() failed\n");
    return 1;
  }
  const nanort::BVHTraceOptions all, half = upper_half(n);
  std::vector<unsigned char> first;

#ifdef NANORT_USE_HIP_BACKEND
  if (accel.NumHipDevices() == 0) {
    fprintf(stderr, "Build() did not go to the GPU: %s\n", accel.LastBackendError().c_str());
    return 1;
  }
  hipStream_t side;
  if (hipStreamCreate(&side) != hipSuccess) return 3;
  const DeviceRays dev(rays);
  std::vector<unsigned char> got(m, 7);
  unsigned char *gp = m ? &got[0] : NULL;
  unsigned char *dp = static_cast<unsigned char *>(dev.flags);
  const Ray *drp = static_cast<const Ray *>(dev.rays);
  // the calls of the other kinds refuse, with a text, and write nothing
  {
    const std::vector<unsigned char> before(got);
    if (kind != "spheres") expect(!accel.OccludedBatchSpheres(rp, m, gp) && !accel.LastBackendError().empty(), "OccludedBatchSpheres did not refuse");
    if (kind != "cylinders") expect(!accel.OccludedBatchCylinders(rp, m, gp) && !accel.LastBackendError().empty(), "OccludedBatchCylinders did not refuse");
    if (kind != "curves") expect(!accel.OccludedBatchCurves(rp, m, gp) && !accel.LastBackendError().empty(), "OccludedBatchCurves did not refuse");
    expect(!accel.OccludedBatch(rp, m, gp) && !accel.LastBackendError().empty(), "the triangle accels' OccludedBatch did not refuse");
    expect(got == before, "a refused call wrote flags");
  }
  Accel copy(accel);  // shares the device context until one of the two needs another test_cap / num_subdivisions
#endif

  if (kind == "spheres") {
    typedef nanort::SphereIntersector<> I;
    const I isector(pos.data(), radii.data());
    for (int r = 0; r < 2; r++) {
      const nanort::BVHTraceOptions &o = r ? half : all;
      const std::vector<unsigned char> want = host_flags<I, nanort::SphereIntersection>(accel, rays, isector, o, r ? "spheres, upper half" : "spheres");
      if (r == 0) first = want;
#ifdef NANORT_USE_HIP_BACKEND
      got.assign(m, 7);
      expect(accel.OccludedBatchSpheres(rp, m, gp, o) && got == want, "OccludedBatchSpheres differs from the host: " + accel.LastBackendError());
      dev.poison();
      expect(accel.OccludedBatchSpheresDevice(drp, m, dp, side, o) && dev.fetch(side) == want, "OccludedBatchSpheresDevice differs from the host");
      got.assign(m, 7);
      expect(copy.OccludedBatchSpheres(rp, m, gp, o) && got == want, "OccludedBatchSpheres on the copy differs from the host");
#endif
    }
  } else if (kind == "cylinders") {
    typedef nanort::CylinderIntersector<> I;
    const bool caps[4] = {true, false, false, true};  // (the flag changes between calls, both ways)
    for (int pass = 0; pass < 4; pass++) {
      const bool cap = caps[pass];
      const I isector(pos.data(), radii.data(), cap);
      const nanort::BVHTraceOptions &o = (pass & 1) ? half : all;
      const std::vector<unsigned char> want = host_flags<I, nanort::CylinderIntersection>(accel, rays, isector, o, cap ? "cylinders, caps" : "cylinders, no caps");
      if (pass == 0) first = want;
#ifdef NANORT_USE_HIP_BACKEND
      // (pass 1: the accel leaves the context it shares with `copy` — copy-on-write — and the copy keeps test_cap = true)
      got.assign(m, 7);
      expect(accel.OccludedBatchCylinders(rp, m, gp, o, cap) && got == want, "OccludedBatchCylinders differs from the host: " + accel.LastBackendError());
      dev.poison();
      expect(accel.OccludedBatchCylindersDevice(drp, m, dp, side, o, cap) && dev.fetch(side) == want, "OccludedBatchCylindersDevice differs from the host");
      const I cap_on(pos.data(), radii.data(), true);
      got.assign(m, 7);
      expect(copy.OccludedBatchCylinders(rp, m, gp, o, true) && got == host_flags<I, nanort::CylinderIntersection>(copy, rays, cap_on, o, "cylinders, the copy"),
             "OccludedBatchCylinders on the copy differs from the host");
#endif
    }
  } else {
    typedef nanort::BezierCurveIntersector<> I;
    const int subdivs[4] = {4, 7, 1, 4};
    for (int pass = 0; pass < 4; pass++) {
      const int sd = subdivs[pass];
      const I isector(pos.data(), radii.data(), sd);
      const nanort::BVHTraceOptions &o = (pass & 1) ? half : all;
      const std::vector<unsigned char> want = host_flags<I, nanort::BezierCurveIntersection>(accel, rays, isector, o, "curves, " + std::to_string(sd) + " subdivisions");
      if (pass == 0) first = want;
#ifdef NANORT_USE_HIP_BACKEND
      got.assign(m, 7);
      expect(accel.OccludedBatchCurves(rp, m, gp, o, sd) && got == want, "OccludedBatchCurves differs from the host: " + accel.LastBackendError());
      dev.poison();
      expect(accel.OccludedBatchCurvesDevice(drp, m, dp, side, o, sd) && dev.fetch(side) == want, "OccludedBatchCurvesDevice differs from the host");
      const I four(pos.data(), radii.data(), 4);
      got.assign(m, 7);
      expect(copy.OccludedBatchCurves(rp, m, gp, o, 4) && got == host_flags<I, nanort::BezierCurveIntersection>(copy, rays, four, o, "curves, the copy"),
             "OccludedBatchCurves on the copy differs from the host");
#endif
    }
#ifdef NANORT_USE_HIP_BACKEND
    expect(!accel.OccludedBatchCurves(rp, m, gp, all, 0) && !accel.OccludedBatchCurves(rp, m, gp, all, 65) &&
               accel.LastBackendError().find("1..64") != std::string::npos,
           "OccludedBatchCurves took a subdivision count outside 1..64");
#endif
  }
#ifdef NANORT_USE_HIP_BACKEND
  (void)hipStreamDestroy(side);
#endif

  FILE *fp = fopen(argv[4], "wb");
  if (!fp) return 2;
  if (m) fwrite(&first[0], 1, m, fp);
  fclose(fp);
  if (g_failures) return 1;
  printf("occluded_kinds_check ok: %s, %u primitives, %zu rays\n", kind.c_str(), n, m);
  return 0;
}

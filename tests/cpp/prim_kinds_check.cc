// tests/cpp/prim_kinds_check.cc — prints what nanort_amd/csrc/prim_kinds.h says, for tests/test_prim_kinds.py to compare with
// literals and a numpy restatement.  Commands on stdin, one per line:
//   table                                              -> per kind: name pos_bytes radius_bytes num_verts fp64 max_count post_pass hit_bytes (fp32)
//   count x0 y0 z0 x1 y1 z1 r0 r1 seg_radii kmax       -> the cylinder's segment count
//   offsets n seg_radii split limit, then n x (x0 y0 z0 x1 y1 z1 r0 r1) -> total, then off[0 .. n]
#include <stdio.h>
#include <string.h>

#include <vector>

#include "prim_kinds.h"

int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "table")) {
      for (int k = 0; k < nrt::kNumPrimKinds; k++) {
        const nrt::PrimKind &p = nrt::kPrimKinds[k];
        printf("%s %zu %zu %d %d %u %d %d\n", p.name, p.pos_floats * sizeof(float), p.radius_floats * sizeof(float), p.num_verts, (int)p.fp64,
               p.max_count, (int)p.post_pass, p.hit_bytes);
      }
    } else if (!strcmp(cmd, "count")) {
      float v[8];
      int seg_radii;
      unsigned kmax;
      for (float &x : v)
        if (scanf("%f", &x) != 1) return 2;
      if (scanf("%d %u", &seg_radii, &kmax) != 2) return 2;
      printf("%u\n", nrt::cylinder_segment_count(v, v + 3, v[6], v[7], seg_radii, kmax));
    } else if (!strcmp(cmd, "offsets")) {
      unsigned n, split;
      int seg_radii;
      unsigned long long limit;
      if (scanf("%u %d %u %llu", &n, &seg_radii, &split, &limit) != 4) return 2;
      std::vector<float> ends(6 * (size_t)n), radii(2 * (size_t)n);
      for (unsigned i = 0; i < n; i++) {
        for (int k = 0; k < 6; k++)
          if (scanf("%f", &ends[6 * (size_t)i + k]) != 1) return 2;
        if (scanf("%f %f", &radii[2 * (size_t)i], &radii[2 * (size_t)i + 1]) != 2) return 2;
      }
      std::vector<uint32_t> off((size_t)n + 1);
      const uint64_t total = nrt::cylinder_segment_offsets(ends.data(), radii.data(), n, seg_radii, split, limit, off.data());
      printf("%llu", (unsigned long long)total);
      for (uint32_t o : off) printf(" %u", o);
      printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}

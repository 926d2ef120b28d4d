// tests/test_launch_plan.py: prints what nanort_amd/csrc/launch_plan.h plans, one line per request read from stdin.
//   grid  rays block cus blocks_per_cu parts                          -> grid parts blocks_per_part
//   plan  rays waves parts static_pct static_bands slice_groups chunk -> the nine fields of DistributionPlan
//   spill depth two_level lds_entries                                 -> levels
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "launch_plan.h"

int main() {
  char kind[16];
  unsigned long long v[7];
  while (scanf("%15s", kind) == 1) {
    const int want = !strcmp(kind, "grid") ? 5 : (!strcmp(kind, "plan") ? 7 : (!strcmp(kind, "spill") ? 3 : -1));
    if (want < 0) return 2;
    for (int k = 0; k < want; k++)
      if (scanf("%llu", &v[k]) != 1) return 2;
    if (want == 5) {
      const nrt::GridPlan g = nrt::plan_grid(v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4]);
      printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", g.grid, g.parts, g.blocks_per_part);
    } else if (want == 7) {
      const nrt::DistributionPlan p = nrt::plan_distribution((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4],
                                                             (uint32_t)v[5], (uint32_t)v[6]);
      printf("%" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", p.static_per_wave,
             p.static_bands, p.band_static, p.dyn_per_band, p.band_len, p.dyn_banded, p.tail_begin, p.dyn_total, p.dyn_per_part);
    } else {
      printf("%" PRIu32 "\n", nrt::plan_spill_levels((uint32_t)v[0], v[1] != 0, (uint32_t)v[2]));
    }
  }
  return 0;
}

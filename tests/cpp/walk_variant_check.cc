// tests/test_walk_variant.py: prints what nanort_amd/csrc/walk_variant.h picks, one line per request read from stdin.
//   pick f32 kind lds_entries wide4 wide4_big leaf_items order4 plain_options stats clock prof_build
//   occ  f32 kind lds_entries wide4
//     -> f32 stack stats kind plain clock width order listed   (listed: the variant exists in that build; occ: in the product library)
#include <stdio.h>
#include <string.h>

#include "walk_variant.h"

int main() {
  char what[16];
  int v[11];
  while (scanf("%15s", what) == 1) {
    const int want = !strcmp(what, "pick") ? 11 : (!strcmp(what, "occ") ? 4 : -1);
    if (want < 0) return 2;
    for (int k = 0; k < want; k++)
      if (scanf("%d", &v[k]) != 1) return 2;
    nrt::WalkVariant w;
    bool prof = false;
    if (want == 11) {
      const nrt::WalkRequest r = {v[0] != 0, v[1], v[2], v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0, v[7] != 0, v[8] != 0, v[9] != 0};
      prof = v[10] != 0;
      w = nrt::pick_wide_variant(r, prof);
    } else {
      w = nrt::occupancy_variant(v[0] != 0, v[1], v[2], v[3] != 0);
    }
    printf("%d %d %d %d %d %d %d %d %d\n", (int)w.f32, w.stack, (int)w.stats, w.kind, (int)w.plain, (int)w.clock, w.width, w.order,
           (int)nrt::walk_variant_exists(w, prof));
  }
  return 0;
}

// nanort_amd/csrc/launch_plan.h — the integer arithmetic of a traversal launch (api_query.hip, traverse_device): how large the
// persistent grid is, how a batch is dealt out to its waves, how deep the overflow stack has to be.  Plain C++ without a HIP
// include, so that tests/cpp/launch_plan_check.cc can check it on a machine without a GPU: hit records are identical under
// every plan, so no parity test notices a slip here.  (Which kernel the launch runs: walk_variant.h, in the same style.)
#pragma once
#include <stdint.h>

namespace nrt {

// Persistent grid: every block resident (`blocks_per_cu`: occupancy of the chosen variant), never more blocks than the batch
// has rays for, whole blocks per partition (ranks are partition-major).
struct GridPlan {
  uint32_t grid, parts, blocks_per_part;
};
inline GridPlan plan_grid(uint64_t rays, uint32_t block_threads, uint32_t num_cus, uint32_t blocks_per_cu, uint32_t num_parts) {
  const uint64_t need_blocks = (rays + block_threads - 1) / block_threads;
  const uint64_t resident = (uint64_t)num_cus * blocks_per_cu;
  uint32_t grid = (uint32_t)(need_blocks < resident ? need_blocks : resident);
  const uint32_t most = num_parts < grid ? num_parts : grid;
  GridPlan g;
  g.parts = most > 1u ? most : 1u;
  g.grid = ((grid + g.parts - 1) / g.parts) * g.parts;
  g.blocks_per_part = g.grid / g.parts;
  return g;
}

// Work distribution (traverse.hip, Claim; the fields are TraverseArgs' of the same names).  Static share: `static_pct` percent
// of the batch, in whole 64-ray groups per wave, cut into up to `static_bands` slices — one at the head of each of as many
// equal bands of the batch; the rest of each band (a whole number of chunks) and the tail behind the last band are claimed
// dynamically.
struct DistributionPlan {
  uint32_t static_per_wave; // rays of one static slice of a wave (0: the whole batch is claimed in chunks)
  uint32_t static_bands;    // bands, each headed by one slice per wave (0 without a static share)
  uint32_t band_len, band_static, dyn_per_band;
  uint32_t dyn_banded;      // dynamic rays inside the bands
  uint32_t tail_begin;      // first ray behind the last band
  uint32_t dyn_total;       // dyn_banded + the tail
  uint32_t dyn_per_part;    // home range of a partition's cursor (whole chunks)
};
inline DistributionPlan plan_distribution(uint32_t rays, uint32_t total_waves, uint32_t parts, uint32_t static_pct, uint32_t static_bands,
                                          uint32_t static_slice_groups, uint32_t chunk) {
  // (less than one group per wave: none — a batch of fewer than ~400 rays per wave is claimed in chunks from its first ray; a forced
  // group per wave measured -2.7 % on a 1600x960 wave, profiles/r06y_distribution10.txt)
  const uint32_t static_share = (uint32_t)(((uint64_t)rays * static_pct / 100) / total_waves / 64); // 64-ray groups per wave
  // (a slice shorter than two 64-ray groups makes the waves of an XCD drift apart over the bands within one refill, and its
  // L2 then holds several strips of the scene at once: measured on C3, 64-ray slices in 4 bands cost 3 %; two bands of 128
  // cost nothing and still take 8 % off C2, whose sky rows otherwise leave one XCD with the whole sphere: profiles/r03d_*)
  const uint32_t most = static_share / static_slice_groups;
  const uint32_t fewer = static_bands < most ? static_bands : most;
  const uint32_t bands = fewer > 1u ? fewer : 1u;
  DistributionPlan p;
  p.static_per_wave = (static_share / bands) * 64u;
  p.band_static = p.static_per_wave * total_waves;
  p.dyn_per_band = p.static_per_wave ? (uint32_t)(((uint64_t)rays / bands - p.band_static) / chunk) * chunk : 0u;
  p.band_len = p.band_static + p.dyn_per_band;
  p.static_bands = p.static_per_wave ? bands : 0u;
  p.dyn_banded = p.static_bands * p.dyn_per_band;
  p.tail_begin = p.static_bands * p.band_len;
  p.dyn_total = p.dyn_banded + (rays - p.tail_begin);
  p.dyn_per_part = (p.dyn_total / parts / chunk) * chunk;
  return p;
}

// Levels of the per-lane overflow stack behind the `lds_entries` kept in LDS.  Deepest possible stack: one pending sibling
// per level of the path — three per TWO levels when a step covers two.
inline uint32_t plan_spill_levels(uint32_t tree_depth, bool two_level, uint32_t lds_entries) {
  const uint32_t max_entries = two_level ? 3u * (tree_depth / 2u + 1u) + 2u : tree_depth + 2u;
  return max_entries > lds_entries ? max_entries - lds_entries : 0u;
}

} // namespace nrt

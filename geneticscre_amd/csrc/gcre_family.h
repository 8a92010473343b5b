// gcre_family.h -- the host plan of the family-wise set tests (gcre_score_sets_family), defined once: the
// slab of permutation tiles, the walk order with its tie groups and threshold bins (f32_threshold: gcre_threshold.h), and the
// finish of the device's counts.  Plain C++17 over include/gcre_hip.h, no HIP: the host stage (gcre_host_family.hip) includes
// it under hipcc and tests/native/family_main.cpp under plain g++.
#pragma once
#include "../../include/gcre_hip.h"
#include "gcre_env.h"
#include "gcre_threshold.h"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

namespace gcre_family __attribute__((visibility("hidden"))) {

using gcre_host::f32_threshold;

// GCRE_FAMILY_MAX_MB: the bound on the null matrix a slab holds on the device, read per call (tests set fractions); default
// 1024.  GCRE_FAMILY_SLAB_PERMS (tests) bounds the permutations of a slab further; 0 = no bound.
inline double family_max_mb() { return gcre_env::env_mb("GCRE_FAMILY_MAX_MB", 1024, 1048576.0); }
inline int64_t family_slab_perms() { return gcre_env::env_count("GCRE_FAMILY_SLAB_PERMS"); }

// The slab: whole tiles of `tile` permutations whose null matrix, one row per valid set, stays under `max_mb`, and under
// `slab_perms` permutations (0: no such bound; one tile at the least).  One row of one tile above the limit is refused.
// Without a valid set or a permutation there is no slab (0).
inline int family_slab(int64_t V, int K, int tile, double max_mb, int64_t slab_perms, const std::string& who, int64_t& slab_tiles,
                       std::string& msg) {
  slab_tiles = 0;
  if (V == 0 || K == 0) return GCRE_OK;
  const double tile_bytes = (double)V * tile * 4.0;
  if (tile_bytes > max_mb * 1048576.0) {
    msg = who + ": the null scores of " + std::to_string(V) + " sets under one tile of " + std::to_string(tile) +
          " permutations exceed GCRE_FAMILY_MAX_MB";
    return GCRE_ERR_ARG;
  }
  const int64_t tiles = ((int64_t)K + tile - 1) / tile;
  slab_tiles = std::min<int64_t>(tiles, (int64_t)(max_mb * 1048576.0 / tile_bytes));
  if (slab_perms > 0) slab_tiles = std::min<int64_t>(slab_tiles, std::max<int64_t>(slab_perms / tile, 1));
  return GCRE_OK;
}

// The walk: the rows of the null matrix are the valid sets in ascending observed order (NaN first, then as doubles, +-0 tie;
// stable).  Per row of the walk: the threshold pattern, whether it ends its tie group (bit 31 of meta), the start of that
// group and its bin among the ascending distinct patterns (-1: a NaN score, which reaches nothing and nothing reaches it).
struct FamilyWalk {
  std::vector<int64_t> order;    // [V] row of the walk -> valid set
  std::vector<uint32_t> rank;    // [V] valid set -> row of the walk
  std::vector<uint32_t> meta;    // [V rounded up to whole 64 rows], zeros behind row V - 1
  std::vector<int64_t> gstart;   // [V]
  std::vector<int64_t> bin;      // [V]
  std::vector<uint32_t> pat;     // [max(m, 1)] the distinct patterns of the scored rows, ascending
  int m = 0;                     // how many there are; 0: every score is NaN -- no histogram, and the scan counts nothing
};
inline void family_walk(const double* obs, int64_t V, FamilyWalk& w) {
  w.order.assign((size_t)V, 0);
  for (int64_t v = 0; v < V; v++) w.order[(size_t)v] = v;
  std::stable_sort(w.order.begin(), w.order.end(), [&](int64_t x, int64_t y) {
    const double a = obs[x], b = obs[y];
    const bool na = a != a, nb = b != b;
    return (na || nb) ? (na && !nb) : a < b;
  });
  w.rank.assign((size_t)V, 0u);
  w.meta.assign((size_t)((V + 63) / 64 * 64), 0u);
  w.gstart.assign((size_t)V, 0);
  w.bin.assign((size_t)V, -1);
  w.pat.clear();
  for (int64_t i = 0; i < V; i++) {
    const double o = obs[w.order[(size_t)i]];
    w.rank[(size_t)w.order[(size_t)i]] = (uint32_t)i;
    const uint32_t thr = f32_threshold(o);
    const bool end = i + 1 == V || !(obs[w.order[(size_t)(i + 1)]] == o);
    w.meta[(size_t)i] = thr | (end ? 0x80000000u : 0u);
    w.gstart[(size_t)i] = i > 0 && obs[w.order[(size_t)(i - 1)]] == o ? w.gstart[(size_t)(i - 1)] : i;
    if (o != o) continue;
    if (w.pat.empty() || w.pat.back() != thr) w.pat.push_back(thr);   // (ascending: the threshold is monotone in the score)
    w.bin[(size_t)i] = (int64_t)w.pat.size() - 1;
  }
  w.m = (int)w.pat.size();
  if (w.pat.empty()) w.pat.push_back(0u);
}

// The finish: sd [V] the step-down counts as the device left them, at the last row of every tie group, and hist [max(m, 1)]
// the pooled histogram per bin.  The suffix sums make hist the exceedances per bin, a tie group's count goes to its other
// rows, and row i of the walk writes the record of set vset[order[i]] (a NaN score keeps 0 / 0 / 0).
inline void family_finish(const FamilyWalk& w, const int64_t* vset, uint32_t* sd, unsigned long long* hist, gcre_family_score* fam) {
  const int64_t V = (int64_t)w.order.size();
  for (int b = w.m - 2; b >= 0; b--) hist[b] += hist[b + 1];
  for (int64_t i = V - 2; i >= 0; i--)
    if (!(w.meta[(size_t)i] >> 31)) sd[i] = sd[i + 1];
  for (int64_t i = 0; i < V; i++) {
    if (w.bin[(size_t)i] < 0) continue;
    gcre_family_score& f = fam[vset[w.order[(size_t)i]]];
    f.n_ge_stepdown = (int64_t)sd[i];
    f.exceed = hist[w.bin[(size_t)i]];
    f.observed = V - w.gstart[(size_t)i];
  }
}

}  // namespace gcre_family

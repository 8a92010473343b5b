// gcre_minp.h -- the host plan of the min-P set tests (gcre_score_sets_minp), defined once: the slab of whole
// rows, the walk order with its tie groups, and the finish of the device's counts and minima.  Plain C++17 over
// include/gcre_hip.h, no HIP: the host stage (gcre_host_minp.hip) includes it under hipcc and tests/native/family_main.cpp
// under plain g++.
#pragma once
#include "../../include/gcre_hip.h"
#include "gcre_env.h"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

namespace gcre_minp __attribute__((visibility("hidden"))) {

// GCRE_MINP_MAX_MB: the bound on the null scores and counts a slab holds on the device, read per call (tests set fractions);
// default 1024.  GCRE_MINP_SLAB_SETS (tests) bounds the rows of a slab further; 0 = no bound.
inline double minp_max_mb() { return gcre_env::env_mb("GCRE_MINP_MAX_MB", 1024, 1048576.0); }
inline int64_t minp_slab_sets() { return gcre_env::env_count("GCRE_MINP_SLAB_SETS"); }

// The slab: whole rows -- every tile of `tile` permutations of a valid set, its null scores and its counts, 8 bytes per
// column -- under `max_mb`, and at most `slab_sets` rows (0: no such bound).  One row above the limit is refused.  Without a
// valid set or a permutation there is no slab (0).
inline int minp_slab(int64_t V, int K, int tile, double max_mb, int64_t slab_sets, const std::string& who, int64_t& slab_rows,
                     std::string& msg) {
  slab_rows = 0;
  if (V == 0 || K == 0) return GCRE_OK;
  const int64_t tiles = ((int64_t)K + tile - 1) / tile;
  const double row_bytes = (double)tiles * tile * 8.0;
  if (row_bytes > max_mb * 1048576.0) {
    msg = who + ": the null scores and counts of one set under " + std::to_string(tiles) + " tiles of " + std::to_string(tile) +
          " permutations exceed GCRE_MINP_MAX_MB";
    return GCRE_ERR_ARG;
  }
  slab_rows = std::min<int64_t>(V, (int64_t)(max_mb * 1048576.0 / row_bytes));
  if (slab_sets > 0) slab_rows = std::min<int64_t>(slab_rows, slab_sets);
  return GCRE_OK;
}

// The walk: NaN scores first, then the sets' own counts c = ge descending; stable.  Per row of the walk meta = c, with bit 31
// set where the row ends a tie group that is counted: a run of equal c among the scored sets (c <= iterations < 2^31).
struct MinpWalk {
  std::vector<uint32_t> order;   // [V] row of the walk -> valid set
  std::vector<uint32_t> meta;    // [V]
};
inline void minp_walk(const double* obs, const unsigned long long* ge, int64_t V, MinpWalk& w) {
  auto is_nan = [&](uint32_t v) { return obs[v] != obs[v]; };
  w.order.resize((size_t)V);
  for (int64_t v = 0; v < V; v++) w.order[(size_t)v] = (uint32_t)v;
  std::stable_sort(w.order.begin(), w.order.end(), [&](uint32_t x, uint32_t y) {
    const bool nx = is_nan(x), ny = is_nan(y);
    return (nx || ny) ? (nx && !ny) : ge[x] > ge[y];
  });
  w.meta.resize((size_t)V);
  for (int64_t i = 0; i < V; i++) {
    const uint32_t v = w.order[(size_t)i];
    const bool end = !is_nan(v) && (i + 1 == V || ge[w.order[(size_t)(i + 1)]] != ge[v]);   // (NaN rows come first: none follows)
    w.meta[(size_t)i] = (uint32_t)ge[v] | (end ? 0x80000000u : 0u);
  }
}

// The finish: le [V] the step-down counts as the device left them, at the last row of every tie group, and q [K] the minimum
// count of every permutation, which is sorted here.  A tie group's count goes to its other rows, and row i of the walk
// writes the record of set vset[order[i]]: n_le_minp = the minima at or below its c (a NaN score keeps 0 / 0).
inline void minp_finish(const MinpWalk& w, const double* obs, const unsigned long long* ge, const int64_t* vset, uint32_t* le,
                        std::vector<uint32_t>& q, gcre_minp_score* mp) {
  const int64_t V = (int64_t)w.order.size();
  auto is_nan = [&](uint32_t v) { return obs[v] != obs[v]; };
  std::sort(q.begin(), q.end());
  for (int64_t i = V - 2; i >= 0; i--)
    if (!(w.meta[(size_t)i] >> 31) && !is_nan(w.order[(size_t)i])) le[i] = le[i + 1];
  for (int64_t i = 0; i < V; i++) {
    const uint32_t v = w.order[(size_t)i];
    if (is_nan(v)) continue;
    gcre_minp_score& m = mp[vset[v]];
    m.n_le_stepdown = (int64_t)le[i];
    m.n_le_minp = (int64_t)(std::upper_bound(q.begin(), q.end(), (uint32_t)ge[v]) - q.begin());
  }
}

}  // namespace gcre_minp

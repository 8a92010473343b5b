// gcre_clumporder.h -- what gcre_clump_sets (gcre_host_stats.hip) refuses of its rule, of its walk order and of its size
// before anything is launched.  Plain C++17 over include/gcre_hip.h and gcre_setlists.h, no HIP:
// tests/native/clump_main.cpp drives it on a machine without a GPU.  DESIGN.md §3.11.
#pragma once
#include "gcre_setlists.h"

#include <algorithm>
#include <cstdlib>

namespace gcre_host __attribute__((visibility("hidden"))) {

// The rule: r in (0, 1] (a NaN fails both comparisons), measure 0 jaccard / 1 containment, patients 0 all / 1 cases.
inline int check_clump_rule(double r, int measure, int patients, std::string& msg) {
  if (!(r > 0.0 && r <= 1.0))
    msg = "clump_sets: r must be > 0 and <= 1, not " + std::to_string(r);
  else if (measure != 0 && measure != 1)
    msg = "clump_sets: measure must be 0 (jaccard) or 1 (containment), not " + std::to_string(measure);
  else if (patients != 0 && patients != 1)
    msg = "clump_sets: patients must be 0 (all) or 1 (cases), not " + std::to_string(patients);
  else
    return GCRE_OK;
  return GCRE_ERR_ARG;
}

// The walk order over a set list that passed check_set_shape and check_set_members: every entry names a set, no set is
// named twice, and no named set has an NA member.
inline int check_clump_order(const gcre_set_input* in, const int64_t* order, int64_t n_order, std::string& msg) {
  const int64_t S = in->n_sets;
  if (n_order < 0 || (n_order > 0 && !order)) {
    msg = "clump_sets: bad order (a negative length or a NULL array)";
    return GCRE_ERR_ARG;
  }
  std::vector<unsigned char> seen((size_t)S, 0);
  for (int64_t i = 0; i < n_order; i++) {
    const int64_t s = order[i];
    const std::string at = "clump_sets: order[" + std::to_string(i) + "] = " + std::to_string(s);
    if (s < 0 || s >= S) {
      msg = at + " out of range (" + std::to_string(S) + " sets)";
      return GCRE_ERR_RANGE;
    }
    if (seen[(size_t)s]) {
      msg = at + " is listed twice";
      return GCRE_ERR_ARG;
    }
    seen[(size_t)s] = 1;
    if (!set_is_valid(in, s)) {
      msg = at + " names a set with an NA member";
      return GCRE_ERR_ARG;
    }
  }
  return GCRE_OK;
}

// GCRE_CLUMP_MAX_MB: the bound on the union rows the device holds, read per call (tests set fractions); default 32768
inline double clump_max_mb() { return gcre_env::env_mb("GCRE_CLUMP_MAX_MB", 32768, 65536.0); }

// n_order union rows of row_bytes each against the bound
inline int check_clump_bytes(int64_t n_order, int64_t row_bytes, double max_mb, std::string& msg) {
  if ((double)n_order * (double)row_bytes <= max_mb * 1048576.0) return GCRE_OK;
  msg = "clump_sets: " + std::to_string(n_order) + " rows of " + std::to_string(row_bytes) + " bytes exceed GCRE_CLUMP_MAX_MB = " +
        std::to_string(max_mb);
  return GCRE_ERR_ARG;
}

}  // namespace gcre_host

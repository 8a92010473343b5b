// gcre_dose.h -- the host plan of the multi-hit set tests (gcre_score_sets_dose): what the entry refuses of
// its own arguments.  The slabs of whole sets and the block table are gcre_prefix.h's own (prefix_slabs, prefix_blocks), with
// n_levels rows for every valid set.  Plain C++17 over include/gcre_hip.h, no HIP: the host stage (gcre_host_steps.hip, through
// gcre_steps.h) includes it under hipcc and tests/native/dose_main.cpp under plain g++.
#pragma once
#include "gcre_prefix.h"

namespace gcre_dose __attribute__((visibility("hidden"))) {

constexpr int kDoseMaxLevel = GCRE_DOSE_MAX_LEVEL;   // the 4-plane counter of k_dose_rows counts to 15; beyond, a sticky plane
static_assert(kDoseMaxLevel == 15, "four planes");

// The levels as k_dose_rows takes them: level i in bits [4 i, 4 i + 4)
inline uint64_t pack_levels(const int32_t* levels, int32_t n_levels) {
  uint64_t p = 0;
  for (int32_t i = 0; i < n_levels; i++) p |= (uint64_t)(levels[i] & 15) << (4 * i);
  return p;
}

// What gcre_score_sets_dose refuses of its own arguments, after the checks of the set list (gcre_setlists.h) passed.  With
// permutations (iterations > 0) the n_levels level rows of one valid set (and its null_max row, when asked) must fit `max_mb`:
// the sets are walked in slabs of whole sets.
inline int check_dose_args(const gcre_set_input* in, const int32_t* levels, int32_t n_levels, bool have_out, int32_t iterations,
                           int method, int32_t W32p, int32_t Kpad, bool want_null, double max_mb, const std::string& who,
                           std::string& msg) {
  const int64_t S = in->n_sets;
  if (!have_out) { msg = who + ": NULL argument (dose_out)"; return GCRE_ERR_ARG; }
  if (n_levels < 1 || n_levels > kDoseMaxLevel) {
    msg = who + ": n_levels = " + std::to_string(n_levels) + ": 1 .. " + std::to_string(kDoseMaxLevel) + " levels";
    return GCRE_ERR_ARG;
  }
  if (!levels) { msg = who + ": NULL argument (levels)"; return GCRE_ERR_ARG; }
  for (int32_t i = 0; i < n_levels; i++) {
    if (levels[i] < 1 || levels[i] > kDoseMaxLevel) {
      msg = who + ": level " + std::to_string(levels[i]) + " (index " + std::to_string(i) + ") is outside 1 .. " + std::to_string(kDoseMaxLevel);
      return GCRE_ERR_ARG;
    }
    if (i > 0 && levels[i] <= levels[i - 1]) {
      msg = who + ": the levels are not strictly ascending (" + std::to_string(levels[i]) + " after " + std::to_string(levels[i - 1]) + ")";
      return GCRE_ERR_ARG;
    }
  }
  if (S > 0x7fffffff || (S > 0 && in->set_off[S] > 0x7fffffff)) { msg = who + ": too many sets or members"; return GCRE_ERR_ARG; }
  if (iterations <= 0) return GCRE_OK;
  // every valid set has the same rows: the first one names the refusal
  const double bytes = gcre_prefix::prefix_set_bytes(n_levels, method, W32p, Kpad, want_null);
  if (bytes > max_mb * 1048576.0)
    for (int64_t s = 0; s < S; s++) {
      if (!gcre_prefix::prefix_set_valid(in, s)) continue;   // never launched
      msg = who + ": the " + std::to_string(n_levels) + " level rows of set " + std::to_string(s) + " take " + std::to_string((int64_t)bytes) +
            " bytes: above GCRE_PREFIX_MAX_MB = " + std::to_string(max_mb);
      return GCRE_ERR_ARG;
    }
  return GCRE_OK;
}

}  // namespace gcre_dose

// gcre_seq_prefix.h -- the host plan of the sequential p-values of the two adaptive set tests
// (gcre_score_sets_prefix_sequential, gcre_score_sets_dose_sequential), defined once: what the entries refuse
// of their own arguments, the first active list of a slab, what the slabs of a call add up to and how many kernels it
// launches.  The steps and the slabs of whole sets are gcre_prefix.h's, the levels gcre_dose.h's, the stopping rule and the
// batch schedule gcre_sequential.h's.  Plain C++17 over include/gcre_hip.h, no HIP: the host stage
// (gcre_host_seq_prefix.hip, through gcre_steps.h) includes it under hipcc and tests/native/seq_prefix_main.cpp under plain g++.
// tests/test_seq_prefix_host.py restates it in Python.
//
// Slabs.  The sequential loop runs once per slab of gcre_prefix.h, from permutation 0, and draws the masks again: they are a
// function of (seed, r), so no result depends on the slabs; a second slab pays for the draw a second time.
#pragma once
#include "gcre_dose.h"
#include "gcre_prefix.h"
#include "gcre_sequential.h"

namespace gcre_seq_prefix __attribute__((visibility("hidden"))) {

// What gcre_score_sets_prefix_sequential refuses of its own arguments, after the checks of the set list passed: the prefix
// entry's refusals without a null_max matrix (the step rows of one set must fit GCRE_PREFIX_MAX_MB where permutations are
// drawn), then the sequential entry's.
inline int check_seq_prefix_args(const gcre_set_input* in, const gcre_prefix::PrefixSteps& st, bool have_px, bool have_seq, int method,
                                 int32_t W32p, double max_mb, int64_t h, int64_t max_perms, const std::string& who, std::string& msg) {
  if (int rc = gcre_prefix::check_prefix_args(in, st, have_px, max_perms > 0 ? 1 : 0, method, W32p, 0, false, max_mb, who, msg)) return rc;
  return gcre_sequential::check_sequential_args(h, max_perms, have_seq, who, msg);
}

// The same for gcre_score_sets_dose_sequential
inline int check_seq_dose_args(const gcre_set_input* in, const int32_t* levels, int32_t n_levels, bool have_out, bool have_seq,
                               int method, int32_t W32p, double max_mb, int64_t h, int64_t max_perms, const std::string& who,
                               std::string& msg) {
  if (int rc = gcre_dose::check_dose_args(in, levels, n_levels, have_out, max_perms > 0 ? 1 : 0, method, W32p, 0, false, max_mb, who, msg))
    return rc;
  return gcre_sequential::check_sequential_args(h, max_perms, have_seq, who, msg);
}

// The first active list of a slab: its slots by step count descending, ties by slot -- prefix_blocks' order, so that the four
// sets of a group of k_seq_prefix_null are alike.  `score_nan` [nv]: the slot's best observed score is NaN (every step is).
// Uniform call: such a slot is never reached and is left off.  Weighted call: it stays on, never stops, and so forces the
// refusal at a left-over permutation (gcre_seq_weighted.h).
inline void first_active(const int64_t* vsteps, int64_t nv, const uint8_t* score_nan, bool weighted, std::vector<uint32_t>& act) {
  std::vector<int32_t> order;
  std::vector<gcre_prefix::PrefixWave> waves;
  gcre_prefix::prefix_blocks(vsteps, nv, order, waves);
  act.clear();
  for (int32_t e : order)
    if (!score_nan[e] || weighted) act.push_back((uint32_t)e);
}

// What the slabs of one call add up to.  R, its stratum and the cap are functions of the inputs alone, so every slab that
// reaches R reports the same; the sets still active there are summed.
struct SeqPrefixTotals {
  int64_t left_over = -1;
  int left_stratum = -1;
  int64_t n_active = 0;     // sets still active at R, over the slabs that reached it
  // one slab behind its loop: the R it met (-1: none), R's stratum and the sets it still had active there
  void add(int64_t slab_left_over, int slab_stratum, int64_t slab_active) {
    if (slab_left_over < 0) return;
    left_over = slab_left_over;
    left_stratum = slab_stratum;
    n_active += slab_active;
  }
  bool refused() const { return left_over >= 0 && n_active > 0; }
};

// kernels of one slab: rows, observed scores, pick; then per batch masks (uniform: one kernel; weighted: search and write),
// the null kernel and the retirement
inline int64_t seq_prefix_slab_launches(int64_t batches, bool weighted) { return 3 + (weighted ? 4 : 3) * batches; }

}  // namespace gcre_seq_prefix

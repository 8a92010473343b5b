// gcre_seq_weighted.h -- the rule of the weighted sequential p-values (gcre_score_sets_sequential_weighted),
// defined once: which permutations of a batch are drawn and scored when one of them has no accepted attempt, when the call
// is refused, what it then says, and how many dwords a permutation of a batch takes.  Plain C++17 over gcre_weighted.h (the
// law, the thresholds, the draw: wt_*) and gcre_sequential.h (the stopping rule and the batch schedule): the kernels of
// gcre_seq_weighted.hip include it under hipcc, the host stage (gcre_host_sequential.hip) too, and
// tests/native/seq_weighted_main.cpp under plain g++.  report.weighted_sequential_reference restates it in Python.
//
// Masks.  Permutation r of the call is, bit for bit, mask r of gcre_generate_weighted_masks(seed, odds, stratum, n_strata,
// max_attempts): thresholds from weighted_plan, a*(r, s) the smallest accepted attempt below the cap.  r is 64-bit from the
// batch's first permutation onwards: wt_key takes it whole.
//
// Left-over permutations.  R = the smallest r < max_perms for which some stratum has no accepted attempt below max_attempts
// (none: infinity).  The sequential rule of gcre_sequential.h is applied to permutations 0 .. min(max_perms, R) - 1.  R >=
// max_perms: the usual answer.  R < max_perms and every scored set stopped with n_perm <= R: the answer is complete.
// Otherwise -- a set still active behind permutation R - 1; a set with a NaN score always is -- the call is refused with
// GCRE_ERR_RANGE.  The batches only find R: a batch [r0, r0 + nb) that holds R is cut to [r0, R), nothing is drawn or scored
// at and beyond R, and the loop ends behind it.  A set is active behind the cut batch exactly when it has fewer than h
// exceedances in [0, R): a function of the inputs, not of the batches.
#pragma once
#include "gcre_sequential.h"
#include "gcre_weighted.h"

namespace gcre_seq_weighted __attribute__((visibility("hidden"))) {

constexpr uint32_t kSeqWtNoColumn = 0xffffffffu;   // the first left-over column of a batch without one (columns are < 2^30)

// dwords per permutation of a batch, for sequential_batch: its mask and its accepted attempts
inline int32_t seq_weighted_dwords(int32_t W32p, int n_strata) { return W32p + n_strata; }

// One batch behind its search.  `first`: the smallest column of the batch whose permutation has a stratum without an
// accepted attempt, or kSeqWtNoColumn.
struct SeqWeightedCut {
  int64_t keep;        // the permutations of the batch that are drawn and scored: r0 .. r0 + keep - 1
  int64_t left_over;   // R, or -1: the batch holds none
};
inline SeqWeightedCut seq_weighted_cut(int64_t r0, int64_t nb, uint32_t first) {
  if (first == kSeqWtNoColumn || (int64_t)first >= nb) return {nb, -1};
  return {(int64_t)first, r0 + (int64_t)first};
}

// behind the cut batch (left_over >= 0; n_active: the sets that have not stopped in [0, R)): refused or complete
inline bool seq_weighted_refused(int64_t left_over, int64_t n_active) { return left_over >= 0 && n_active > 0; }

// kernels of one batch: the search alone when nothing remains in front of R, else search, write, null, retire
inline int seq_weighted_batch_launches(const SeqWeightedCut& cut) { return cut.keep > 0 ? 4 : 1; }

// the stratum the message names: the smallest one without an accepted attempt.  att[s * stride + column]
inline int seq_weighted_left_stratum(const uint32_t* att, int n_strata, size_t stride, size_t column) {
  for (int s = 0; s < n_strata; s++)
    if (att[(size_t)s * stride + column] == gcre_weighted::kWeightedNone) return s;
  return -1;
}

inline std::string seq_weighted_message(const std::string& who, int64_t left_over, int stratum, uint32_t cap, int64_t n_active,
                                        int64_t max_perms) {
  return who + ": permutation " + std::to_string(left_over) + " has no accepted attempt below max_attempts = " + std::to_string(cap) +
         " in stratum " + std::to_string(stratum) + ", and " + std::to_string(n_active) + " sets were still active there (max_perms = " +
         std::to_string(max_perms) + "): raise max_attempts or lower max_perms";
}

}  // namespace gcre_seq_weighted

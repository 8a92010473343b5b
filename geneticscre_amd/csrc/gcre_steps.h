// gcre_steps.h -- what the variable-threshold test, the multi-hit test (§3.20) and their sequential forms
// (§3.25) differ in on the host, defined once: the two row variants.  A variant holds what its entry takes and returns beside
// the set records and supplies the argument checks (gcre_prefix.h, gcre_dose.h, gcre_seq_prefix.h), the steps of every valid
// set, the defaults of its records and what one pick of the device writes into them.  n_ge is the caller's: the resident
// stage writes the device's count, the sequential stage leaves the default.  Plain C++17 over include/gcre_hip.h, no HIP:
// StepRows (gcre_step_rows.h) is built on a variant under hipcc, tests/native/steps_main.cpp drives both under plain g++.
#pragma once
#include "gcre_seq_prefix.h"

#include <cstring>
#include <limits>

namespace gcre_steps __attribute__((visibility("hidden"))) {

// first step row of every slot of the slab of valid sets [v0, v0 + nv): the running sum of their steps.  row0 [nv + 1]
inline void slab_row0(const std::vector<int64_t>& vsteps, int64_t v0, int64_t nv, std::vector<int64_t>& row0) {
  row0.assign((size_t)nv + 1, 0);
  for (int64_t e = 0; e < nv; e++) row0[(size_t)e + 1] = row0[(size_t)e] + vsteps[(size_t)(v0 + e)];
}

// What both records share.  Before the device has run: an invalid set -1, a NaN score, zeros.  And of a pick (PrefixPick of
// gcre_kernels.h): its score and the counts of its step.
template <typename Rec>
void default_record(Rec& x, bool valid) {
  std::memset(&x, 0, sizeof x);
  x.score = std::numeric_limits<double>::quiet_NaN();
  x.n_ge = valid ? 0 : -1;
}
template <typename Rec, typename Pick>
void pick_record(Rec& x, const Pick& p) {
  x.score = p.score;
  x.cases_pos = p.cnt[0];
  x.ctrls_pos = p.cnt[1];
  x.cases_neg = p.cnt[2];
  x.ctrls_neg = p.cnt[3];
}

// The variable-threshold test: the steps of a set are the prefixes of its member list that end at a cut member
struct PrefixRows {
  const uint8_t* cut;        // [members of the list] or NULL
  gcre_prefix_score* rec;    // [n_sets]
  double* scores;            // step_scores: optional [members of the list]
  gcre_prefix::PrefixSteps st = {};   // the steps of every set, from the checks

  // the refusal that precedes the steps, then the steps
  bool steps(const gcre_set_input* in, const std::string& who, std::string& msg) {
    if (in->n_sets > 0x7fffffff || (in->n_sets > 0 && in->set_off[in->n_sets] > 0x7fffffff)) {
      msg = who + ": too many sets or members";
      return false;
    }
    gcre_prefix::prefix_steps(in, cut, st);
    return true;
  }
  int check(const gcre_set_input* in, int32_t iterations, int method, int32_t W32p, int32_t Kpad, bool want_null, double max_mb,
            const std::string& who, std::string& msg) {
    if (!steps(in, who, msg)) return GCRE_ERR_ARG;
    return gcre_prefix::check_prefix_args(in, st, rec != nullptr, iterations, method, W32p, Kpad, want_null, max_mb, who, msg);
  }
  int check_seq(const gcre_set_input* in, bool have_seq, int method, int32_t W32p, double max_mb, int64_t h, int64_t max_perms,
                const std::string& who, std::string& msg) {
    if (!steps(in, who, msg)) return GCRE_ERR_ARG;
    return gcre_seq_prefix::check_seq_prefix_args(in, st, rec != nullptr, have_seq, method, W32p, max_mb, h, max_perms, who, msg);
  }
  int64_t steps_of(int64_t s) const { return st.off[(size_t)s + 1] - st.off[(size_t)s]; }
  void vsteps(const std::vector<int64_t>& vset, std::vector<int64_t>& out) const {
    out.resize(vset.size());
    for (size_t v = 0; v < vset.size(); v++) out[v] = steps_of(vset[v]);
  }
  // no best step without a permutation
  void defaults(const gcre_set_input* in, const gcre_set_score* out) const {
    const int64_t S = in->n_sets;
    for (int64_t s = 0; s < S; s++) {
      default_record(rec[s], out[s].valid);
      rec[s].best_step = -1;
      rec[s].steps = (int32_t)steps_of(s);
    }
    if (scores && S > 0) std::fill(scores, scores + (size_t)in->set_off[S], std::numeric_limits<double>::quiet_NaN());
  }
  // the pick of set s; obs_rows: the observed scores of its step rows, read where the step scores are asked for
  template <typename Pick>
  void write(int64_t s, const Pick& p, const double* obs_rows) const {
    gcre_prefix_score& x = rec[s];
    pick_record(x, p);
    x.best_step = p.best_step;
    x.best_members = p.best_step >= 0 ? st.members[(size_t)(st.off[(size_t)s] + p.best_step)] : 0;
    for (int64_t k = 0; scores && k < steps_of(s); k++) scores[st.end[(size_t)(st.off[(size_t)s] + k)]] = obs_rows[k];
  }
};

// The multi-hit test: step k of every set is "carries at least levels[k] of its members"
struct DoseRows {
  static constexpr const uint8_t* cut = nullptr;
  const int32_t* levels;     // [n_levels]
  int32_t n_levels;
  gcre_dose_score* rec;      // [n_sets]
  double* scores;            // level_scores: optional [n_sets][n_levels]

  int check(const gcre_set_input* in, int32_t iterations, int method, int32_t W32p, int32_t Kpad, bool want_null, double max_mb,
            const std::string& who, std::string& msg) {
    return gcre_dose::check_dose_args(in, levels, n_levels, rec != nullptr, iterations, method, W32p, Kpad, want_null, max_mb, who, msg);
  }
  int check_seq(const gcre_set_input* in, bool have_seq, int method, int32_t W32p, double max_mb, int64_t h, int64_t max_perms,
                const std::string& who, std::string& msg) {
    return gcre_seq_prefix::check_seq_dose_args(in, levels, n_levels, rec != nullptr, have_seq, method, W32p, max_mb, h, max_perms, who,
                                                msg);
  }
  void vsteps(const std::vector<int64_t>& vset, std::vector<int64_t>& out) const { out.assign(vset.size(), (int64_t)n_levels); }
  // no best level without a permutation
  void defaults(const gcre_set_input* in, const gcre_set_score* out) const {
    const int64_t S = in->n_sets;
    for (int64_t s = 0; s < S; s++) {
      default_record(rec[s], out[s].valid);
      rec[s].best_index = -1;
      rec[s].levels = n_levels;
    }
    if (scores) std::fill(scores, scores + (size_t)S * (size_t)n_levels, std::numeric_limits<double>::quiet_NaN());
  }
  template <typename Pick>
  void write(int64_t s, const Pick& p, const double* obs_rows) const {
    gcre_dose_score& x = rec[s];
    pick_record(x, p);
    x.best_index = p.best_step;
    x.best_level = p.best_step >= 0 ? levels[p.best_step] : 0;
    if (scores) std::copy(obs_rows, obs_rows + n_levels, scores + (size_t)s * (size_t)n_levels);
  }
};

}  // namespace gcre_steps

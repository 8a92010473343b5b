// gcre_setlists.h -- the host stage that gcre_score_sets (gcre_host_sets.hip), gcre_set_overlap and gcre_exceed_stepdown
// (gcre_host_stats.hip) share:
// what they refuse of a caller's set list, and the union rows and counts of one set.  Plain C++17 over include/gcre_hip.h, no
// HIP: tests/native/setlists_main.cpp drives it on a machine without a GPU (given_main.cpp, patients_main.cpp and
// burden_main.cpp: the argument checks of gcre_score_sets_given, gcre_set_patient_counts and gcre_patient_burden).
#pragma once
#include "../../include/gcre_hip.h"
#include "gcre_env.h"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

namespace gcre_host __attribute__((visibility("hidden"))) {

// The two checks return a code and leave the message in `msg`; `who` opens it.  They are separate so that an entry can put
// checks of its own between them.

// The shape of the input: the column count against the context's n patients, negative counts, NULL arrays.
inline int check_set_shape(const gcre_set_input* in, int n, const std::string& who, std::string& msg) {
  const int64_t S = in->n_sets;
  if (in->n_cols != n)
    msg = who + ": the rows have " + std::to_string(in->n_cols) + " columns, not n_cases + n_ctrls = " + std::to_string(n);
  else if (S < 0 || in->n_rows < 0 || (S > 0 && (!in->set_off || !in->members)) || (in->n_rows > 0 && !in->rows))
    msg = who + ": bad input (a negative count or a NULL array)";
  else
    return GCRE_OK;
  return GCRE_ERR_ARG;
}

// Every set's members and signs: no empty set, rows -1 (NA) .. n_rows - 1, signs +1 or -1.
inline int check_set_members(const gcre_set_input* in, const std::string& who, std::string& msg) {
  auto bad = [&](int code, int64_t s, const std::string& what) {
    msg = who + ": set " + std::to_string(s) + what;
    return code;
  };
  for (int64_t s = 0; s < in->n_sets; s++) {
    const int64_t b = in->set_off[s], e = in->set_off[s + 1];
    if (b < 0 || e <= b) return bad(GCRE_ERR_ARG, s, " has no members");
    for (int64_t i = b; i < e; i++) {
      const int32_t row = in->members[i];
      if (row < -1 || row >= in->n_rows)
        return bad(GCRE_ERR_RANGE, s, ": member row " + std::to_string(row) + " out of range (" + std::to_string(in->n_rows) + " rows)");
      if (in->signs && in->signs[i] != 1 && in->signs[i] != -1)
        return bad(GCRE_ERR_ARG, s, ": sign " + std::to_string(in->signs[i]) + " is neither +1 nor -1");
    }
  }
  return GCRE_OK;
}

// no member of set s is NA
inline bool set_is_valid(const gcre_set_input* in, int64_t s) {
  bool valid = true;
  for (int64_t i = in->set_off[s]; i < in->set_off[s + 1]; i++) valid = valid && in->members[i] >= 0;
  return valid;
}

// The index lists of gcre_score_sets_given, after the two checks above passed: `which` [n_which] names the sets to score
// (NULL: 0 .. n_sets - 1, and then n_which must be n_sets), `given` [n_which] the set whose carriers are set aside (-1 or
// NULL: none), which must not have an NA member; `cap` records are there to be written.
inline int check_given_index(const gcre_set_input* in, const int64_t* which, const int64_t* given, int64_t n_which,
                             int64_t cap, const std::string& who, std::string& msg) {
  const int64_t S = in->n_sets;
  if (n_which < 0 || (!which && n_which != S)) {
    msg = who + ": bad index list (a negative length, or NULL `which` with a length other than n_sets)";
    return GCRE_ERR_ARG;
  }
  for (int64_t i = 0; i < n_which; i++) {
    if (which && (which[i] < 0 || which[i] >= S)) {
      msg = who + ": which[" + std::to_string(i) + "] = " + std::to_string(which[i]) + " out of range (" + std::to_string(S) + " sets)";
      return GCRE_ERR_RANGE;
    }
    if (given && (given[i] < -1 || given[i] >= S)) {
      msg = who + ": given[" + std::to_string(i) + "] = " + std::to_string(given[i]) + " out of range (" + std::to_string(S) + " sets, -1 = none)";
      return GCRE_ERR_RANGE;
    }
  }
  for (int64_t i = 0; given && i < n_which; i++)
    if (given[i] >= 0 && !set_is_valid(in, given[i])) {
      msg = who + ": given[" + std::to_string(i) + "] = set " + std::to_string(given[i]) + " has an NA member: its carriers are not known";
      return GCRE_ERR_ARG;
    }
  if (n_which > cap) {
    msg = who + ": " + std::to_string(n_which) + " entries, room for " + std::to_string(cap) + " records (out of range)";
    return GCRE_ERR_RANGE;
  }
  return GCRE_OK;
}

// GCRE_PATIENT_MAX_MB: the bound on the count cells (and on the member table) gcre_set_patient_counts holds on the device,
// read per call (tests set fractions); default 1024
inline double patient_max_mb() { return gcre_env::env_mb("GCRE_PATIENT_MAX_MB", 1024, 65536.0); }

// What gcre_set_patient_counts refuses of its own arguments, after the two checks above passed: `which` [n_which] names the
// sets to count (NULL: 0 .. n_sets - 1, and then n_which must be n_sets), `group` [n_which] the group of every entry (-1:
// not counted; NULL: group 0, and then n_groups must be 1); H = 1 + by_sign planes of n_cols int32 cells per group against
// `max_mb`.  Fewer than 2^31 - 16 entries, so that a 32-bit cell cannot overflow.
inline int check_patient_index(const gcre_set_input* in, const int64_t* which, int64_t n_which, const int32_t* group,
                               int32_t n_groups, int by_sign, bool have_counts, double max_mb, const std::string& who,
                               std::string& msg) {
  const int64_t S = in->n_sets;
  if (by_sign != 0 && by_sign != 1)
    msg = who + ": by_sign must be 0 or 1, not " + std::to_string(by_sign);
  else if (n_groups < 1)
    msg = who + ": n_groups must be at least 1, not " + std::to_string(n_groups);
  else if (n_which < 0 || (!which && n_which != S))
    msg = who + ": bad index list (a negative length, or NULL `which` with a length other than n_sets)";
  else if (!group && n_groups != 1)
    msg = who + ": NULL `group` puts every entry in group 0: n_groups must be 1, not " + std::to_string(n_groups);
  else if (!have_counts)
    msg = who + ": NULL counts";
  else if (n_which >= 0x7fffffff - 16)
    msg = who + ": " + std::to_string(n_which) + " entries: a 32-bit count could overflow (fewer than 2^31 - 16)";
  else if ((double)n_groups * (double)(1 + by_sign) * (double)in->n_cols * 4.0 > max_mb * 1048576.0)
    msg = who + ": " + std::to_string(n_groups) + " groups x " + std::to_string(1 + by_sign) + " planes x " +
          std::to_string(in->n_cols) + " patients x 4 bytes exceed GCRE_PATIENT_MAX_MB = " + std::to_string(max_mb);
  else {
    for (int64_t i = 0; i < n_which; i++) {
      if (which && (which[i] < 0 || which[i] >= S)) {
        msg = who + ": which[" + std::to_string(i) + "] = " + std::to_string(which[i]) + " out of range (" + std::to_string(S) + " sets)";
        return GCRE_ERR_RANGE;
      }
      if (group && (group[i] < -1 || group[i] >= n_groups)) {
        msg = who + ": group[" + std::to_string(i) + "] = " + std::to_string(group[i]) + " out of range (" + std::to_string(n_groups) +
              " groups, -1 = not counted)";
        return GCRE_ERR_RANGE;
      }
    }
    return GCRE_OK;
  }
  return GCRE_ERR_ARG;
}

// GCRE_BURDEN_MAX_MB: the bound on the bit planes and the sums gcre_patient_burden holds on the device at one time, read
// per call (tests set fractions); default 1024
inline double burden_max_mb() { return gcre_env::env_mb("GCRE_BURDEN_MAX_MB", 1024, 65536.0); }

// the bit length of a non-negative weight: the planes a row whose largest weight it is needs
inline int32_t burden_bit_length(int32_t v) {
  int32_t b = 0;
  for (uint32_t u = (uint32_t)v; u != 0; u >>= 1) b++;
  return b;
}

// What gcre_patient_burden refuses of its arguments: weights [n_rows][n_cols], >= 0, on a context of `n_patients` patients,
// `iterations` permutations (`have_masks`: set) whose masks are [W32p][Kpad] dwords.  planes[g] = the bit length of row
// g's largest weight; a row's device bytes are its planes of W32p dwords and its Kpad 64-bit sums, and the largest row's
// must fit `max_mb` (the rows are walked in slabs).
inline int check_burden_args(const int32_t* weights, int64_t n_rows, int32_t n_cols, int32_t n_patients, bool have_out,
                             int32_t iterations, bool have_masks, int32_t W32p, int32_t Kpad, double max_mb,
                             const std::string& who, std::vector<int32_t>& planes, std::string& msg) {
  planes.clear();
  if (!have_out)
    msg = who + ": NULL out";
  else if (n_rows < 0)
    msg = who + ": n_rows must not be negative, not " + std::to_string(n_rows);
  else if (!weights && n_rows > 0)
    msg = who + ": NULL weights with " + std::to_string(n_rows) + " rows";
  else if (n_cols != n_patients)
    msg = who + ": " + std::to_string(n_cols) + " columns for " + std::to_string(n_patients) + " patients (n_cases + n_ctrls)";
  else if (iterations > 0 && !have_masks) {
    msg = "assertion: " + who + " needs the permutation masks (iterations > 0, none set)";
    return GCRE_ERR_ASSERT;
  } else {
    planes.assign((size_t)n_rows, 0);
    int32_t most = 0;
    for (int64_t g = 0; g < n_rows; g++) {
      const int32_t* w = weights + (size_t)g * (size_t)n_cols;
      int32_t top = 0;
      for (int32_t q = 0; q < n_cols; q++) {
        if (w[q] < 0) {
          msg = who + ": weights[" + std::to_string(g) + "][" + std::to_string(q) + "] = " + std::to_string(w[q]) + " is negative";
          planes.clear();
          return GCRE_ERR_ARG;
        }
        top = std::max(top, w[q]);
      }
      planes[(size_t)g] = burden_bit_length(top);
      most = std::max(most, planes[(size_t)g]);
    }
    const double row_bytes = (double)most * (double)W32p * 4.0 + (double)Kpad * 8.0;
    if (iterations > 0 && most > 0 && row_bytes > max_mb * 1048576.0) {
      msg = who + ": one row of " + std::to_string(most) + " planes and " + std::to_string(Kpad) + " sums takes " +
            std::to_string((int64_t)row_bytes) + " bytes: above GCRE_BURDEN_MAX_MB = " + std::to_string(max_mb);
      planes.clear();
      return GCRE_ERR_ARG;
    }
    return GCRE_OK;
  }
  return GCRE_ERR_ARG;
}

// The case / control masks of the n patients (cases are the first n_cases columns), and one set's union rows: P = the OR of
// its (+) members, N = P + neg_off the OR of its (-) members (`split` off: everything into P, N is not touched), within the
// n patients -- with k = cases_pos, ctrls_pos, cases_neg, ctrls_neg (NULL: not counted).  `P` (and N) hold W zeroed words at
// the least; no member is NA.
struct SetUnion {
  int W;
  std::vector<uint64_t> cases, ctrls;
  SetUnion(int words, int n, int n_cases) : W(words), cases((size_t)words, 0), ctrls((size_t)words, 0) {
    for (int q = 0; q < n; q++) (q < n_cases ? cases : ctrls)[(size_t)q / 64] |= uint64_t(1) << (q % 64);
  }
  int count_and(const uint64_t* a, const std::vector<uint64_t>& m) const {
    int n = 0;
    for (int w = 0; w < W; w++) n += __builtin_popcountll(a[w] & m[w]);
    return n;
  }
  void build(const gcre_set_input* in, int64_t s, uint64_t* P, size_t neg_off, bool split, int32_t k[4]) const {
    uint64_t* N = split ? P + neg_off : P;
    for (int64_t i = in->set_off[s]; i < in->set_off[s + 1]; i++) {
      const uint64_t* r = in->rows + (size_t)in->members[i] * W;
      uint64_t* d = (split && in->signs && in->signs[i] == -1) ? N : P;
      for (int w = 0; w < W; w++) d[w] |= r[w] & (cases[w] | ctrls[w]);
    }
    if (!k) return;   // the rows only
    k[0] = count_and(P, cases);
    k[1] = count_and(P, ctrls);
    k[2] = k[3] = 0;
    if (split) {
      k[2] = count_and(N, ctrls);   // the (-) half counts the other way round (methods.h:183-184)
      k[3] = count_and(N, cases);
    }
  }
};

}  // namespace gcre_host

// gcre_strata.h -- the host plan of the stratified set scores (gcre_score_sets_strata), defined once: the
// cases and the patients of every stratum, what the entry refuses of its own arguments, where every stratum's diagonal-major
// table lies in the one device array, and the slabs of whole sets.  Plain C++17 over include/gcre_hip.h, no HIP: the host
// stage (gcre_host_strata.hip) includes it under hipcc and tests/native/strata_main.cpp under plain g++.
#pragma once
#include "../../include/gcre_hip.h"
#include "gcre_env.h"
#include "gcre_sequential.h"   // strata_counts: the strata as gcre_generate_perm_masks reads them

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

namespace gcre_strata __attribute__((visibility("hidden"))) {

constexpr int kStrataMax = GCRE_STRATA_MAX;
constexpr int kStrataTile = 512;   // permutations per tile of k_strata_null
static_assert(kStrataMax == 16, "the limit the header promises, and the four waves x four rows of the check launch");

// GCRE_STRATA_MAX_MB: the bound on the stratum rows (and the null_scores rows, when asked) a slab holds on the device, read
// per call (tests set fractions); default 1024.  GCRE_STRATA_SLAB_SETS (tests) bounds the sets of a slab further; 0 = no bound.
inline double strata_max_mb() { return gcre_env::env_mb("GCRE_STRATA_MAX_MB", 1024, 1048576.0); }
inline int64_t strata_slab_sets_env() { return gcre_env::env_count("GCRE_STRATA_SLAB_SETS"); }

// What the entry is told beside the set list; pointers only as "given or not" where they are not read here
struct StrataAsk {
  int32_t n, n_cases;                   // the context's cohort
  int32_t iterations, Kpad;             // its permutations, and their padded count
  const int32_t* stratum;               // [n] or NULL
  int32_t n_strata;
  bool have_tables;
  const int32_t* nrow;                  // [n_strata] or NULL
  const int32_t* ncol;                  // [n_strata] or NULL
  const int64_t* tab_off;               // [n_strata] or NULL
  bool have_px;
  bool want_null, want_family;
};

// What gcre_score_sets_strata refuses of its own arguments, after the checks of the set list (gcre_setlists.h) passed; on
// GCRE_OK cases_in / size_of [n_strata] hold every stratum's cases (columns < n_cases) and patients.  An optional matrix
// [n_sets][iterations] is read back a slab of sets at a time, but one 512-permutation tile of it over all sets must fit
// `max_mb`: a list too long for that is split by the caller.
inline int check_strata_args(const gcre_set_input* in, const StrataAsk& q, double max_mb, const std::string& who,
                             std::vector<uint32_t>& cases_in, std::vector<uint32_t>& size_of, std::string& msg) {
  if (!q.have_px) { msg = who + ": NULL argument (px_out)"; return GCRE_ERR_ARG; }
  if (!q.stratum) { msg = who + ": NULL argument (stratum)"; return GCRE_ERR_ARG; }
  if (q.n_strata < 1 || q.n_strata > kStrataMax) {
    msg = who + ": n_strata = " + std::to_string(q.n_strata) + " outside 1 .. GCRE_STRATA_MAX = " + std::to_string(kStrataMax);
    return GCRE_ERR_ARG;
  }
  if (!q.have_tables || !q.nrow || !q.ncol || !q.tab_off) {
    msg = who + ": NULL argument (tables, nrow, ncol or tab_off)";
    return GCRE_ERR_ARG;
  }
  for (int s = 0; s < q.n_strata; s++)
    if (q.nrow[s] < 1 || q.ncol[s] < 1 || q.tab_off[s] < 0) {
      msg = who + ": the table of stratum " + std::to_string(s) + " must have at least one row and one column, not " +
            std::to_string(q.nrow[s]) + " x " + std::to_string(q.ncol[s]) + " at offset " + std::to_string(q.tab_off[s]);
      return GCRE_ERR_ARG;
    }
  if (in->n_sets > 0x7fffffff / kStrataMax) { msg = who + ": too many sets"; return GCRE_ERR_ARG; }
  if (int rc = gcre_sequential::strata_counts(q.n, q.n_cases, q.stratum, q.n_strata, cases_in, size_of, who, msg)) return rc;
  const double tile = (double)in->n_sets * 8.0 * (double)kStrataTile;
  if (q.want_null && q.iterations > 0 && tile > max_mb * 1048576.0) {
    msg = who + ": one tile of " + std::to_string(kStrataTile) + " permutations of null_scores takes " + std::to_string((int64_t)tile) +
          " bytes: above GCRE_STRATA_MAX_MB = " + std::to_string(max_mb);
    return GCRE_ERR_ARG;
  }
  return GCRE_OK;
}

// The message of the one refusal that comes after launches: `bad` (stratum, permutation) pairs of the resident masks do not
// hold the stratum's cases
inline std::string strata_mask_message(const std::string& who, long long bad) {
  return who + ": " + std::to_string(bad) + " (stratum, permutation) pairs of the context's masks do not keep the cases of the stratum: " +
         "the masks must come from generate_permutations(seed, strata) with these strata";
}

// Where stratum s's diagonal-major table starts in the one device array, in doubles: table s has size_of[s] + 1 diagonals
// (k_table_to_diag with n = size_of[s]), (n + 1)(n + 2) / 2 cells.  diag_off [n_strata + 1]; the last entry is the total.
inline void strata_diag_offsets(const std::vector<uint32_t>& size_of, std::vector<int64_t>& diag_off) {
  diag_off.assign(size_of.size() + 1, 0);
  for (size_t s = 0; s < size_of.size(); s++) {
    const int64_t td = (int64_t)size_of[s] + 1;
    diag_off[s + 1] = diag_off[s] + td * (td + 1) / 2;
  }
}

// the working rows of one set on the device: its stratum rows [n_strata][M][W32p] dwords, and with null_scores one row of
// Kpad doubles
inline double strata_set_bytes(int n_strata, int method, int32_t W32p, int32_t Kpad, bool want_null) {
  return (double)n_strata * (double)method * (double)W32p * 4.0 + (want_null ? (double)Kpad * 8.0 : 0.0);
}

// Valid sets per slab: as many as stay under `max_mb` (one at the least), never more than `slab_sets` (0: no such bound), than
// the rows a 32-bit row index holds, or than there are
inline int64_t strata_slab_sets(int64_t n_valid, int n_strata, int method, int32_t W32p, int32_t Kpad, bool want_null, double max_mb,
                                int64_t slab_sets) {
  const double fit = max_mb * 1048576.0 / strata_set_bytes(n_strata, method, W32p, Kpad, want_null);
  int64_t per = fit >= 2147483647.0 ? 0x7fffffff : std::max<int64_t>((int64_t)fit, 1);
  per = std::min<int64_t>(per, 0x7fffffff / std::max(n_strata, 1));
  if (slab_sets > 0) per = std::min(per, slab_sets);
  return std::max<int64_t>(std::min(per, n_valid), 1);
}

}  // namespace gcre_strata

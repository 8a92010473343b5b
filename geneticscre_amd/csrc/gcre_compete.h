// gcre_compete.h -- the draw rule of the competitive set tests (gcre_score_sets_compete), defined once: the
// pool table, what the entry refuses of its own arguments, the pick of one member and the loop over a draw.  Plain C++17
// over include/gcre_hip.h: k_compete_null (gcre_compete.hip) includes it under hipcc, where the draw functions are
// __host__ __device__, and tests/native/compete_main.cpp under plain g++.  report.competitive_picks restates it in Python.
#pragma once
#include "../../include/gcre_hip.h"
#include "gcre_env.h"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define GCRE_COMPETE_HD __host__ __device__
#else
#define GCRE_COMPETE_HD
#endif

namespace gcre_compete __attribute__((visibility("hidden"))) {

constexpr int kCompeteAttempts = 64;                       // attempts of a member before the fallback: the stride of j in the stream
constexpr int kCompeteMaxMembers = GCRE_COMPETE_MAX_MEMBERS;
static_assert(kCompeteMaxMembers >= 1024, "the limit the header promises");

// gcre_mix64, dp_split_key and dp_perm_base of gcre_kernels.h, restated so that a program without HIP has them
// (tests/test_compete_host.py holds them against the library's gcre_mix64)
GCRE_COMPETE_HD inline uint64_t compete_mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// base of draw b of set s: dp_perm_base(dp_split_key(seed, s), b)
GCRE_COMPETE_HD inline uint64_t compete_base(uint64_t seed, int64_t s, int64_t b) {
  const uint64_t key = compete_mix64(seed ^ (0xd1b54a32d192ed03ull * (uint64_t)(s + 1)));
  return compete_mix64(key ^ (0x51ed270b7f3c9a1dull * (uint64_t)(b + 1)));
}
// floor(u * n / 2^64) by the 128-bit product (k_generate_masks' idiom)
GCRE_COMPETE_HD inline uint32_t compete_index(uint64_t u, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__umul64hi(u, (uint64_t)n);
#else
  return (uint32_t)(((unsigned __int128)u * n) >> 64);
#endif
}

// The pick of member j of a draw whose stream starts at `base`: attempt t reads compete_mix64(base + 64 j + t) and takes pool
// entry floor(u * N / 2^64); the first candidate that taken(row) does not hold is the pick; after `attempts` (1 .. 64) failed
// ones the lowest pool entry not taken.  `pool` [N] are the rows of the member's bin, ascending.  With at most N / 2 rows
// taken the fallback always finds one.  On the device every argument is wave-uniform, taken() may be a wave-wide vote and
// `pool` a pointer into the constant address space.
template <typename Pool, typename Taken>
GCRE_COMPETE_HD inline int32_t compete_pick(uint64_t base, int32_t j, Pool pool, int32_t N, int attempts, Taken&& taken) {
  const uint64_t at = base + (uint64_t)kCompeteAttempts * (uint64_t)j;
  for (int t = 0; t < attempts; t++) {
    const int32_t cand = pool[compete_index(compete_mix64(at + (uint64_t)t), (uint32_t)N)];
    if (!taken(cand)) return cand;
  }
  for (int32_t i = 0; i < N; i++)
    if (!taken(pool[i])) return pool[i];
  return -1;   // (not reached: 2k <= N)
}

// One member as a draw reads it: a fixed member (`off` < 0) stays row `n`; any other draws among pool rows [off, off + n)
struct CompeteMember { int32_t off, n; };

// Draw b of set s, in member order: picks[j] = the row member j receives.  `mem` [k] as above, `pool_rows` the pool table.
inline void compete_draw(uint64_t seed, int64_t s, int64_t b, const CompeteMember* mem, int32_t k, const int32_t* pool_rows,
                         int attempts, int32_t* picks) {
  const uint64_t base = compete_base(seed, s, b);
  for (int32_t j = 0; j < k; j++) {
    if (mem[j].off < 0) { picks[j] = mem[j].n; continue; }
    auto taken = [&](int32_t row) {
      for (int32_t i = 0; i < j; i++) if (picks[i] == row) return true;
      return false;
    };
    picks[j] = compete_pick(base, j, pool_rows + mem[j].off, mem[j].n, attempts, taken);
  }
}

// The pool table: the rows of every bin in ascending row order, bins ascending; bin beta = rows[off[beta] .. off[beta + 1]).
// `bin` NULL: every row in bin 0.  Values are checked before (check_compete_args).
inline void compete_pool(const int32_t* bin, int64_t n_rows, int32_t n_bins, std::vector<int32_t>& rows, std::vector<int32_t>& off) {
  off.assign((size_t)n_bins + 1, 0);
  for (int64_t r = 0; r < n_rows; r++) {
    const int32_t b = bin ? bin[r] : 0;
    if (b >= 0) off[(size_t)b + 1]++;
  }
  for (int32_t b = 0; b < n_bins; b++) off[(size_t)b + 1] += off[(size_t)b];
  rows.assign((size_t)off[(size_t)n_bins], 0);
  std::vector<int32_t> at(off.begin(), off.end() - 1);
  for (int64_t r = 0; r < n_rows; r++) {
    const int32_t b = bin ? bin[r] : 0;
    if (b >= 0) rows[(size_t)at[(size_t)b]++] = (int32_t)r;
  }
}

// every member of the list as a draw reads it (NA members: fixed on row -1, their sets are never drawn)
inline void compete_members(const gcre_set_input* in, const int32_t* bin, const std::vector<int32_t>& off, std::vector<CompeteMember>& mem) {
  const int64_t T = in->n_sets > 0 ? in->set_off[in->n_sets] : 0;
  mem.resize((size_t)T);
  for (int64_t i = 0; i < T; i++) {
    const int32_t row = in->members[i];
    const int32_t b = row < 0 ? -1 : (bin ? bin[row] : 0);
    mem[(size_t)i] = b < 0 ? CompeteMember{-1, row} : CompeteMember{off[(size_t)b], off[(size_t)b + 1] - off[(size_t)b]};
  }
}

// GCRE_COMPETE_ATTEMPTS (tests: 1 .. 64 forces the fallback), GCRE_COMPETE_MAX_MB (the optional outputs a slab of draws holds
// on the device; tests set fractions), GCRE_COMPETE_SLAB_DRAWS (tests): read per call
inline int compete_attempts() {
  int a = kCompeteAttempts;
  if (const char* e = std::getenv("GCRE_COMPETE_ATTEMPTS")) a = std::min(std::max(std::atoi(e), 1), kCompeteAttempts);
  return a;
}
inline double compete_max_mb() { return gcre_env::env_mb("GCRE_COMPETE_MAX_MB", 1024, 1048576.0); }

// What gcre_score_sets_compete refuses of its own arguments, after the checks of the set list (gcre_setlists.h) passed.
// The bytes one draw adds to the optional outputs -- 8 per set of null_scores, 4 per listed member of picks -- must fit
// `max_mb`: the draws are walked in slabs of whole draws.
inline int check_compete_args(const gcre_set_input* in, const int32_t* bin, int32_t n_bins, int64_t draws, bool have_n_ge,
                              bool want_null, bool want_picks, double max_mb, const std::string& who, std::string& msg) {
  const int64_t S = in->n_sets;
  if (!have_n_ge) { msg = who + ": NULL argument (n_ge)"; return GCRE_ERR_ARG; }
  if (draws < 0) { msg = who + ": draws must not be negative, not " + std::to_string(draws); return GCRE_ERR_ARG; }
  if (n_bins < 1) { msg = who + ": n_bins must be at least 1, not " + std::to_string(n_bins); return GCRE_ERR_ARG; }
  if (in->n_rows > 0x7fffffff) { msg = who + ": too many rows"; return GCRE_ERR_ARG; }
  for (int64_t r = 0; bin && r < in->n_rows; r++)
    if (bin[r] < -1 || bin[r] >= n_bins) {
      msg = who + ": bin[" + std::to_string(r) + "] = " + std::to_string(bin[r]) + " out of range (" + std::to_string(n_bins) +
            " bins, -1 = never drawn)";
      return GCRE_ERR_ARG;
    }
  std::vector<int32_t> size((size_t)n_bins, 0), need((size_t)n_bins, 0), touched;
  for (int64_t r = 0; r < in->n_rows; r++) {
    const int32_t b = bin ? bin[r] : 0;
    if (b >= 0) size[(size_t)b]++;
  }
  for (int64_t s = 0; s < S; s++) {
    const int64_t k = in->set_off[s + 1] - in->set_off[s];
    if (k > kCompeteMaxMembers) {
      msg = who + ": set " + std::to_string(s) + " has " + std::to_string(k) + " members, more than GCRE_COMPETE_MAX_MEMBERS = " +
            std::to_string(kCompeteMaxMembers);
      return GCRE_ERR_ARG;
    }
    bool valid = true;
    for (int64_t i = in->set_off[s]; i < in->set_off[s + 1]; i++) valid = valid && in->members[i] >= 0;
    if (!valid) continue;   // never drawn
    touched.clear();
    for (int64_t i = in->set_off[s]; i < in->set_off[s + 1]; i++) {
      const int32_t b = bin ? bin[in->members[i]] : 0;
      if (b < 0) continue;
      if (need[(size_t)b]++ == 0) touched.push_back(b);
    }
    int32_t bad = -1;
    for (int32_t b : touched) {
      if (2 * (int64_t)need[(size_t)b] > (int64_t)size[(size_t)b] && (bad < 0 || b < bad)) bad = b;
    }
    if (bad >= 0) {
      msg = who + ": set " + std::to_string(s) + " draws " + std::to_string(need[(size_t)bad]) + " members from bin " +
            std::to_string(bad) + " of " + std::to_string(size[(size_t)bad]) + " rows: a bin must hold twice as many rows as a set draws from it";
      return GCRE_ERR_ARG;
    }
    for (int32_t b : touched) need[(size_t)b] = 0;
  }
  const double per_draw = (want_null ? (double)S * 8.0 : 0.0) + (want_picks && S > 0 ? (double)in->set_off[S] * 4.0 : 0.0);
  if (draws > 0 && per_draw > max_mb * 1048576.0) {
    msg = who + ": the optional outputs of one draw take " + std::to_string((int64_t)per_draw) + " bytes: above GCRE_COMPETE_MAX_MB = " +
          std::to_string(max_mb);
    return GCRE_ERR_ARG;
  }
  return GCRE_OK;
}

// draws per slab: all of them, or what keeps the optional outputs of a slab under `max_mb` (one draw at the least; the check
// above has passed), and GCRE_COMPETE_SLAB_DRAWS below that
inline int64_t compete_slab_draws(int64_t draws, double per_draw_bytes, double max_mb) {
  int64_t slab = std::max<int64_t>(draws, 1);
  if (per_draw_bytes > 0) slab = std::min<int64_t>(slab, std::max<int64_t>((int64_t)(max_mb * 1048576.0 / per_draw_bytes), 1));
  if (const char* e = std::getenv("GCRE_COMPETE_SLAB_DRAWS")) slab = std::min<int64_t>(slab, std::max<int64_t>(std::atoll(e), 1));
  return slab;
}

}  // namespace gcre_compete

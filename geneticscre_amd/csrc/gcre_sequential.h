// gcre_sequential.h -- the rule of the sequential permutation p-values (gcre_score_sets_sequential), defined
// once: the mask step per patient with caller strata (k_generate_masks' rule, gcre_frontend.hip, for a 64-bit permutation
// index), where in a batch's bit row the stopping exceedance lies, what the entry refuses of its own arguments and the batch
// schedule.  Plain C++17 over include/gcre_hip.h: the kernels of gcre_sequential.hip include it under hipcc, where the mask
// and bit functions are __host__ __device__, and tests/native/sequential_main.cpp under plain g++.
// report.permutation_masks and report.sequential_reference restate it in Python.
#pragma once
#include "../../include/gcre_hip.h"
#include "gcre_env.h"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define GCRE_SEQ_HD __host__ __device__
#else
#define GCRE_SEQ_HD
#endif

namespace gcre_sequential __attribute__((visibility("hidden"))) {

constexpr int kSeqTile = 512;                              // permutations per tile of k_seq_null: a batch is whole tiles
constexpr int64_t kSeqMaxHits = 0x7fffffff;                // h: 1 .. 2^31 - 1
constexpr int64_t kSeqMaxPerms = (int64_t)1 << 40;         // max_perms: 0 .. 2^40
constexpr int64_t kSeqFirstBatch = 8 * kSeqTile;           // the first batch: 4,096 permutations
constexpr int64_t kSeqGrowth = 4;                          // every later batch: four times the one before, up to the bound
constexpr int64_t kSeqBatchLimit = (int64_t)1 << 30;       // the 32-bit column index of a batch

// gcre_mix64 of gcre_kernels.h, restated so that a program without HIP has it (tests/test_sequential_host.py holds it against
// the library's gcre_mix64)
GCRE_SEQ_HD inline uint64_t seq_mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// base of permutation r: k_generate_masks' own, no tag in between -- for r below a context's iterations the masks are the
// context's
GCRE_SEQ_HD inline uint64_t seq_base(uint64_t seed, uint64_t r) { return seq_mix64(seed ^ (0x51ed270b7f3c9a1dull * (r + 1))); }
// floor(u * n / 2^64) by the 128-bit product (k_generate_masks' idiom)
GCRE_SEQ_HD inline uint32_t seq_index(uint64_t u, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__umul64hi(u, (uint64_t)n);
#else
  return (uint32_t)(((unsigned __int128)u * n) >> 64);
#endif
}
// The step of patient c in permutation `base` (Knuth's selection sampling, Algorithm S): `rem` patients of its stratum are
// left, this one included, and `need` of them are still to become cases.  Returns whether c is a case; both counts move on.
GCRE_SEQ_HD inline bool seq_step(uint64_t base, uint32_t c, uint32_t& rem, uint32_t& need) {
  const uint64_t u = seq_mix64(base + (uint64_t)c);
  const bool take = seq_index(u, rem) < need;
  need -= take ? 1u : 0u;
  rem--;
  return take;
}

// The strata as gcre_generate_perm_masks reads and refuses them: the cases are the columns < n_cases; cases_in / size_of
// [n_strata] (one stratum without `stratum`).  `n_strata` is what the caller passed.
inline int strata_counts(int32_t n, int32_t n_cases, const int32_t* stratum, int n_strata, std::vector<uint32_t>& cases_in,
                         std::vector<uint32_t>& size_of, const std::string& who, std::string& msg) {
  if (stratum && n_strata < 1) {
    msg = who + ": bad strata";
    return GCRE_ERR_ARG;
  }
  const int ns = stratum ? n_strata : 1;
  cases_in.assign((size_t)ns, 0u);
  size_of.assign((size_t)ns, 0u);
  for (int32_t q = 0; q < n; q++) {
    const int s = stratum ? stratum[q] : 0;
    if (s < 0 || s >= ns) {
      msg = who + ": stratum id out of range";
      return GCRE_ERR_RANGE;
    }
    size_of[(size_t)s]++;
    if (q < n_cases) cases_in[(size_t)s]++;
  }
  return GCRE_OK;
}

// Permutation r as packed dwords: bit c & 31 of words[c >> 5] is patient c; `words` holds ceil(n / 32) dwords.  Inside every
// stratum exactly cases_in[s] bits.
inline void sequential_mask(uint64_t seed, uint64_t r, int32_t n, const int32_t* stratum, const std::vector<uint32_t>& cases_in,
                            const std::vector<uint32_t>& size_of, uint32_t* words) {
  const uint64_t base = seq_base(seed, r);
  for (int32_t k = 0; k < (n + 31) / 32; k++) words[k] = 0;
  std::vector<uint32_t> need(cases_in), rem(size_of);
  for (int32_t c = 0; c < n; c++) {
    const size_t s = stratum ? (size_t)stratum[c] : 0;
    if (seq_step(base, (uint32_t)c, rem[s], need[s])) words[c >> 5] |= 1u << (c & 31);
  }
}

GCRE_SEQ_HD inline int seq_popcount64(uint64_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(w);
#else
  return __builtin_popcountll(w);
#endif
}
// the position of the k-th set bit of w (k = 0: the lowest); w has more than k bits set
GCRE_SEQ_HD inline int seq_select64(uint64_t w, int k) {
  int at = 0;
  for (int width = 32; width >= 1; width >>= 1) {   // binary search on the popcount of the low part
    const uint64_t low = w & ((1ull << width) - 1ull);
    const int c = seq_popcount64(low);
    if (k >= c) {
      k -= c;
      w >>= width;
      at += width;
    } else {
      w = low;
    }
  }
  return at;
}

// A batch's bit row: bit i & 63 of bits[i >> 6] says whether permutation r0 + i reached the score, i < n_bits (the bits at and
// beyond n_bits are zero).  `prior` exceedances came before the batch, prior < h.  Returns the index i of the one that is the
// h-th over all, or -1 when the batch does not hold it.
inline int64_t sequential_find(const uint64_t* bits, int64_t n_bits, int64_t prior, int64_t h) {
  int64_t need = h - prior;   // >= 1
  for (int64_t w = 0; w < (n_bits + 63) / 64; w++) {
    const int c = seq_popcount64(bits[w]);
    if (need <= c) return w * 64 + seq_select64(bits[w], (int)(need - 1));
    need -= c;
  }
  return -1;
}

// GCRE_SEQ_MAX_MB (the masks and the bit rows of one batch on the device; tests set fractions) and GCRE_SEQ_BATCH_PERMS
// (tests; 0 = unset): read per call
inline double seq_max_mb() { return gcre_env::env_mb("GCRE_SEQ_MAX_MB", 1024, 1048576.0); }
inline int64_t seq_batch_perms_env() {
  const char* e = std::getenv("GCRE_SEQ_BATCH_PERMS");
  return e ? std::max<int64_t>(std::atoll(e), 0) : 0;
}

// What gcre_score_sets_sequential refuses of its own arguments, after the checks of the set list (gcre_setlists.h) passed;
// the strata are strata_counts' business.
inline int check_sequential_args(int64_t h, int64_t max_perms, bool have_seq_out, const std::string& who, std::string& msg) {
  if (!have_seq_out)
    msg = who + ": NULL argument (seq_out)";
  else if (h < 1 || h > kSeqMaxHits)
    msg = who + ": hits = " + std::to_string(h) + " outside 1 .. " + std::to_string(kSeqMaxHits);
  else if (max_perms < 0 || max_perms > kSeqMaxPerms)
    msg = who + ": max_perms = " + std::to_string(max_perms) + " outside 0 .. " + std::to_string(kSeqMaxPerms);
  else
    return GCRE_OK;
  return GCRE_ERR_ARG;
}

// The permutations of the batch behind one of `prev` (0: the first batch), whole tiles: the first batch small, every later one
// kSeqGrowth times the one before, never above the tiles whose masks (W32p dwords a permutation) and bit rows (one bit per
// active set and permutation) stay under `max_mb` -- one tile at the least -- nor above `cap_perms` rounded down to whole tiles
// (0: no such cap; one tile at the least).  Always a positive multiple of the tile: the caller's r0 moves on every turn.
inline int64_t sequential_batch(int64_t prev, int32_t W32p, int64_t n_active, double max_mb, int64_t cap_perms) {
  const int64_t T = kSeqTile;
  int64_t want = prev <= 0 ? kSeqFirstBatch : (prev >= kSeqBatchLimit / kSeqGrowth ? kSeqBatchLimit : prev * kSeqGrowth);
  const double tile_bytes = (double)T * ((double)W32p * 4.0 + (double)n_active / 8.0);
  const double fit = max_mb * 1048576.0 / tile_bytes;
  const int64_t tiles_fit = fit >= (double)(kSeqBatchLimit / T) ? kSeqBatchLimit / T : std::max<int64_t>((int64_t)fit, 1);
  want = std::min(want, tiles_fit * T);
  // the dword index of a batch's masks stays below 2^30 (k_seq_null's 32-bit byte offsets)
  want = std::min(want, std::max<int64_t>(kSeqBatchLimit / std::max<int64_t>(W32p, 1) / T, 1) * T);
  if (cap_perms > 0) want = std::min(want, std::max<int64_t>(cap_perms / T, 1) * T);
  return std::max<int64_t>(want / T, 1) * T;
}

}  // namespace gcre_sequential

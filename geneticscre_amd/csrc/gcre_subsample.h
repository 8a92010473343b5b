// gcre_subsample.h -- the draw rule of the split-half stability counts (gcre_score_sets_subsample), defined
// once: the seed derivation, the per-patient step of the selection sampling, what the entry refuses of its own arguments and
// the slab sizing.  Plain C++17 over include/gcre_hip.h: k_subsample_masks (gcre_subsample.hip) includes it under hipcc, where
// the draw functions are __host__ __device__, and tests/native/subsample_main.cpp under plain g++.  report.subsample_masks
// restates it in Python.
#pragma once
#include "../../include/gcre_hip.h"
#include "gcre_env.h"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define GCRE_SUBSAMPLE_HD __host__ __device__
#else
#define GCRE_SUBSAMPLE_HD
#endif

namespace gcre_subsample __attribute__((visibility("hidden"))) {

constexpr int kSubsampleTile = 512;                        // draws per tile of k_subsample_null: a slab is whole tiles
constexpr int kSubsampleMaxCuts = GCRE_SUBSAMPLE_MAX_CUTS;
static_assert(kSubsampleMaxCuts == 8, "the limit the header promises");

// gcre_mix64 of gcre_kernels.h, restated so that a program without HIP has it (tests/test_subsample_host.py holds it against
// the library's gcre_mix64)
GCRE_SUBSAMPLE_HD inline uint64_t subsample_mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// seed' of the entry: the caller's seed under the entry's own tag ("subsampl"), so that the draws share nothing with the
// permutation masks gcre_generate_perm_masks makes from the same seed
GCRE_SUBSAMPLE_HD inline uint64_t subsample_seed(uint64_t seed) { return subsample_mix64(seed ^ 0x73756273616d706cull); }
// base of draw b: k_generate_masks' base of permutation b under seed'
GCRE_SUBSAMPLE_HD inline uint64_t subsample_base(uint64_t seed1, int64_t b) {
  return subsample_mix64(seed1 ^ (0x51ed270b7f3c9a1dull * (uint64_t)(b + 1)));
}
// floor(u * n / 2^64) by the 128-bit product (k_generate_masks' idiom)
GCRE_SUBSAMPLE_HD inline uint32_t subsample_index(uint64_t u, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__umul64hi(u, (uint64_t)n);
#else
  return (uint32_t)(((unsigned __int128)u * n) >> 64);
#endif
}
// The step of patient c in draw `base` (Knuth's selection sampling, Algorithm S): `rem` patients of its stratum are left,
// this one included, and `need` of them are still to be taken.  Returns whether c is taken; both counts move on.
GCRE_SUBSAMPLE_HD inline bool subsample_step(uint64_t base, uint32_t c, uint32_t& rem, uint32_t& need) {
  const uint64_t u = subsample_mix64(base + (uint64_t)c);
  const bool take = subsample_index(u, rem) < need;
  need -= take ? 1u : 0u;
  rem--;
  return take;
}

// Draw b as packed dwords: bit c & 31 of words[c >> 5] is patient c; `words` holds ceil(n / 32) dwords.  Exactly m_cases bits
// among the columns < n_cases and m_ctrls among the rest.
inline void subsample_draw(uint64_t seed, int64_t b, int32_t n_cases, int32_t n_ctrls, int32_t m_cases, int32_t m_ctrls, uint32_t* words) {
  const uint64_t base = subsample_base(subsample_seed(seed), b);
  const int32_t n = n_cases + n_ctrls;
  for (int32_t k = 0; k < (n + 31) / 32; k++) words[k] = 0;
  uint32_t rem = (uint32_t)n_cases, need = (uint32_t)m_cases;
  for (int32_t c = 0; c < n; c++) {
    if (c == n_cases) { rem = (uint32_t)n_ctrls; need = (uint32_t)m_ctrls; }
    if (subsample_step(base, (uint32_t)c, rem, need)) words[c >> 5] |= 1u << (c & 31);
  }
}

// GCRE_SUBSAMPLE_MAX_MB (the masks and the optional outputs a slab of draws holds on the device; tests set fractions) and
// GCRE_SUBSAMPLE_SLAB_DRAWS (tests): read per call
inline double subsample_max_mb() { return gcre_env::env_mb("GCRE_SUBSAMPLE_MAX_MB", 1024, 1048576.0); }

// What the entry is told beside the set list; pointers only as "given or not"
struct SubsampleAsk {
  int32_t n_cases, n_ctrls;             // the context's cohort
  int32_t m_cases, m_ctrls;
  int64_t draws;
  bool have_table_a;
  int nrow_a, ncol_a;
  bool have_table_b;
  int nrow_b, ncol_b;
  const double* cut;                    // [n_sets][n_cut] or NULL
  int32_t n_cut;
  bool have_n_a, have_n_b, have_n_both;
  bool want_scores_a, want_scores_b;
};

// the bytes one draw adds to the optional outputs: 8 per set and matrix
inline double subsample_draw_bytes(const gcre_set_input* in, const SubsampleAsk& q) {
  return (double)in->n_sets * 8.0 * (double)((q.want_scores_a ? 1 : 0) + (q.want_scores_b ? 1 : 0));
}

// What gcre_score_sets_subsample refuses of its own arguments, after the checks of the set list (gcre_setlists.h) passed.
// The optional outputs of one tile of draws must fit `max_mb`: the draws are walked in slabs of whole tiles.
inline int check_subsample_args(const gcre_set_input* in, const SubsampleAsk& q, double max_mb, const std::string& who, std::string& msg) {
  if (q.draws < 0)
    msg = who + ": draws must not be negative, not " + std::to_string(q.draws);
  else if (q.m_cases < 0 || q.m_cases > q.n_cases)
    msg = who + ": m_cases = " + std::to_string(q.m_cases) + " outside 0 .. n_cases = " + std::to_string(q.n_cases);
  else if (q.m_ctrls < 0 || q.m_ctrls > q.n_ctrls)
    msg = who + ": m_ctrls = " + std::to_string(q.m_ctrls) + " outside 0 .. n_ctrls = " + std::to_string(q.n_ctrls);
  else if (!q.have_table_a)
    msg = who + ": NULL argument (table_a)";
  else if (q.nrow_a < 1 || q.ncol_a < 1)
    msg = who + ": table_a must have at least one row and one column, not " + std::to_string(q.nrow_a) + " x " + std::to_string(q.ncol_a);
  else if (q.have_table_b && (q.nrow_b < 1 || q.ncol_b < 1))
    msg = who + ": table_b must have at least one row and one column, not " + std::to_string(q.nrow_b) + " x " + std::to_string(q.ncol_b);
  else if (q.n_cut < 0 || q.n_cut > kSubsampleMaxCuts)
    msg = who + ": n_cut = " + std::to_string(q.n_cut) + " outside 0 .. GCRE_SUBSAMPLE_MAX_CUTS = " + std::to_string(kSubsampleMaxCuts);
  else if (q.n_cut > 0 && !q.cut)
    msg = who + ": NULL argument (cut) with n_cut = " + std::to_string(q.n_cut);
  else if (q.n_cut > 0 && !q.have_n_a)
    msg = who + ": NULL argument (n_a) with n_cut = " + std::to_string(q.n_cut);
  else if (!q.have_table_b && (q.have_n_b || q.have_n_both || q.want_scores_b))
    msg = who + ": " + std::string(q.have_n_b ? "n_b" : q.have_n_both ? "n_both" : "scores_b") + " without table_b: half B is not scored";
  else {
    for (int64_t i = 0; q.n_cut > 0 && i < in->n_sets * (int64_t)q.n_cut; i++)
      if (q.cut[i] != q.cut[i]) {
        msg = who + ": cut[" + std::to_string(i / q.n_cut) + "][" + std::to_string(i % q.n_cut) + "] is NaN";
        return GCRE_ERR_ARG;
      }
    const double tile = subsample_draw_bytes(in, q) * (double)kSubsampleTile;
    if (q.draws > 0 && tile > max_mb * 1048576.0) {
      msg = who + ": the optional outputs of one tile of " + std::to_string(kSubsampleTile) + " draws take " + std::to_string((int64_t)tile) +
            " bytes: above GCRE_SUBSAMPLE_MAX_MB = " + std::to_string(max_mb);
      return GCRE_ERR_ARG;
    }
    return GCRE_OK;
  }
  return GCRE_ERR_ARG;
}

// draws per slab, a multiple of the tile: all of them, or the tiles whose masks (W32p dwords a draw) and optional outputs stay
// under `max_mb` (one tile at the least; the check above has passed), and GCRE_SUBSAMPLE_SLAB_DRAWS, rounded down to whole
// tiles, below that
inline int64_t subsample_slab_draws(int64_t draws, int32_t W32p, double per_draw_opt_bytes, double max_mb) {
  const int64_t T = kSubsampleTile;
  int64_t tiles = std::max<int64_t>((draws + T - 1) / T, 1);
  const double tile_bytes = (double)T * ((double)W32p * 4.0 + per_draw_opt_bytes);
  tiles = std::min<int64_t>(tiles, std::max<int64_t>((int64_t)(max_mb * 1048576.0 / tile_bytes), 1));
  if (const char* e = std::getenv("GCRE_SUBSAMPLE_SLAB_DRAWS")) tiles = std::min<int64_t>(tiles, std::max<int64_t>(std::atoll(e) / T, 1));
  return tiles * T;
}

}  // namespace gcre_subsample

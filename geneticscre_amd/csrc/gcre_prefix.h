// gcre_prefix.h -- the host plan of the variable-threshold set tests (gcre_score_sets_prefix), defined once:
// the expansion of the cut flags into steps, what the entry refuses of its own arguments, the slabs of whole sets, the
// size-sorted order of a slab's sets and the block table k_prefix_null reads.  Plain C++17 over include/gcre_hip.h, no HIP:
// the host stage (gcre_host_steps.hip, through gcre_steps.h) includes it under hipcc and tests/native/prefix_main.cpp under plain g++.
// tests/test_prefix_host.py restates it in Python.
#pragma once
#include "../../include/gcre_hip.h"
#include "gcre_env.h"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

namespace gcre_prefix __attribute__((visibility("hidden"))) {

constexpr int kPrefixBlockSets = 4;   // sets per block of k_prefix_null: one per wave

// The steps of every set of the list.  Member i of the flat member list ends a step if cut[i] != 0 (cut NULL: every member
// does); the last member of a set always ends one.  Step k of set s = its members up to and including the k-th cut member.
struct PrefixSteps {
  std::vector<int64_t> off;      // [n_sets + 1] steps of set s = [off[s], off[s + 1])
  std::vector<int64_t> end;      // [steps] the index in the flat member list of the member that ends the step
  std::vector<int32_t> members;  // [steps] members of the prefix: end - set_off[s] + 1
};
inline void prefix_steps(const gcre_set_input* in, const uint8_t* cut, PrefixSteps& st) {
  const int64_t S = in->n_sets;
  st.off.assign((size_t)S + 1, 0);
  st.end.clear();
  st.members.clear();
  for (int64_t s = 0; s < S; s++) {
    const int64_t b = in->set_off[s], e = in->set_off[s + 1];
    for (int64_t i = b; i < e; i++)
      if (!cut || cut[i] != 0 || i + 1 == e) {
        st.end.push_back(i);
        st.members.push_back((int32_t)(i - b + 1));
      }
    st.off[(size_t)s + 1] = (int64_t)st.end.size();
  }
}

// GCRE_PREFIX_MAX_MB: the bound on the step rows (and the null_max rows, when asked) a slab holds on the device, read per call
// (tests set fractions); default 1024.  GCRE_PREFIX_SLAB_SETS (tests) bounds the sets of a slab further; 0 = no bound.
inline double prefix_max_mb() { return gcre_env::env_mb("GCRE_PREFIX_MAX_MB", 1024, 1048576.0); }
inline int64_t prefix_slab_sets() { return gcre_env::env_count("GCRE_PREFIX_SLAB_SETS"); }

// the working rows of one set on the device: its step rows [steps][M][W32p] dwords, and with null_max one row of Kpad floats
inline double prefix_set_bytes(int64_t steps, int method, int32_t W32p, int32_t Kpad, bool want_null) {
  return (double)steps * (double)method * (double)W32p * 4.0 + (want_null ? (double)Kpad * 4.0 : 0.0);
}

// no member of set s is NA (set_is_valid of gcre_setlists.h, restated so that this header stands alone)
inline bool prefix_set_valid(const gcre_set_input* in, int64_t s) {
  bool valid = true;
  for (int64_t i = in->set_off[s]; i < in->set_off[s + 1]; i++) valid = valid && in->members[i] >= 0;
  return valid;
}

// What gcre_score_sets_prefix refuses of its own arguments, after the checks of the set list (gcre_setlists.h) passed.  With
// permutations (iterations > 0) the working rows of every valid set must fit `max_mb`: the sets are walked in slabs of whole
// sets.
inline int check_prefix_args(const gcre_set_input* in, const PrefixSteps& st, bool have_px, int32_t iterations, int method,
                             int32_t W32p, int32_t Kpad, bool want_null, double max_mb, const std::string& who, std::string& msg) {
  const int64_t S = in->n_sets;
  if (!have_px) { msg = who + ": NULL argument (px_out)"; return GCRE_ERR_ARG; }
  if (S > 0x7fffffff || (S > 0 && in->set_off[S] > 0x7fffffff)) { msg = who + ": too many sets or members"; return GCRE_ERR_ARG; }
  if (iterations <= 0) return GCRE_OK;
  for (int64_t s = 0; s < S; s++) {
    if (!prefix_set_valid(in, s)) continue;   // never launched
    const int64_t n = st.off[(size_t)s + 1] - st.off[(size_t)s];
    const double bytes = prefix_set_bytes(n, method, W32p, Kpad, want_null);
    if (bytes > max_mb * 1048576.0) {
      msg = who + ": the " + std::to_string(n) + " step rows of set " + std::to_string(s) + " take " + std::to_string((int64_t)bytes) +
            " bytes: above GCRE_PREFIX_MAX_MB = " + std::to_string(max_mb);
      return GCRE_ERR_ARG;
    }
  }
  return GCRE_OK;
}

// One slab: valid sets [v0, v0 + nv) of the list of valid sets (input order) and the step rows they hold
struct PrefixSlab { int64_t v0, nv, steps; };

// The slabs: whole valid sets in input order; a slab closes before the set that would take it over `max_mb` or over
// `slab_sets` sets (0: no such bound).  `vsteps` [V] the steps of every valid set.  The check above has passed: every set fits.
inline void prefix_slabs(const std::vector<int64_t>& vsteps, int method, int32_t W32p, int32_t Kpad, bool want_null, double max_mb,
                         int64_t slab_sets, std::vector<PrefixSlab>& slabs) {
  slabs.clear();
  const double cap = max_mb * 1048576.0;
  PrefixSlab cur{0, 0, 0};
  double bytes = 0;
  for (int64_t v = 0; v < (int64_t)vsteps.size(); v++) {
    const double b = prefix_set_bytes(vsteps[(size_t)v], method, W32p, Kpad, want_null);
    if (cur.nv > 0 && (bytes + b > cap || (slab_sets > 0 && cur.nv >= slab_sets) || cur.steps + vsteps[(size_t)v] > 0x7fffffff)) {
      slabs.push_back(cur);
      cur = PrefixSlab{v, 0, 0};
      bytes = 0;
    }
    cur.nv++;
    cur.steps += vsteps[(size_t)v];
    bytes += b;
  }
  if (cur.nv > 0) slabs.push_back(cur);
}

// One wave of a block of k_prefix_null: the set in slot `slot` of the slab (-1: none, the wave idles on the slab's first row),
// whose `steps` step rows start at row `row0` of the slab
struct PrefixWave { int32_t slot, steps; int64_t row0; };
static_assert(sizeof(PrefixWave) == 16, "the layout the kernel reads");

// The sets of a slab in the order the blocks take them: by step count descending, ties by slot (stable); slot = the set's
// position in the slab, rows in slot order.  Block b takes entries [4 b, 4 b + 4) of the order, so it loops to its first
// wave's step count.  order [nv]; waves [ceil(nv / 4) * 4].
inline void prefix_blocks(const int64_t* vsteps, int64_t nv, std::vector<int32_t>& order, std::vector<PrefixWave>& waves) {
  std::vector<int64_t> row0((size_t)nv + 1, 0);
  for (int64_t i = 0; i < nv; i++) row0[(size_t)i + 1] = row0[(size_t)i] + vsteps[i];
  order.resize((size_t)nv);
  for (int64_t i = 0; i < nv; i++) order[(size_t)i] = (int32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return vsteps[x] > vsteps[y]; });
  const int64_t nb = (nv + kPrefixBlockSets - 1) / kPrefixBlockSets;
  waves.assign((size_t)(nb * kPrefixBlockSets), PrefixWave{-1, 0, 0});
  for (int64_t i = 0; i < nv; i++) {
    const int32_t e = order[(size_t)i];
    waves[(size_t)i] = PrefixWave{e, (int32_t)vsteps[e], row0[(size_t)e]};
  }
}

}  // namespace gcre_prefix

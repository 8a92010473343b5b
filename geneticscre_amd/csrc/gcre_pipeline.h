// gcre_pipeline.h -- what the one-call pipeline (gcre_host_pipeline.hip) works out from numbers and host arrays alone: the
// top-k merge, the sets a permutation window is planned for, the window rounding, a device's shard and its number of
// threshold exchanges, the hints of levels 4 and 5, and the hub where the device threads of one call meet.  Plain C++17 over
// include/gcre_hip.h, no HIP: tests/native/pipeline_main.cpp drives it on a machine without a GPU.
#pragma once
#include "../../include/gcre_hip.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <limits>
#include <mutex>
#include <vector>

namespace gcre_host __attribute__((visibility("hidden"))) {

constexpr int kWindowTile = 2048;   // permutations per tile of the count planes (kSparseTile, gcre_kernels.h)

struct Candidate {
  double score;
  int64_t path;   // absolute joined-path ordinal
  int32_t src, trg, cases, ctrls;
};

// ---- merge: global heap starts with the {-inf,-1,-1,0,0} sentinel (join_base.cpp:192-194); the best
// top_k of {sentinel} U candidates survive, reported in ascending order (format_result :140-151).
// Ties: smaller joined-path ordinal wins (DESIGN.md "Ties").
inline void merge_candidates(std::vector<Candidate>& cands, int top_k, gcre_result* out) {
  std::sort(cands.begin(), cands.end(), [](const Candidate& a, const Candidate& b) {
    if (a.score != b.score) return a.score > b.score;
    return a.path < b.path;
  });
  size_t keepn = std::min(cands.size(), (size_t)top_k);
  const bool with_sentinel = cands.size() < (size_t)top_k;
  const size_t n_out = keepn + (with_sentinel ? 1 : 0);
  out->n = (int32_t)n_out;
  out->scores = (double*)std::calloc(std::max<size_t>(n_out, 1), sizeof(double));
  out->src = (int32_t*)std::calloc(std::max<size_t>(n_out, 1), sizeof(int32_t));
  out->trg = (int32_t*)std::calloc(std::max<size_t>(n_out, 1), sizeof(int32_t));
  out->cases = (int32_t*)std::calloc(std::max<size_t>(n_out, 1), sizeof(int32_t));
  out->ctrls = (int32_t*)std::calloc(std::max<size_t>(n_out, 1), sizeof(int32_t));
  size_t o = 0;
  if (with_sentinel) {
    out->scores[o] = -std::numeric_limits<double>::infinity();
    out->src[o] = -1;
    out->trg[o] = -1;
    o++;
  }
  for (size_t i = keepn; i-- > 0;) {   // ascending: worst kept first
    out->scores[o] = cands[i].score;
    out->src[o] = cands[i].src;
    out->trg[o] = cands[i].trg;
    out->cases[o] = cands[i].cases;
    out->ctrls[o] = cands[i].ctrls;
    o++;
  }
}

// count_total_paths() of a level's uid table
inline int64_t total_paths(const gcre_level& lv) {
  int64_t t = 0;
  for (int64_t i = 0; i < lv.n_uids; i++) t += std::max(lv.uid_count[i], 0);
  return t;
}

// The sets a permutation window is planned for (gcre_plan_perm_window): the two data matrices, then the kept sets of
// levels 1a, 2 and 3 as far as the path length goes.  Every device of a call plans with the same list.
inline std::vector<int64_t> set_rows(const gcre_pp_input* in) {
  std::vector<int64_t> rows = {in->data1_rows, in->data2_rows};
  for (int lv = 0; lv < 4 && lv <= in->path_length; lv++)
    if (lv != 1) rows.push_back(total_paths(in->level[lv]));
  return rows;
}

// gcre_pp_input.window_perms > 0: whole tiles, at least one; everything when it reaches the permutation count
inline int round_window_perms(int window_perms, int Kall) {
  return window_perms >= Kall ? std::max(Kall, 1) : std::max(kWindowTile, window_perms / kWindowTile * kWindowTile);
}

// one device of several: its slice [begin, end) of a level's joined-path ordinals
inline void shard_bounds(int64_t total, int rank, int world, int64_t* begin, int64_t* end) {
  *begin = total * rank / world;
  *end = total * (rank + 1) / world;
}

// The devices of a call share their running maxima during a join: one exchange per doubling of a device's work beyond
// `unit` path-tiles (GCRE_EXCHANGE_UNIT; as ResidentPlan.exchange_count), `most` at the most (GCRE_EXCHANGE_MAX); 0: none.
// The same on every device: it depends on nothing a device has of its own.
inline int exchange_count(int64_t total, int world, int window, double unit, double most) {
  const double work = (double)total / world * (double)((window + kWindowTile - 1) / kWindowTile);
  if (!(unit > 0 && work >= 2 * unit)) return 0;
  return (int)std::min(most, std::floor(std::log2(work / unit)));
}

// tag = (level, permutation window, ordinal of the exchange inside the join; 0xffff: the merge that ends the level): every
// device of a round must bring the same one -- a device that skipped or repeated an exchange would otherwise MAX another
// level's maxima into the thresholds
inline uint64_t hub_tag(int level, int k0, int round) {
  return ((uint64_t)(uint32_t)level << 48) ^ ((uint64_t)(uint32_t)k0 << 16) ^ (uint64_t)(round & 0xffff);
}

// Level 4's hint.  paths2[loc] = (c, d) with c already on paths3[idx]: the join adds gene d = the data row level 2 joined at
// loc (signed method: level 2 put d into the (-) half when the relation's sign is not 1, gcre.h:71-81 -> bit 31)
inline std::vector<int32_t> added_rows_hint(int method, const int32_t* data_inds, int64_t n, const gcre_level& l2) {
  std::vector<int32_t> added((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    const bool neg = method == 2 && i < l2.n_signs && l2.signs[i] != 1;
    added[(size_t)i] = (int32_t)((uint32_t)data_inds[i] | (neg ? 0x80000000u : 0u));
  }
  return added;
}

// Level 5's hint.  paths3[loc] = (c, d, e) with c on paths3[idx]: the join adds the 2-gene path (d, e) = paths2[second
// relation], and the second relation of joined path q of level 3 is the paths1 row it joined: location3[uid] + offset
inline std::vector<int32_t> second_relation_hint(int method, const gcre_level& l3) {
  std::vector<int32_t> second;
  for (int64_t i = 0; i < l3.n_uids; i++) {
    // signed method: (d, e) sits in paths3[loc] with both halves swapped when the relation (c, d) is not positive
    const bool neg = method == 2 && i < l3.n_signs && l3.signs[i] != 1;
    for (int32_t t = 0; t < l3.uid_count[i]; t++)
      second.push_back((int32_t)((uint32_t)(l3.uid_location[i] + t) | (neg ? 0x80000000u : 0u)));
  }
  return second;
}

// gcre_process_paths_devices: the device threads of one call meet here to MAX-merge their running null maxima during a
// join (gcre_join_opts.exchange, served inside the library).  K floats per call: the host does the reduction.  With RCCL
// the data stays on the devices and only the meeting (`meet`) happens here.
struct ExchangeHub {
  int n = 0;
  std::mutex m;
  std::condition_variable cv;
  int arrived = 0;
  uint64_t gen = 0;
  bool failed = false, timed_out = false;
  double timeout_s = 300.0;
  std::vector<float> acc, result;
  uint64_t round_tag = 0;
  // every device of a round brings the same hub_tag
  int reduce(std::vector<float>& mine, uint64_t tag) {   // in: this device's maxima; out: the MAX over all devices
    std::unique_lock<std::mutex> lk(m);
    if (failed) return 1;
    if (arrived == 0) {
      acc = mine;
      round_tag = tag;
    } else {
      if (acc.size() != mine.size() || tag != round_tag) { failed = true; cv.notify_all(); return 1; }
      for (size_t i = 0; i < mine.size(); i++) acc[i] = std::max(acc[i], mine[i]);
    }
    if (++arrived == n) {
      result.swap(acc);
      arrived = 0;
      gen++;
      cv.notify_all();
    } else {
      // a device that never arrives (its thread died, it took another road through the join) must not hold the others for
      // ever: past the deadline the round -- and with it the call -- fails (GCRE_HUB_TIMEOUT_S, default 300 s: a join of
      // configs[4] on a shared GPU takes seconds)
      const uint64_t g = gen;
      if (!cv.wait_for(lk, std::chrono::duration<double>(timeout_s), [&] { return gen != g || failed; })) {
        failed = true;
        timed_out = true;
        cv.notify_all();
        return 1;
      }
      if (gen == g) return 1;   // somebody failed before this round completed
    }
    mine = result;
    return 0;
  }
  // every device arrives with the same tag or the round fails; no data (the collective that follows moves it)
  int meet(uint64_t tag) {
    std::vector<float> none;
    return reduce(none, tag);
  }
  void fail() {
    std::lock_guard<std::mutex> lk(m);
    failed = true;
    cv.notify_all();
  }
};

}  // namespace gcre_host

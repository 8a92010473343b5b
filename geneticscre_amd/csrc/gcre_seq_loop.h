// gcre_seq_loop.h -- the batch loop every sequential stage drives (hipcc only): the schedule
// of gcre_sequential.h, the batch's masks -- uniform (k_seq_masks) or weighted (k_seq_weighted_search, the cut at a left-over
// permutation by the rule of gcre_seq_weighted.h, k_seq_weighted_write) --, the stage's own null kernel through a callback,
// k_seq_retire, the one dword that comes back per batch and the GCRE_SEQ_STATS trace.  gcre_host_sequential.hip runs it with
// k_seq_null over the union rows, gcre_host_seq_prefix.hip with k_seq_prefix_null over a slab's step rows.  Nothing here is
// part of the ABI.
#pragma once
#include "gcre_set_stage.h"
#include "gcre_seq_weighted.h"

#include <functional>

namespace gcre_host __attribute__((visibility("hidden"))) {

// A device array of one batch that grows with the schedule and is freed with the call
struct BatchBuf {
  void* p = nullptr;
  size_t bytes = 0;
  BatchBuf() = default;
  BatchBuf(const BatchBuf&) = delete;
  BatchBuf& operator=(const BatchBuf&) = delete;
  ~BatchBuf() { if (p) (void)hipFree(p); }
  // (the stream is idle here: every batch ends with the read-back of the active count)
  void ensure(DevScratch& d, size_t need) {
    if (!d.ok() || need <= bytes) return;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    d.e = hipMalloc(&p, need);
    if (d.ok()) bytes = need;
  }
};

// What a call draws its permutations from: the seed, the strata as check() left them, and for the weighted call the cap and
// the plan of gcre_weighted.h
struct SeqDraw {
  uint64_t seed = 0;
  const int32_t* stratum = nullptr;            // [n] or nullptr: one stratum
  const std::vector<uint32_t>* cases_in = nullptr;
  const std::vector<uint32_t>* size_of = nullptr;
  const double* odds = nullptr;                // weighted iff given
  uint32_t wt_cap = 0;
  const gcre_weighted::WeightedPlan* plan = nullptr;
};

// Launches the stage's null kernel for one batch: the bit rows [nactive][stride / 64] of the sets on `active` against the nb
// permutations in masks [W32p][stride], nkt tiles
using SeqNullLaunch = std::function<hipError_t(const uint32_t* active, int64_t nactive, const uint32_t* masks, int stride, int nb,
                                               int nkt, unsigned long long* bits)>;

// What the loop leaves: the sets still active behind the last batch, R and its stratum (-1: none), and -- unless the call is
// refused by the rule of gcre_seq_weighted.h -- per set its exceedances while active and the position of its stop (0: none)
struct SeqLoopResult {
  int64_t nact = 0, left_over = -1, batches = 0;
  int left_stratum = -1;
  bool refused = false;
  std::vector<uint32_t> prior;     // [V]
  std::vector<long long> nperm;    // [V]
};

// V sets with indices 0 .. V-1; `act` the first active list.  Per batch: its masks, the bit rows of the active sets, the
// retirement; one dword comes back, the length of the next list.  r0 moves on by the batch every turn, so the loop ends at
// max_perms whatever the device reports.  `launches` counts the kernels.  Errors stay in `d`.
inline void seq_batch_loop(gcre_ctx* c, DevScratch& d, const SeqDraw& dr, int64_t h, int64_t max_perms, int64_t V,
                           const std::vector<uint32_t>& act, const SeqNullLaunch& null_launch, int64_t& launches, SeqLoopResult& out) {
  const Geometry& g = c->g;
  const int W32p = 2 * g.Wp;
  const std::vector<uint32_t>& cases_in = *dr.cases_in;
  const std::vector<uint32_t>& size_of = *dr.size_of;
  const int32_t* stratum = dr.stratum;
  const int ns = (int)cases_in.size();

  uint32_t* d_act[2] = {d.take<uint32_t>((size_t)V), d.take<uint32_t>((size_t)V)};
  if (!act.empty()) d.upload(d_act[0], act.data(), act.size());
  uint32_t* d_prior = d.take<uint32_t>((size_t)V);
  long long* d_nperm = d.take<long long>((size_t)V);
  uint32_t* d_count = d.take<uint32_t>(1);
  d.zero(d_prior, (size_t)V);
  d.zero(d_nperm, (size_t)V);
  const uint32_t* d_cases = d.put(cases_in.data(), (size_t)ns);
  const uint32_t* d_size = d.put(size_of.data(), (size_t)ns);
  const int32_t* d_str = stratum ? d.put(stratum, (size_t)g.n) : nullptr;

  const bool weighted = dr.odds != nullptr;
  const double max_mb = gcre_sequential::seq_max_mb();
  const int64_t cap = gcre_sequential::seq_batch_perms_env();
  const bool work = !weighted && ns > kSeqRegStrata;
  // per permutation: its mask, and need / rem where they are in memory -- or, weighted, its accepted attempts
  const int32_t dwords = weighted ? gcre_seq_weighted::seq_weighted_dwords(W32p, ns) : W32p + (work ? 2 * ns : 0);
  BatchBuf masks, bits, wk;

  // the weighted call, once: per stratum, one behind the other, the columns and their thresholds (as
  // gcre_generate_weighted_masks lists them), the thresholds by column, and the one dword the search reports through
  SeqWeightedArgs wa{};
  const uint32_t no_column = gcre_seq_weighted::kSeqWtNoColumn;
  if (weighted) {
    const gcre_weighted::WeightedPlan& plan = *dr.plan;
    std::vector<uint32_t> soff((size_t)ns + 1, 0u);
    for (int s = 0; s < ns; s++) soff[(size_t)s + 1] = soff[(size_t)s] + size_of[(size_t)s];
    std::vector<int32_t> cols((size_t)g.n + 1);   // (never empty)
    std::vector<uint32_t> cthr((size_t)g.n + 1), at(soff.begin(), soff.end() - 1);
    for (int32_t q = 0; q < g.n; q++) {
      const uint32_t i = at[(size_t)(stratum ? stratum[q] : 0)]++;
      cols[i] = q;
      cthr[i] = plan.thr[(size_t)q];
    }
    wa.seed1 = gcre_weighted::wt_seed(dr.seed);
    wa.cols = d.put(cols.data(), cols.size());
    wa.cthr = d.put(cthr.data(), cthr.size());
    wa.soff = d.put(soff.data(), soff.size());
    wa.cases_in = d_cases;
    wa.first = d.take<uint32_t>(1);
    wa.cap = dr.wt_cap;
    wa.stratum = ns > 1 ? d_str : nullptr;
    wa.thr = d.put(plan.thr.data(), (size_t)g.n);
    wa.S = ns;
    wa.n = g.n;
    wa.W32p = W32p;
    d.sync();   // (the host lists above end with this block)
  }
  int64_t left_over = -1;   // R of gcre_seq_weighted.h, once a batch has held it
  int left_stratum = -1;

  std::vector<int64_t> trace;   // the active count behind every batch (GCRE_SEQ_STATS)
  int64_t r0 = 0, batch = 0, nact = (int64_t)act.size();
  int cur = 0;
  while (d.ok() && r0 < max_perms && nact > 0) {
    batch = gcre_sequential::sequential_batch(batch, dwords, nact, max_mb, cap);
    int64_t nb = std::min(batch, max_perms - r0);
    int nkt = (int)((nb + kSetPermTile - 1) / kSetPermTile);
    int64_t stride = (int64_t)nkt * kSetPermTile;
    masks.ensure(d, (size_t)W32p * (size_t)stride * 4);
    bits.ensure(d, (size_t)nact * (size_t)(stride / 64) * 8);
    if (work) wk.ensure(d, (size_t)2 * (size_t)ns * (size_t)stride * 4);
    if (weighted) wk.ensure(d, (size_t)ns * (size_t)stride * 4);   // att [ns][stride]
    if (!d.ok()) break;

    if (!weighted) {
      SeqMaskArgs ma{};
      ma.seed = dr.seed;
      ma.r0 = (uint64_t)r0;
      ma.stratum = ns > 1 ? d_str : nullptr;
      ma.cases_in = d_cases;
      ma.size_of = d_size;
      ma.work = (uint32_t*)wk.p;
      ma.masks = (uint32_t*)masks.p;
      ma.n = g.n;
      ma.n_strata = ns;
      ma.nb = (int)nb;
      ma.W32p = W32p;
      ma.stride = (int)stride;
      d.e = launch_seq_masks(ma, c->stream);
      if (d.ok()) launches++;
    } else {
      // search; the first left-over column comes back; the columns in front of it are written and scored
      wa.r0 = (uint64_t)r0;
      wa.att = (uint32_t*)wk.p;
      wa.masks = (uint32_t*)masks.p;
      wa.nb = (int)nb;
      wa.att_stride = (int)stride;
      d.upload(wa.first, &no_column, 1);
      if (d.ok()) {
        d.e = launch_seq_weighted_search(wa, c->stream);
        if (d.ok()) launches++;
      }
      uint32_t first = no_column;
      d.download(&first, wa.first, 1);
      d.sync();
      if (!d.ok()) break;
      const gcre_seq_weighted::SeqWeightedCut cut = gcre_seq_weighted::seq_weighted_cut(r0, nb, first);
      if (cut.left_over >= 0) {
        left_over = cut.left_over;
        std::vector<uint32_t> col((size_t)ns);
        for (int s = 0; s < ns; s++) d.download(&col[(size_t)s], wa.att + (size_t)s * (size_t)stride + first, 1);
        d.sync();
        if (!d.ok()) break;
        left_stratum = gcre_seq_weighted::seq_weighted_left_stratum(col.data(), ns, 1, 0);
        if (cut.keep == 0) break;   // nothing in front of R: nothing is drawn or scored
        nb = cut.keep;
        nkt = (int)((nb + kSetPermTile - 1) / kSetPermTile);
        stride = (int64_t)nkt * kSetPermTile;
      }
      wa.nb = (int)nb;
      wa.stride = (int)stride;
      d.e = launch_seq_weighted_write(wa, c->stream);
      if (d.ok()) launches++;
    }

    if (d.ok()) {
      d.e = null_launch(d_act[cur], nact, (const uint32_t*)masks.p, (int)stride, (int)nb, nkt, (unsigned long long*)bits.p);
      if (d.ok()) launches++;
    }

    SeqRetireArgs ra{};
    ra.bits = (const unsigned long long*)bits.p;
    ra.active = d_act[cur];
    ra.next = d_act[cur ^ 1];
    ra.n_next = d_count;
    ra.prior = d_prior;
    ra.n_perm = d_nperm;
    ra.r0 = (uint64_t)r0;
    ra.nactive = nact;
    ra.wstride = stride / 64;
    ra.nw = (int)(stride / 64);
    ra.h = (uint32_t)h;
    d.zero(d_count, 1);
    if (d.ok()) {
      d.e = launch_seq_retire(ra, c->stream);
      if (d.ok()) launches++;
    }
    uint32_t left = 0;
    d.download(&left, d_count, 1);
    d.sync();
    if (!d.ok()) break;
    nact = std::min<int64_t>((int64_t)left, nact);   // a list never grows
    trace.push_back(nact);
    cur ^= 1;
    r0 += nb;
    if (left_over >= 0) break;   // the batch was cut at R
  }
  if (!d.ok()) return;
  out.nact = nact;
  out.left_over = left_over;
  out.left_stratum = left_stratum;
  out.batches = (int64_t)trace.size();
  out.refused = gcre_seq_weighted::seq_weighted_refused(left_over, nact);
  if (out.refused) return;   // nothing is read back: the entry refuses
  out.prior.assign((size_t)V, 0u);
  out.nperm.assign((size_t)V, 0);
  d.download(out.prior.data(), d_prior, (size_t)V);
  d.download(out.nperm.data(), d_nperm, (size_t)V);
  d.sync();
  if (!d.ok()) return;
  if (std::getenv("GCRE_SEQ_STATS")) {   // (tools/sequential_time.py)
    std::string s;
    for (int64_t x : trace) s += (s.empty() ? "" : ",") + std::to_string(x);
    fprintf(stderr, "sequential sets=%lld hits=%lld max_perms=%lld batches=%zu last_batch=%lld active=%s%s\n", (long long)V, (long long)h,
            (long long)max_perms, trace.size(), (long long)batch, s.c_str(),
            weighted ? (" weighted strata=" + std::to_string(ns) + " left_over=" + std::to_string(left_over)).c_str() : "");
  }
}

// one set's record from what the loop left
inline void seq_fill(gcre_seq_score& o, uint32_t prior, long long nperm, int64_t h, int64_t max_perms) {
  const bool stopped = nperm != 0;
  o.n_hit = stopped ? h : (int64_t)prior;
  o.n_perm = stopped ? (int64_t)nperm : max_perms;
  o.stopped = stopped ? 1 : 0;
}

}  // namespace gcre_host

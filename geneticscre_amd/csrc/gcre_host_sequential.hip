// gcre_host_sequential.hip -- gcre_score_sets_sequential on a context: the stage that score_sets_common
// (gcre_set_stage.h) runs behind the set scores.  The rule -- argument checks, strata, batch schedule -- is
// gcre_sequential.h's; here are the uploads, the batch loop over gcre_sequential.hip's kernels and the downloads.
// gcre_score_sets_sequential_weighted is the same stage with another mask step: the batch's masks come from
// gcre_seq_weighted.hip's two kernels, by the rule of gcre_seq_weighted.h, with one read-back between them.  Host code only.
#include "gcre_set_stage.h"
#include "gcre_seq_weighted.h"

namespace {

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

struct SequentialStage final : SetStage {
  const uint64_t seed;
  const int32_t* const stratum;
  const int n_strata;
  const int64_t h, max_perms;
  gcre_seq_score* const seq_out;
  std::vector<uint32_t> cases_in, size_of;   // per stratum, from check()
  // the weighted call (odds given): its cap, its plan from check(), and what run() leaves for the entry to refuse
  const double* const odds;
  const int64_t max_attempts;
  uint32_t wt_cap = 0;
  gcre_weighted::WeightedPlan plan;
  std::string who_, refusal;

  SequentialStage(uint64_t seed_, const int32_t* stratum_, int n_strata_, int64_t h_, int64_t max_perms_, gcre_seq_score* seq_out_,
                  const double* odds_ = nullptr, int64_t max_attempts_ = 0)
      : seed(seed_), stratum(stratum_), n_strata(n_strata_), h(h_), max_perms(max_perms_), seq_out(seq_out_), odds(odds_),
        max_attempts(max_attempts_) {}

  // the argument checks of gcre_sequential.h, the strata as gcre_generate_perm_masks reads them, and what the device's 32-bit
  // set indices add
  int check(gcre_ctx* c, const gcre_set_input* in, const std::string& who) override {
    std::string msg;
    if (int rc = gcre_sequential::check_sequential_args(h, max_perms, seq_out != nullptr, who, msg)) return fail(c, rc, msg);
    if (odds) {   // the strata and the refusals of gcre_weighted.h
      who_ = who;
      if (int rc = gcre_weighted::weighted_plan(c->g.n, c->g.n_cases, odds, stratum, n_strata, who, plan, msg)) return fail(c, rc, msg);
      if (int rc = gcre_weighted::weighted_cap(max_attempts, who, wt_cap, msg)) return fail(c, rc, msg);
      if (int rc = gcre_weighted::weighted_plan_fits(plan, wt_cap, who, msg)) return fail(c, rc, msg);
      cases_in = plan.cases_in;
      size_of = plan.size_of;
    } else if (int rc = gcre_sequential::strata_counts(c->g.n, c->g.n_cases, stratum, n_strata, cases_in, size_of, who, msg)) {
      return fail(c, rc, msg);
    }
    if (in->n_sets > 0x7fffffff) return fail(c, GCRE_ERR_ARG, who + ": too many sets");
    return GCRE_OK;
  }

  // an invalid set -1; zeros without a permutation
  void defaults(const gcre_set_input* in, const gcre_set_score* out) override {
    for (int64_t s = 0; s < in->n_sets; s++) {
      const int64_t v = out[s].valid ? 0 : -1;
      seq_out[s] = {v, v, 0, 0};
    }
  }

  bool runs(const gcre_ctx*) const override { return max_perms > 0; }

  // The valid sets' union rows, totals and observed scores are on the device as k_set_null reads them.  Every set with a
  // score starts on the active list (a NaN score is never reached: such a set keeps zero exceedances).  Per batch: its masks,
  // the bit rows of the active sets, the retirement; one dword comes back, the length of the next list.  r0 moves on by the
  // batch every turn, so the loop ends at max_perms whatever the device reports.
  void run(const SetScoreRun& r) override {
    gcre_ctx* c = r.c;
    DevScratch& d = r.d;
    const Geometry& g = c->g;
    const int M = g.method;
    const int64_t V = (int64_t)r.vset.size();
    const int W32p = 2 * g.Wp;
    const int ns = (int)cases_in.size();

    std::vector<uint32_t> thr((size_t)V), act;
    for (int64_t v = 0; v < V; v++) {
      thr[(size_t)v] = f32_threshold(r.obs[(size_t)v]);
      // (weighted: a NaN score's threshold is past +inf, so the set counts nothing and never stops -- it stays active, and
      // with it the search for a left-over permutation runs to max_perms, as gcre_seq_weighted.h's rule asks)
      if (r.obs[(size_t)v] == r.obs[(size_t)v] || odds) act.push_back((uint32_t)v);
    }
    const uint32_t* d_thr = d.put(thr.data(), (size_t)V);
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

    const bool weighted = odds != nullptr;
    const double max_mb = gcre_sequential::seq_max_mb();
    const int64_t cap = gcre_sequential::seq_batch_perms_env();
    const bool work = !weighted && ns > kSeqRegStrata;
    // per permutation: its mask, and need / rem where they are in memory -- or, weighted, its accepted attempts
    const int32_t dwords = weighted ? gcre_seq_weighted::seq_weighted_dwords(W32p, ns) : W32p + (work ? 2 * ns : 0);
    const int64_t tpb = set_null_tile_sets(M);
    BatchBuf masks, bits, wk;

    // the weighted call, once: per stratum, one behind the other, the columns and their thresholds (as
    // gcre_generate_weighted_masks lists them), the thresholds by column, and the one dword the search reports through
    SeqWeightedArgs wa{};
    const uint32_t no_column = gcre_seq_weighted::kSeqWtNoColumn;
    if (weighted) {
      std::vector<uint32_t> soff((size_t)ns + 1, 0u);
      for (int s = 0; s < ns; s++) soff[(size_t)s + 1] = soff[(size_t)s] + size_of[(size_t)s];
      std::vector<int32_t> cols((size_t)g.n + 1);   // (never empty)
      std::vector<uint32_t> cthr((size_t)g.n + 1), at(soff.begin(), soff.end() - 1);
      for (int32_t q = 0; q < g.n; q++) {
        const uint32_t i = at[(size_t)(stratum ? stratum[q] : 0)]++;
        cols[i] = q;
        cthr[i] = plan.thr[(size_t)q];
      }
      wa.seed1 = gcre_weighted::wt_seed(seed);
      wa.cols = d.put(cols.data(), cols.size());
      wa.cthr = d.put(cthr.data(), cthr.size());
      wa.soff = d.put(soff.data(), soff.size());
      wa.cases_in = d_cases;
      wa.first = d.take<uint32_t>(1);
      wa.cap = wt_cap;
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
        ma.seed = seed;
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
        if (d.ok()) c->sequential_launches++;
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
          if (d.ok()) c->sequential_launches++;
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
        if (d.ok()) c->sequential_launches++;
      }

      SeqNullArgs na{};
      na.rows = (const uint32_t*)r.d_rows;
      na.masks = (const uint32_t*)masks.p;
      na.tot = r.d_tot;
      na.thr = d_thr;
      na.t32 = c->d_t32;
      na.d64 = c->d_dmax;
      na.d64n = c->d_dmaxn ? c->d_dmaxn : c->d_dmax;
      na.active = d_act[cur];
      na.bits = (unsigned long long*)bits.p;
      na.nactive = nact;
      na.npt = (nact + tpb - 1) / tpb;
      na.W32p = W32p;
      na.stride = (int)stride;
      na.K = (int)nb;
      na.nkt = nkt;
      // one set tile per block while that makes at least ~8 blocks per resident block slot, more per block beyond (k_set_null's rule)
      const int64_t slots = (int64_t)c->cus * 4 * 8;
      const int64_t per = std::max<int64_t>(1, (na.npt * na.nkt) / slots);
      na.pgroups = (int)std::min<int64_t>((na.npt + per - 1) / per, 0x7fffffff / std::max(na.nkt, 1));
      if (d.ok()) {
        d.e = launch_seq_null(na, M, c->stream);
        if (d.ok()) c->sequential_launches++;
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
        if (d.ok()) c->sequential_launches++;
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
    if (gcre_seq_weighted::seq_weighted_refused(left_over, nact)) {   // seq_out keeps its defaults; the entry refuses
      refusal = gcre_seq_weighted::seq_weighted_message(who_, left_over, left_stratum, wt_cap, nact, max_perms);
      return;
    }

    std::vector<uint32_t> prior((size_t)V);
    std::vector<long long> nperm((size_t)V);
    d.download(prior.data(), d_prior, (size_t)V);
    d.download(nperm.data(), d_nperm, (size_t)V);
    d.sync();
    if (!d.ok()) return;
    for (int64_t v = 0; v < V; v++) {
      gcre_seq_score& o = seq_out[r.vset[(size_t)v]];
      const bool stopped = nperm[(size_t)v] != 0;
      o.n_hit = stopped ? h : (int64_t)prior[(size_t)v];
      o.n_perm = stopped ? (int64_t)nperm[(size_t)v] : max_perms;
      o.stopped = stopped ? 1 : 0;
    }
    if (std::getenv("GCRE_SEQ_STATS")) {   // (tools/sequential_time.py)
      std::string s;
      for (int64_t x : trace) s += (s.empty() ? "" : ",") + std::to_string(x);
      fprintf(stderr, "sequential sets=%lld hits=%lld max_perms=%lld batches=%zu last_batch=%lld active=%s%s\n", (long long)V, (long long)h,
              (long long)max_perms, trace.size(), (long long)batch, s.c_str(),
              weighted ? (" weighted strata=" + std::to_string(ns) + " left_over=" + std::to_string(left_over)).c_str() : "");
    }
  }
};

}  // namespace

extern "C" {

// Sequential permutation p-values of the given sets: gcre_score_sets, then the same device rows against batches of
// permutations drawn as they are needed, every set until its h-th exceedance.
int gcre_score_sets_sequential(gcre_ctx* c, const gcre_set_input* in, uint64_t seed, const int32_t* stratum, int n_strata, int64_t h,
                               int64_t max_perms, gcre_set_score* out, int64_t cap, int64_t* n_out, gcre_seq_score* seq_out) {
  SequentialStage st(seed, stratum, n_strata, h, max_perms, seq_out);
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_sequential", &st);
}

// The same with covariate-adjusted masks: permutation r is mask r of gcre_generate_weighted_masks(seed, odds, stratum, n_strata,
// max_attempts).  The one refusal that comes after launches is gcre_seq_weighted.h's.
int gcre_score_sets_sequential_weighted(gcre_ctx* c, const gcre_set_input* in, uint64_t seed, const double* odds, const int32_t* stratum,
                                        int n_strata, int64_t max_attempts, int64_t h, int64_t max_perms, gcre_set_score* out, int64_t cap,
                                        int64_t* n_out, gcre_seq_score* seq_out) {
  const std::string who = "score_sets_sequential_weighted";
  if (c && !odds) return fail(c, GCRE_ERR_ARG, who + ": NULL argument (odds)");
  SequentialStage st(seed, stratum, n_strata, h, max_perms, seq_out, odds, max_attempts);
  const int rc = score_sets_common(c, in, out, cap, n_out, nullptr, who, &st);
  if (rc == GCRE_OK && !st.refusal.empty()) return fail(c, GCRE_ERR_RANGE, st.refusal);
  return rc;
}

int64_t gcre_sequential_launches(const gcre_ctx* c) { return c ? c->sequential_launches : -1; }

}  // extern "C"

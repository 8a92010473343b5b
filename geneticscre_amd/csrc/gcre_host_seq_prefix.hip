// gcre_host_seq_prefix.hip -- gcre_score_sets_prefix_sequential and gcre_score_sets_dose_sequential on a context (DESIGN.md
// §3.25): the stage that score_sets_common (gcre_set_stage.h) runs behind the set scores.  The plan -- argument checks, first
// active list, what the slabs add up to -- is gcre_seq_prefix.h's, the two row variants gcre_steps.h's; per slab StepRows
// (gcre_step_rows.h) builds and scores the step rows with the three launches of the resident entries (gcre_prefix.hip /
// gcre_dose.hip, unchanged); here are the draw, the batch loop of gcre_seq_loop.h with k_seq_prefix_null (gcre_seq_prefix.hip)
// as its null kernel, and the totals.  Host code only.
#include "gcre_seq_loop.h"
#include "gcre_step_rows.h"

namespace {

static_assert(sizeof(gcre_dose_score) == 48, "the ABI");

template <typename Variant>
struct SeqPrefixStage final : SetStage {
  Variant v;   // what the entry takes and returns beside the records
  const uint64_t seed;
  const int32_t* const stratum;
  const int n_strata;
  const int64_t h, max_perms;
  gcre_seq_score* const seq_out;
  const double* const odds;
  const int64_t max_attempts;
  std::vector<uint32_t> cases_in, size_of;   // per stratum, from check()
  uint32_t wt_cap = 0;
  gcre_weighted::WeightedPlan plan;
  std::string who_, refusal;

  SeqPrefixStage(const Variant& v_, uint64_t seed_, const double* odds_, const int32_t* stratum_, int n_strata_,
                 int64_t max_attempts_, int64_t h_, int64_t max_perms_, gcre_seq_score* seq_out_)
      : v(v_), seed(seed_), stratum(stratum_), n_strata(n_strata_), h(h_), max_perms(max_perms_), seq_out(seq_out_),
        odds(odds_), max_attempts(max_attempts_) {}

  // the argument checks of gcre_seq_prefix.h, then the strata as the sequential stage reads them
  int check(gcre_ctx* c, const gcre_set_input* in, const std::string& who) override {
    who_ = who;
    std::string msg;
    if (int rc = v.check_seq(in, seq_out != nullptr, c->g.method, 2 * c->g.Wp, gcre_prefix::prefix_max_mb(), h, max_perms, who, msg))
      return fail(c, rc, msg);
    if (odds) {   // the strata and the refusals of gcre_weighted.h
      if (int rc = gcre_weighted::weighted_plan(c->g.n, c->g.n_cases, odds, stratum, n_strata, who, plan, msg)) return fail(c, rc, msg);
      if (int rc = gcre_weighted::weighted_cap(max_attempts, who, wt_cap, msg)) return fail(c, rc, msg);
      if (int rc = gcre_weighted::weighted_plan_fits(plan, wt_cap, who, msg)) return fail(c, rc, msg);
      cases_in = plan.cases_in;
      size_of = plan.size_of;
    } else if (int rc = gcre_sequential::strata_counts(c->g.n, c->g.n_cases, stratum, n_strata, cases_in, size_of, who, msg)) {
      return fail(c, rc, msg);
    }
    return GCRE_OK;
  }

  // what the resident entries and the sequential entry leave: an invalid set -1; a NaN score, no best step and zeros without a
  // permutation
  void defaults(const gcre_set_input* in, const gcre_set_score* out) override {
    v.defaults(in, out);
    for (int64_t s = 0; s < in->n_sets; s++) {
      const int64_t n = out[s].valid ? 0 : -1;
      seq_out[s] = {n, n, 0, 0};
    }
  }

  bool runs(const gcre_ctx*) const override { return max_perms > 0; }

  // Per slab of whole valid sets StepRows builds the step rows, scores them and takes every set's best step and threshold;
  // the picks come back (one synchronisation) and give the first active list; then the whole sequential loop from permutation
  // 0, with k_seq_prefix_null between the masks and the retirement.  No resident mask is read.
  void run(const SetScoreRun& r) override {
    gcre_ctx* c = r.c;
    DevScratch& d = r.d;
    const int M = c->g.method;
    const int W32p = 2 * c->g.Wp;
    const int64_t S = r.in->n_sets;
    StepRows<Variant> rows(v, r);
    rows.plan(false, 0);
    rows.upload(r.in);
    const PrefixArgs& a = rows.a;

    SeqDraw dr;
    dr.seed = seed;
    dr.stratum = stratum;
    dr.cases_in = &cases_in;
    dr.size_of = &size_of;
    dr.odds = odds;
    dr.wt_cap = wt_cap;
    dr.plan = &plan;

    // the null kernel of a batch: k_seq_prefix_null over the slab's step rows, groups of four slots of the active list
    const SeqNullLaunch null_launch = [&](const uint32_t* active, int64_t nact, const uint32_t* masks, int stride, int nb, int nkt,
                                          unsigned long long* bits) {
      SeqPrefixArgs na{};
      na.rows = a.rows;
      na.masks = masks;
      na.tot = a.tot;
      na.thr = a.thr;
      na.row0 = a.row0;
      na.t32 = c->d_t32;
      na.d64 = c->d_dmax;
      na.d64n = c->d_dmaxn ? c->d_dmaxn : c->d_dmax;
      na.active = active;
      na.bits = bits;
      na.nactive = nact;
      na.ngroups = (nact + gcre_prefix::kPrefixBlockSets - 1) / gcre_prefix::kPrefixBlockSets;
      na.W32p = W32p;
      na.stride = stride;
      na.K = nb;
      na.nkt = nkt;
      // one group per block while that makes at least ~8 blocks per resident block slot, more per block beyond (k_set_null's rule)
      const int64_t slots = (int64_t)c->cus * 4 * 8;
      const int64_t per = std::max<int64_t>(1, (na.ngroups * na.nkt) / slots);
      na.pgroups = (int)std::min<int64_t>((na.ngroups + per - 1) / per, 0x7fffffff / std::max(na.nkt, 1));
      return launch_seq_prefix_null(na, M, c->stream);
    };

    std::vector<gcre_seq_score> seq(seq_out, seq_out + S);   // committed behind the last slab, unless the call is refused
    gcre_seq_prefix::SeqPrefixTotals totals;
    std::vector<uint32_t> act;
    for (const auto& sl : rows.slabs) {
      if (!d.ok()) break;
      rows.build(sl, c->seq_prefix_launches);
      rows.fetch(sl);
      d.sync();   // the picks give the first active list
      if (!d.ok()) break;
      rows.collect(sl);
      gcre_seq_prefix::first_active(rows.vsteps.data() + sl.v0, sl.nv, rows.score_nan.data(), odds != nullptr, act);
      SeqLoopResult res;
      seq_batch_loop(c, d, dr, h, max_perms, sl.nv, act, null_launch, c->seq_prefix_launches, res);
      if (!d.ok()) break;
      totals.add(res.left_over, res.left_stratum, res.nact);
      if (res.refused) continue;   // every slab is run: the message sums the sets still active at R
      for (int64_t e = 0; e < sl.nv; e++) seq_fill(seq[(size_t)rows.which[(size_t)e]], res.prior[(size_t)e], res.nperm[(size_t)e], h, max_perms);
    }
    if (!d.ok()) return;
    if (totals.refused()) {   // seq_out keeps its defaults; the entry refuses
      refusal = gcre_seq_weighted::seq_weighted_message(who_, totals.left_over, totals.left_stratum, wt_cap, totals.n_active, max_perms);
      return;
    }
    std::copy(seq.begin(), seq.end(), seq_out);
  }
};

template <typename Variant>
int run_entry(gcre_ctx* c, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out, const std::string& who,
              SeqPrefixStage<Variant>& st) {
  const int rc = score_sets_common(c, in, out, cap, n_out, nullptr, who, &st);
  if (rc == GCRE_OK && !st.refusal.empty()) return fail(c, GCRE_ERR_RANGE, st.refusal);
  return rc;
}

}  // namespace

extern "C" {

// Sequential p-values of the variable-threshold test: gcre_score_sets on the full sets, the step rows of every set built on
// the device, then batches of permutations drawn as they are needed, every set until the maximum over its steps has reached
// its best observed score h times.  odds NULL: uniform permutations (gcre_score_sets_sequential's); else weighted ones
// (gcre_score_sets_sequential_weighted's).
int gcre_score_sets_prefix_sequential(gcre_ctx* c, const gcre_set_input* in, const uint8_t* cut, uint64_t seed, const double* odds,
                                      const int32_t* stratum, int n_strata, int64_t max_attempts, int64_t h, int64_t max_perms,
                                      gcre_set_score* out, int64_t cap, int64_t* n_out, gcre_prefix_score* px_out,
                                      gcre_seq_score* seq_out, double* step_scores) {
  SeqPrefixStage<gcre_steps::PrefixRows> st({cut, px_out, step_scores}, seed, odds, stratum, n_strata, max_attempts, h, max_perms,
                                            seq_out);
  return run_entry(c, in, out, cap, n_out, "score_sets_prefix_sequential", st);
}

// The same of the multi-hit test: the maximum over the level rows of every set
int gcre_score_sets_dose_sequential(gcre_ctx* c, const gcre_set_input* in, const int32_t* levels, int32_t n_levels, uint64_t seed,
                                    const double* odds, const int32_t* stratum, int n_strata, int64_t max_attempts, int64_t h,
                                    int64_t max_perms, gcre_set_score* out, int64_t cap, int64_t* n_out, gcre_dose_score* dose_out,
                                    gcre_seq_score* seq_out, double* level_scores) {
  SeqPrefixStage<gcre_steps::DoseRows> st({levels, n_levels, dose_out, level_scores}, seed, odds, stratum, n_strata, max_attempts, h,
                                          max_perms, seq_out);
  return run_entry(c, in, out, cap, n_out, "score_sets_dose_sequential", st);
}

int64_t gcre_seq_prefix_launches(const gcre_ctx* c) { return c ? c->seq_prefix_launches : -1; }

}  // extern "C"

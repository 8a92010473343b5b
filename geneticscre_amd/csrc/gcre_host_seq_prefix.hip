// gcre_host_seq_prefix.hip -- gcre_score_sets_prefix_sequential and gcre_score_sets_dose_sequential on a context (DESIGN.md
// §3.25): the stage that score_sets_common (gcre_set_stage.h) runs behind the set scores.  The plan -- argument checks, first
// active list, what the slabs add up to -- is gcre_seq_prefix.h's, the steps and slabs gcre_prefix.h's; here are the
// uploads, per slab the three launches that build and score the step rows (gcre_prefix.hip / gcre_dose.hip, unchanged), the
// batch loop of gcre_seq_loop.h with k_seq_prefix_null (gcre_seq_prefix.hip) as its null kernel, and the downloads.  Host
// code only.
#include "gcre_seq_loop.h"
#include "gcre_seq_prefix.h"

namespace {

static_assert(sizeof(PrefixPick) == 32, "the layout the host reads");
static_assert(sizeof(gcre_dose_score) == 48, "the ABI");

// What the two entries take and return beside the records: the prefix entry has `cut`, `px` and `step_scores`, the dose
// entry `levels`, `ds` and `level_scores`
struct AdaptiveOut {
  const uint8_t* cut;       // [members of the list] or NULL
  gcre_prefix_score* px;    // [n_sets]
  double* step_scores;      // optional [members of the list]
  const int32_t* levels;    // [n_levels]
  int32_t n_levels;
  gcre_dose_score* ds;      // [n_sets]
  double* level_scores;     // optional [n_sets][n_levels]
};

struct SeqPrefixStage final : SetStage {
  const bool dose;
  const AdaptiveOut po;
  const uint64_t seed;
  const int32_t* const stratum;
  const int n_strata;
  const int64_t h, max_perms;
  gcre_seq_score* const seq_out;
  const double* const odds;
  const int64_t max_attempts;
  gcre_prefix::PrefixSteps st;               // the steps of every set (prefix)
  std::vector<uint32_t> cases_in, size_of;   // per stratum, from check()
  uint32_t wt_cap = 0;
  gcre_weighted::WeightedPlan plan;
  std::string who_, refusal;

  SeqPrefixStage(bool dose_, const AdaptiveOut& o, uint64_t seed_, const double* odds_, const int32_t* stratum_, int n_strata_,
                 int64_t max_attempts_, int64_t h_, int64_t max_perms_, gcre_seq_score* seq_out_)
      : dose(dose_), po(o), seed(seed_), stratum(stratum_), n_strata(n_strata_), h(h_), max_perms(max_perms_), seq_out(seq_out_),
        odds(odds_), max_attempts(max_attempts_) {}

  // the argument checks of gcre_seq_prefix.h, then the strata as the sequential stage reads them
  int check(gcre_ctx* c, const gcre_set_input* in, const std::string& who) override {
    who_ = who;
    std::string msg;
    const double max_mb = gcre_prefix::prefix_max_mb();
    if (dose) {
      if (int rc = gcre_seq_prefix::check_seq_dose_args(in, po.levels, po.n_levels, po.ds != nullptr, seq_out != nullptr, c->g.method,
                                                        2 * c->g.Wp, max_mb, h, max_perms, who, msg))
        return fail(c, rc, msg);
    } else {
      if (in->n_sets > 0x7fffffff || (in->n_sets > 0 && in->set_off[in->n_sets] > 0x7fffffff))
        return fail(c, GCRE_ERR_ARG, who + ": too many sets or members");
      gcre_prefix::prefix_steps(in, po.cut, st);
      if (int rc = gcre_seq_prefix::check_seq_prefix_args(in, st, po.px != nullptr, seq_out != nullptr, c->g.method, 2 * c->g.Wp, max_mb,
                                                          h, max_perms, who, msg))
        return fail(c, rc, msg);
    }
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
    const int64_t S = in->n_sets;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t s = 0; s < S; s++) {
      const int64_t v = out[s].valid ? 0 : -1;
      seq_out[s] = {v, v, 0, 0};
      if (dose) {
        gcre_dose_score& x = po.ds[s];
        std::memset(&x, 0, sizeof x);
        x.score = nan;
        x.n_ge = v;
        x.best_index = -1;
        x.levels = po.n_levels;
      } else {
        gcre_prefix_score& x = po.px[s];
        std::memset(&x, 0, sizeof x);
        x.score = nan;
        x.n_ge = v;
        x.best_step = -1;
        x.steps = (int32_t)(st.off[(size_t)s + 1] - st.off[(size_t)s]);
      }
    }
    if (dose && po.level_scores) std::fill(po.level_scores, po.level_scores + (size_t)S * (size_t)po.n_levels, nan);
    if (!dose && po.step_scores && S > 0) std::fill(po.step_scores, po.step_scores + (size_t)in->set_off[S], nan);
  }

  bool runs(const gcre_ctx*) const override { return max_perms > 0; }

  // The caller's gene rows and set list go up once.  Per slab of whole valid sets (gcre_prefix.h): k_prefix_rows or
  // k_dose_rows builds the step rows and their counts, k_set_observed scores them, k_prefix_pick takes every set's best step
  // and threshold; the picks come back (one synchronisation) and give the first active list; then the whole sequential loop
  // from permutation 0, with k_seq_prefix_null between the masks and the retirement.  No resident mask is read.
  void run(const SetScoreRun& r) override {
    gcre_ctx* c = r.c;
    DevScratch& d = r.d;
    const gcre_set_input* in = r.in;
    const std::vector<int64_t>& vset = r.vset;
    const Geometry& g = c->g;
    const int M = g.method;
    const int L = po.n_levels;
    const int W32p = 2 * g.Wp;
    const int64_t S = in->n_sets, V = (int64_t)vset.size(), TM = in->set_off[S];
    std::vector<int64_t> vsteps((size_t)V, (int64_t)L);
    for (int64_t v = 0; !dose && v < V; v++) vsteps[(size_t)v] = st.off[(size_t)vset[(size_t)v] + 1] - st.off[(size_t)vset[(size_t)v]];
    std::vector<gcre_prefix::PrefixSlab> slabs;
    gcre_prefix::prefix_slabs(vsteps, M, W32p, 0, false, gcre_prefix::prefix_max_mb(), gcre_prefix::prefix_slab_sets(), slabs);
    int64_t max_nv = 0, max_rows = 0;
    for (const auto& sl : slabs) {
      max_nv = std::max(max_nv, sl.nv);
      max_rows = std::max(max_rows, sl.steps);
    }
    const size_t rs = (size_t)M * (size_t)W32p;   // dwords per step row

    PrefixArgs a{};
    a.gene_rows = (const uint32_t*)d.put(in->rows, std::max<size_t>((size_t)in->n_rows * (size_t)g.W, 1));
    a.set_off = d.put(in->set_off, (size_t)S + 1);
    a.members = d.put(in->members, (size_t)TM);
    a.signs = M == 2 && in->signs ? d.put(in->signs, (size_t)TM) : nullptr;
    a.cut = !dose && po.cut ? d.put(po.cut, (size_t)TM) : nullptr;
    int64_t* d_which = d.take<int64_t>((size_t)max_nv);
    int64_t* d_row0 = d.take<int64_t>((size_t)max_nv + 1);
    a.rows = d.take<uint32_t>((size_t)max_rows * rs);
    a.cnt = d.take<int32_t>((size_t)max_rows * 4);
    double* d_obs = d.take<double>((size_t)max_rows);
    a.obs = d_obs;
    a.tot = d.take<uint32_t>((size_t)max_rows * M);
    a.thr = d.take<uint32_t>((size_t)max_nv);
    a.pick = d.take<PrefixPick>((size_t)max_nv);
    a.which = d_which;
    a.row0 = d_row0;
    a.W2 = 2 * g.W;
    a.W32p = W32p;
    a.n_patients = g.n;
    a.n_cases = g.n_cases;
    DoseArgs b{};
    if (dose) {
      b.gene_rows = a.gene_rows;
      b.set_off = a.set_off;
      b.members = a.members;
      b.signs = a.signs;
      b.which = d_which;
      b.rows = a.rows;
      b.cnt = a.cnt;
      b.levels = gcre_dose::pack_levels(po.levels, L);
      b.n_levels = L;
      b.W2 = a.W2;
      b.W32p = W32p;
      b.n_patients = g.n;
      b.n_cases = g.n_cases;
    }

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
      na.row0 = d_row0;
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
    std::vector<int64_t> which, row0;
    std::vector<PrefixPick> pick((size_t)max_nv);
    std::vector<double> obs((dose ? po.level_scores : po.step_scores) ? (size_t)max_rows : 0);
    std::vector<uint8_t> score_nan;
    std::vector<uint32_t> act;
    for (const auto& sl : slabs) {
      if (!d.ok()) break;
      which.assign(vset.begin() + sl.v0, vset.begin() + sl.v0 + sl.nv);
      row0.assign((size_t)sl.nv + 1, 0);
      for (int64_t e = 0; e < sl.nv; e++) row0[(size_t)e + 1] = row0[(size_t)e] + vsteps[(size_t)(sl.v0 + e)];
      a.nslots = b.nslots = sl.nv;
      a.nrows = sl.steps;
      d.upload(d_which, which.data(), (size_t)sl.nv);
      d.upload(d_row0, row0.data(), (size_t)sl.nv + 1);
      d.zero(a.cnt, (size_t)sl.steps * 4);
      if (d.ok()) {
        d.e = dose ? launch_dose_rows(b, M, c->stream) : launch_prefix_rows(a, M, c->stream);
        if (d.ok()) c->seq_prefix_launches++;
      }
      if (d.ok()) {
        d.e = launch_set_observed(a.cnt, sl.steps, M, c->d_dvt, d_obs, c->stream);
        if (d.ok()) c->seq_prefix_launches++;
      }
      if (d.ok()) {
        d.e = launch_prefix_pick(a, M, c->stream);
        if (d.ok()) c->seq_prefix_launches++;
      }
      d.download(pick.data(), a.pick, (size_t)sl.nv);
      if (!obs.empty()) d.download(obs.data(), d_obs, (size_t)sl.steps);
      d.sync();   // the picks give the first active list
      if (!d.ok()) break;
      score_nan.assign((size_t)sl.nv, 0);
      for (int64_t e = 0; e < sl.nv; e++) {
        const int64_t s = which[(size_t)e];
        const PrefixPick& p = pick[(size_t)e];
        score_nan[(size_t)e] = p.score != p.score;
        if (dose) {
          gcre_dose_score& x = po.ds[s];
          x.score = p.score;
          x.best_index = p.best_step;
          x.best_level = p.best_step >= 0 ? po.levels[p.best_step] : 0;
          x.cases_pos = p.cnt[0];
          x.ctrls_pos = p.cnt[1];
          x.cases_neg = p.cnt[2];
          x.ctrls_neg = p.cnt[3];
          if (po.level_scores)
            for (int k = 0; k < L; k++) po.level_scores[(size_t)s * (size_t)L + (size_t)k] = obs[(size_t)(row0[(size_t)e] + k)];
        } else {
          gcre_prefix_score& x = po.px[s];
          x.score = p.score;
          x.best_step = p.best_step;
          x.best_members = p.best_step >= 0 ? st.members[(size_t)(st.off[(size_t)s] + p.best_step)] : 0;
          x.cases_pos = p.cnt[0];
          x.ctrls_pos = p.cnt[1];
          x.cases_neg = p.cnt[2];
          x.ctrls_neg = p.cnt[3];
          if (po.step_scores)
            for (int64_t k = 0; k < vsteps[(size_t)(sl.v0 + e)]; k++)
              po.step_scores[st.end[(size_t)(st.off[(size_t)s] + k)]] = obs[(size_t)(row0[(size_t)e] + k)];
        }
      }
      gcre_seq_prefix::first_active(vsteps.data() + sl.v0, sl.nv, score_nan.data(), odds != nullptr, act);
      SeqLoopResult res;
      seq_batch_loop(c, d, dr, h, max_perms, sl.nv, act, null_launch, c->seq_prefix_launches, res);
      if (!d.ok()) break;
      totals.add(res.left_over, res.left_stratum, res.nact);
      if (res.refused) continue;   // every slab is run: the message sums the sets still active at R
      for (int64_t e = 0; e < sl.nv; e++) seq_fill(seq[(size_t)which[(size_t)e]], res.prior[(size_t)e], res.nperm[(size_t)e], h, max_perms);
    }
    if (!d.ok()) return;
    if (totals.refused()) {   // seq_out keeps its defaults; the entry refuses
      refusal = gcre_seq_weighted::seq_weighted_message(who_, totals.left_over, totals.left_stratum, wt_cap, totals.n_active, max_perms);
      return;
    }
    std::copy(seq.begin(), seq.end(), seq_out);
  }
};

int run_entry(gcre_ctx* c, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out, const std::string& who,
              SeqPrefixStage& st) {
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
  SeqPrefixStage st(false, {cut, px_out, step_scores, nullptr, 0, nullptr, nullptr}, seed, odds, stratum, n_strata, max_attempts, h,
                    max_perms, seq_out);
  return run_entry(c, in, out, cap, n_out, "score_sets_prefix_sequential", st);
}

// The same of the multi-hit test: the maximum over the level rows of every set
int gcre_score_sets_dose_sequential(gcre_ctx* c, const gcre_set_input* in, const int32_t* levels, int32_t n_levels, uint64_t seed,
                                    const double* odds, const int32_t* stratum, int n_strata, int64_t max_attempts, int64_t h,
                                    int64_t max_perms, gcre_set_score* out, int64_t cap, int64_t* n_out, gcre_dose_score* dose_out,
                                    gcre_seq_score* seq_out, double* level_scores) {
  SeqPrefixStage st(true, {nullptr, nullptr, nullptr, levels, n_levels, dose_out, level_scores}, seed, odds, stratum, n_strata,
                    max_attempts, h, max_perms, seq_out);
  return run_entry(c, in, out, cap, n_out, "score_sets_dose_sequential", st);
}

int64_t gcre_seq_prefix_launches(const gcre_ctx* c) { return c ? c->seq_prefix_launches : -1; }

}  // extern "C"

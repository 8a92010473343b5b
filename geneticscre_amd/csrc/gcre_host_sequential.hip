// gcre_host_sequential.hip -- gcre_score_sets_sequential on a context: the stage that score_sets_common
// (gcre_set_stage.h) runs behind the set scores.  The rule -- argument checks, strata, batch schedule -- is
// gcre_sequential.h's; here are the uploads, the batch loop over gcre_sequential.hip's kernels and the downloads.
// gcre_score_sets_sequential_weighted is the same stage with another mask step: the batch's masks come from
// gcre_seq_weighted.hip's two kernels, by the rule of gcre_seq_weighted.h, with one read-back between them.  Host code only.
#include "gcre_seq_loop.h"

namespace {

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

    std::vector<uint32_t> thr((size_t)V), act;
    for (int64_t v = 0; v < V; v++) {
      thr[(size_t)v] = f32_threshold(r.obs[(size_t)v]);
      // (weighted: a NaN score's threshold is past +inf, so the set counts nothing and never stops -- it stays active, and
      // with it the search for a left-over permutation runs to max_perms, as gcre_seq_weighted.h's rule asks)
      if (r.obs[(size_t)v] == r.obs[(size_t)v] || odds) act.push_back((uint32_t)v);
    }
    const uint32_t* d_thr = d.put(thr.data(), (size_t)V);
    const int64_t tpb = set_null_tile_sets(M);

    // the batch loop is gcre_seq_loop.h's; the null kernel of a batch is k_seq_null over the union rows
    const SeqNullLaunch null_launch = [&](const uint32_t* active, int64_t nact, const uint32_t* masks, int stride, int nb, int nkt,
                                          unsigned long long* bits) {
      SeqNullArgs na{};
      na.rows = (const uint32_t*)r.d_rows;
      na.masks = masks;
      na.tot = r.d_tot;
      na.thr = d_thr;
      na.t32 = c->d_t32;
      na.d64 = c->d_dmax;
      na.d64n = c->d_dmaxn ? c->d_dmaxn : c->d_dmax;
      na.active = active;
      na.bits = bits;
      na.nactive = nact;
      na.npt = (nact + tpb - 1) / tpb;
      na.W32p = W32p;
      na.stride = stride;
      na.K = nb;
      na.nkt = nkt;
      // one set tile per block while that makes at least ~8 blocks per resident block slot, more per block beyond (k_set_null's rule)
      const int64_t slots = (int64_t)c->cus * 4 * 8;
      const int64_t per = std::max<int64_t>(1, (na.npt * na.nkt) / slots);
      na.pgroups = (int)std::min<int64_t>((na.npt + per - 1) / per, 0x7fffffff / std::max(na.nkt, 1));
      return launch_seq_null(na, M, c->stream);
    };
    SeqDraw dr;
    dr.seed = seed;
    dr.stratum = stratum;
    dr.cases_in = &cases_in;
    dr.size_of = &size_of;
    dr.odds = odds;
    dr.wt_cap = wt_cap;
    dr.plan = &plan;
    SeqLoopResult res;
    seq_batch_loop(c, d, dr, h, max_perms, V, act, null_launch, c->sequential_launches, res);
    if (!d.ok()) return;
    if (res.refused) {   // seq_out keeps its defaults; the entry refuses
      refusal = gcre_seq_weighted::seq_weighted_message(who_, res.left_over, res.left_stratum, wt_cap, res.nact, max_perms);
      return;
    }
    for (int64_t v = 0; v < V; v++) seq_fill(seq_out[r.vset[(size_t)v]], res.prior[(size_t)v], res.nperm[(size_t)v], h, max_perms);
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

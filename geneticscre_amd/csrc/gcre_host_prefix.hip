// gcre_host_prefix.hip -- gcre_score_sets_prefix on a context: the stage that score_sets_common
// (gcre_set_stage.h) runs behind the set scores.  The plan -- steps, argument checks, slabs of whole sets, block table -- is
// gcre_prefix.h's; here are the uploads, the launches of gcre_prefix.hip's kernels and the downloads.  Host code only.
#include "gcre_set_stage.h"
#include "gcre_prefix.h"

namespace {

// What gcre_score_sets_prefix takes and returns beside the records
struct PrefixOut {
  const uint8_t* cut;       // [members of the list] or NULL
  gcre_prefix_score* px;    // [n_sets]
  float* family_max;        // optional [iterations]
  float* null_max;          // optional [n_sets][iterations]
  double* step_scores;      // optional [members of the list]
};
static_assert(sizeof(gcre_prefix::PrefixWave) == sizeof(PrefixWaveDev) && sizeof(PrefixWaveDev) == 16, "one layout");
static_assert(sizeof(PrefixPick) == 32, "the layout the host reads");

struct PrefixStage final : SetStage {
  const PrefixOut po;
  int K = 0;
  gcre_prefix::PrefixSteps st;   // the steps of every set
  explicit PrefixStage(const PrefixOut& o) : po(o) {}

  // the argument checks of gcre_prefix.h
  int check(gcre_ctx* c, const gcre_set_input* in, const std::string& who) override {
    K = c->g.K;
    if (in->n_sets > 0x7fffffff || (in->n_sets > 0 && in->set_off[in->n_sets] > 0x7fffffff))
      return fail(c, GCRE_ERR_ARG, who + ": too many sets or members");
    gcre_prefix::prefix_steps(in, po.cut, st);
    std::string msg;
    if (int rc = gcre_prefix::check_prefix_args(in, st, po.px != nullptr, K, c->g.method, 2 * c->g.Wp, c->g.Kpad,
                                                po.null_max != nullptr, gcre_prefix::prefix_max_mb(), who, msg))
      return fail(c, rc, msg);
    return GCRE_OK;
  }

  // an invalid set -1 and a NaN row; a NaN score and no best step without a permutation
  void defaults(const gcre_set_input* in, const gcre_set_score* out) override {
    const int64_t S = in->n_sets;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t s = 0; s < S; s++) {
      gcre_prefix_score& x = po.px[s];
      std::memset(&x, 0, sizeof x);
      x.score = nan;
      x.n_ge = out[s].valid ? 0 : -1;
      x.best_step = -1;
      x.steps = (int32_t)(st.off[(size_t)s + 1] - st.off[(size_t)s]);
    }
    if (po.family_max) std::fill(po.family_max, po.family_max + K, 0.0f);
    if (po.null_max) std::fill(po.null_max, po.null_max + (size_t)S * (size_t)K, std::numeric_limits<float>::quiet_NaN());
    if (po.step_scores && S > 0) std::fill(po.step_scores, po.step_scores + (size_t)in->set_off[S], nan);
  }

  bool runs(const gcre_ctx* c) const override { return c->g.K > 0; }

  // The caller's gene rows, set list and cut flags go up once; per slab of whole valid sets (gcre_prefix.h) k_prefix_rows
  // builds the step rows and their counts, k_set_observed scores them, k_prefix_pick takes every set's best step and threshold
  // and k_prefix_null the maxima over the steps under every permutation.  n_ge is an exact count per set and family_max a
  // maximum across the slabs, so no result depends on the slabs.
  void run(const SetScoreRun& r) override {
    gcre_ctx* c = r.c;
    DevScratch& d = r.d;
    const gcre_set_input* in = r.in;
    const std::vector<int64_t>& vset = r.vset;
    const Geometry& g = c->g;
    const int M = g.method;
    const int64_t S = in->n_sets, V = (int64_t)vset.size(), TM = in->set_off[S];
    std::vector<int64_t> vsteps((size_t)V);
    for (int64_t v = 0; v < V; v++) vsteps[(size_t)v] = st.off[(size_t)vset[(size_t)v] + 1] - st.off[(size_t)vset[(size_t)v]];
    std::vector<gcre_prefix::PrefixSlab> slabs;
    gcre_prefix::prefix_slabs(vsteps, M, 2 * g.Wp, g.Kpad, po.null_max != nullptr, gcre_prefix::prefix_max_mb(),
                              gcre_prefix::prefix_slab_sets(), slabs);
    int64_t max_nv = 0, max_rows = 0;
    for (const auto& sl : slabs) {
      max_nv = std::max(max_nv, sl.nv);
      max_rows = std::max(max_rows, sl.steps);
    }
    const int64_t max_waves = (max_nv + gcre_prefix::kPrefixBlockSets - 1) / gcre_prefix::kPrefixBlockSets * gcre_prefix::kPrefixBlockSets;
    const size_t rs = (size_t)M * 2 * g.Wp;   // dwords per step row
    const bool fam = po.family_max != nullptr;

    PrefixArgs a{};
    a.gene_rows = (const uint32_t*)d.put(in->rows, std::max<size_t>((size_t)in->n_rows * (size_t)g.W, 1));
    a.set_off = d.put(in->set_off, (size_t)S + 1);
    a.members = d.put(in->members, (size_t)TM);
    a.signs = M == 2 && in->signs ? d.put(in->signs, (size_t)TM) : nullptr;
    a.cut = po.cut ? d.put(po.cut, (size_t)TM) : nullptr;
    int64_t* d_which = d.take<int64_t>((size_t)max_nv);
    int64_t* d_row0 = d.take<int64_t>((size_t)max_nv + 1);
    PrefixWaveDev* d_waves = d.take<PrefixWaveDev>((size_t)max_waves);
    a.rows = d.take<uint32_t>((size_t)max_rows * rs);
    a.cnt = d.take<int32_t>((size_t)max_rows * 4);
    double* d_obs = d.take<double>((size_t)max_rows);
    a.obs = d_obs;
    a.tot = d.take<uint32_t>((size_t)max_rows * M);
    a.thr = d.take<uint32_t>((size_t)max_nv);
    a.pick = d.take<PrefixPick>((size_t)max_nv);
    a.n_ge = d.take<unsigned long long>((size_t)max_nv);
    a.null_max = po.null_max ? d.take<uint32_t>((size_t)max_nv * (size_t)g.Kpad) : nullptr;
    a.fam_bits = fam ? d.take<uint32_t>((size_t)g.Kpad) : nullptr;
    if (fam) d.zero(a.fam_bits, (size_t)g.Kpad);   // once: the maxima run over all slabs
    a.which = d_which;
    a.row0 = d_row0;
    a.waves = d_waves;
    a.masks = c->d_masks;
    a.t32 = c->d_t32;
    a.d64 = c->d_dmax;
    a.d64n = c->d_dmaxn ? c->d_dmaxn : c->d_dmax;
    a.W2 = 2 * g.W;
    a.W32p = 2 * g.Wp;
    a.Kpad = g.Kpad;
    a.K = K;
    a.nkt = (K + kSetPermTile - 1) / kSetPermTile;
    a.n_patients = g.n;
    a.n_cases = g.n_cases;

    std::vector<int64_t> which, row0;
    std::vector<int32_t> order;
    std::vector<gcre_prefix::PrefixWave> waves;
    std::vector<PrefixPick> pick((size_t)max_nv);
    std::vector<unsigned long long> ge((size_t)max_nv);
    std::vector<double> obs(po.step_scores ? (size_t)max_rows : 0);
    for (const auto& sl : slabs) {
      if (!d.ok()) break;
      which.assign(vset.begin() + sl.v0, vset.begin() + sl.v0 + sl.nv);
      row0.assign((size_t)sl.nv + 1, 0);
      for (int64_t e = 0; e < sl.nv; e++) row0[(size_t)e + 1] = row0[(size_t)e] + vsteps[(size_t)(sl.v0 + e)];
      gcre_prefix::prefix_blocks(vsteps.data() + sl.v0, sl.nv, order, waves);
      a.nslots = sl.nv;
      a.nrows = sl.steps;
      a.nblocks = (int)(waves.size() / gcre_prefix::kPrefixBlockSets);
      d.upload(d_which, which.data(), (size_t)sl.nv);
      d.upload(d_row0, row0.data(), (size_t)sl.nv + 1);
      d.upload(d_waves, (const PrefixWaveDev*)waves.data(), waves.size());
      d.zero(a.cnt, (size_t)sl.steps * 4);
      d.zero(a.n_ge, (size_t)sl.nv);
      if (d.ok()) {
        d.e = launch_prefix_rows(a, M, c->stream);
        if (d.ok()) c->prefix_launches++;
      }
      if (d.ok()) {
        d.e = launch_set_observed(a.cnt, sl.steps, M, c->d_dvt, d_obs, c->stream);
        if (d.ok()) c->prefix_launches++;
      }
      if (d.ok()) {
        d.e = launch_prefix_pick(a, M, c->stream);
        if (d.ok()) c->prefix_launches++;
      }
      if (d.ok()) {
        d.e = launch_prefix_null(a, M, c->stream);
        if (d.ok()) c->prefix_launches++;
      }
      d.download(pick.data(), a.pick, (size_t)sl.nv);
      d.download(ge.data(), a.n_ge, (size_t)sl.nv);
      if (po.step_scores) d.download(obs.data(), d_obs, (size_t)sl.steps);
      for (int64_t e = 0; po.null_max && e < sl.nv; e++)   // a row at a time, straight into the caller's matrix
        d.download((uint32_t*)po.null_max + (size_t)which[(size_t)e] * (size_t)K, a.null_max + (size_t)e * (size_t)g.Kpad, (size_t)K);
      d.sync();   // (the host arrays above are reused by the next slab)
      if (!d.ok()) break;
      for (int64_t e = 0; e < sl.nv; e++) {
        const int64_t s = which[(size_t)e];
        const PrefixPick& p = pick[(size_t)e];
        gcre_prefix_score& x = po.px[s];
        x.score = p.score;
        x.n_ge = (int64_t)ge[(size_t)e];
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
    if (fam && d.ok()) {
      d.download((uint32_t*)po.family_max, a.fam_bits, (size_t)K);
      d.sync();
    }
  }
};

}  // namespace

extern "C" {

// Variable-threshold tests of the given sets: gcre_score_sets on the full sets, then the step rows of every set built on the
// device and the maximum over them under every permutation.
int gcre_score_sets_prefix(gcre_ctx* c, const gcre_set_input* in, const uint8_t* cut, gcre_set_score* out, int64_t cap, int64_t* n_out,
                           gcre_prefix_score* px_out, float* family_max, float* null_max, double* step_scores) {
  PrefixStage st({cut, px_out, family_max, null_max, step_scores});
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_prefix", &st);
}

int64_t gcre_prefix_launches(const gcre_ctx* c) { return c ? c->prefix_launches : -1; }

}  // extern "C"

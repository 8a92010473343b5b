// gcre_host_dose.hip -- gcre_score_sets_dose on a context: the stage that score_sets_common
// (gcre_set_stage.h) runs behind the set scores.  The argument checks are gcre_dose.h's, the slabs of whole sets and the block
// table gcre_prefix.h's; here are the uploads, the launches -- k_dose_rows (gcre_dose.hip), then the prefix stage's own
// kernels on the rows it wrote -- and the downloads.  Host code only.
#include "gcre_set_stage.h"
#include "gcre_dose.h"

namespace {

// What gcre_score_sets_dose takes and returns beside the records
struct DoseOut {
  const int32_t* levels;    // [n_levels]
  int32_t n_levels;
  gcre_dose_score* ds;      // [n_sets]
  float* family_max;        // optional [iterations]
  float* null_max;          // optional [n_sets][iterations]
  double* level_scores;     // optional [n_sets][n_levels]
};
static_assert(sizeof(gcre_prefix::PrefixWave) == sizeof(PrefixWaveDev) && sizeof(PrefixWaveDev) == 16, "one layout");
static_assert(sizeof(PrefixPick) == 32, "the layout the host reads");
static_assert(sizeof(gcre_dose_score) == 48, "the ABI");

struct DoseStage final : SetStage {
  const DoseOut po;
  int K = 0;
  explicit DoseStage(const DoseOut& o) : po(o) {}

  // the argument checks of gcre_dose.h
  int check(gcre_ctx* c, const gcre_set_input* in, const std::string& who) override {
    K = c->g.K;
    std::string msg;
    if (int rc = gcre_dose::check_dose_args(in, po.levels, po.n_levels, po.ds != nullptr, K, c->g.method, 2 * c->g.Wp, c->g.Kpad,
                                            po.null_max != nullptr, gcre_prefix::prefix_max_mb(), who, msg))
      return fail(c, rc, msg);
    return GCRE_OK;
  }

  // an invalid set -1 and a NaN row; a NaN score and no best level without a permutation
  void defaults(const gcre_set_input* in, const gcre_set_score* out) override {
    const int64_t S = in->n_sets;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t s = 0; s < S; s++) {
      gcre_dose_score& x = po.ds[s];
      std::memset(&x, 0, sizeof x);
      x.score = nan;
      x.n_ge = out[s].valid ? 0 : -1;
      x.best_index = -1;
      x.levels = po.n_levels;
    }
    if (po.family_max) std::fill(po.family_max, po.family_max + K, 0.0f);
    if (po.null_max) std::fill(po.null_max, po.null_max + (size_t)S * (size_t)K, std::numeric_limits<float>::quiet_NaN());
    if (po.level_scores) std::fill(po.level_scores, po.level_scores + (size_t)S * (size_t)po.n_levels, nan);
  }

  bool runs(const gcre_ctx* c) const override { return c->g.K > 0; }

  // The caller's gene rows and set list go up once; per slab of whole valid sets (gcre_prefix.h) k_dose_rows builds the level
  // rows and their counts, k_set_observed scores them, k_prefix_pick takes every set's best level and threshold and
  // k_prefix_null the maxima over the levels under every permutation.  n_ge is an exact count per set and family_max a
  // maximum across the slabs, so no result depends on the slabs.
  void run(const SetScoreRun& r) override {
    gcre_ctx* c = r.c;
    DevScratch& d = r.d;
    const gcre_set_input* in = r.in;
    const std::vector<int64_t>& vset = r.vset;
    const Geometry& g = c->g;
    const int M = g.method;
    const int L = po.n_levels;
    const int64_t S = in->n_sets, V = (int64_t)vset.size(), TM = in->set_off[S];
    const std::vector<int64_t> vsteps((size_t)V, (int64_t)L);
    std::vector<gcre_prefix::PrefixSlab> slabs;
    gcre_prefix::prefix_slabs(vsteps, M, 2 * g.Wp, g.Kpad, po.null_max != nullptr, gcre_prefix::prefix_max_mb(),
                              gcre_prefix::prefix_slab_sets(), slabs);
    int64_t max_nv = 0, max_rows = 0;
    for (const auto& sl : slabs) {
      max_nv = std::max(max_nv, sl.nv);
      max_rows = std::max(max_rows, sl.steps);
    }
    const int64_t max_waves = (max_nv + gcre_prefix::kPrefixBlockSets - 1) / gcre_prefix::kPrefixBlockSets * gcre_prefix::kPrefixBlockSets;
    const size_t rs = (size_t)M * 2 * g.Wp;   // dwords per level row
    const bool fam = po.family_max != nullptr;

    DoseArgs b{};
    b.gene_rows = (const uint32_t*)d.put(in->rows, std::max<size_t>((size_t)in->n_rows * (size_t)g.W, 1));
    b.set_off = d.put(in->set_off, (size_t)S + 1);
    b.members = d.put(in->members, (size_t)TM);
    b.signs = M == 2 && in->signs ? d.put(in->signs, (size_t)TM) : nullptr;
    int64_t* d_which = d.take<int64_t>((size_t)max_nv);
    int64_t* d_row0 = d.take<int64_t>((size_t)max_nv + 1);
    PrefixWaveDev* d_waves = d.take<PrefixWaveDev>((size_t)max_waves);
    PrefixArgs a{};
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
    b.which = d_which;
    b.rows = a.rows;
    b.cnt = a.cnt;
    b.levels = gcre_dose::pack_levels(po.levels, L);
    b.n_levels = L;
    b.W2 = a.W2;
    b.W32p = a.W32p;
    b.n_patients = g.n;
    b.n_cases = g.n_cases;

    std::vector<int64_t> which, row0;
    std::vector<int32_t> order;
    std::vector<gcre_prefix::PrefixWave> waves;
    std::vector<PrefixPick> pick((size_t)max_nv);
    std::vector<unsigned long long> ge((size_t)max_nv);
    std::vector<double> obs(po.level_scores ? (size_t)max_rows : 0);
    for (const auto& sl : slabs) {
      if (!d.ok()) break;
      which.assign(vset.begin() + sl.v0, vset.begin() + sl.v0 + sl.nv);
      row0.assign((size_t)sl.nv + 1, 0);
      for (int64_t e = 0; e < sl.nv; e++) row0[(size_t)e + 1] = row0[(size_t)e] + L;   // slot e: rows [e L, e L + L), as k_dose_rows writes them
      gcre_prefix::prefix_blocks(vsteps.data() + sl.v0, sl.nv, order, waves);
      a.nslots = b.nslots = sl.nv;
      a.nrows = sl.steps;
      a.nblocks = (int)(waves.size() / gcre_prefix::kPrefixBlockSets);
      d.upload(d_which, which.data(), (size_t)sl.nv);
      d.upload(d_row0, row0.data(), (size_t)sl.nv + 1);
      d.upload(d_waves, (const PrefixWaveDev*)waves.data(), waves.size());
      d.zero(a.cnt, (size_t)sl.steps * 4);
      d.zero(a.n_ge, (size_t)sl.nv);
      if (d.ok()) {
        d.e = launch_dose_rows(b, M, c->stream);
        if (d.ok()) c->dose_launches++;
      }
      if (d.ok()) {
        d.e = launch_set_observed(a.cnt, sl.steps, M, c->d_dvt, d_obs, c->stream);
        if (d.ok()) c->dose_launches++;
      }
      if (d.ok()) {
        d.e = launch_prefix_pick(a, M, c->stream);
        if (d.ok()) c->dose_launches++;
      }
      if (d.ok()) {
        d.e = launch_prefix_null(a, M, c->stream);
        if (d.ok()) c->dose_launches++;
      }
      d.download(pick.data(), a.pick, (size_t)sl.nv);
      d.download(ge.data(), a.n_ge, (size_t)sl.nv);
      if (po.level_scores) d.download(obs.data(), d_obs, (size_t)sl.steps);
      for (int64_t e = 0; po.null_max && e < sl.nv; e++)   // a row at a time, straight into the caller's matrix
        d.download((uint32_t*)po.null_max + (size_t)which[(size_t)e] * (size_t)K, a.null_max + (size_t)e * (size_t)g.Kpad, (size_t)K);
      d.sync();   // (the host arrays above are reused by the next slab)
      if (!d.ok()) break;
      for (int64_t e = 0; e < sl.nv; e++) {
        const int64_t s = which[(size_t)e];
        const PrefixPick& p = pick[(size_t)e];
        gcre_dose_score& x = po.ds[s];
        x.score = p.score;
        x.n_ge = (int64_t)ge[(size_t)e];
        x.best_index = p.best_step;
        x.best_level = p.best_step >= 0 ? po.levels[p.best_step] : 0;
        x.cases_pos = p.cnt[0];
        x.ctrls_pos = p.cnt[1];
        x.cases_neg = p.cnt[2];
        x.ctrls_neg = p.cnt[3];
        if (po.level_scores)
          for (int k = 0; k < L; k++) po.level_scores[(size_t)s * (size_t)L + (size_t)k] = obs[(size_t)(row0[(size_t)e] + k)];
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

// Multi-hit tests of the given sets: gcre_score_sets on the full sets, then the level rows of every set built on the device
// and the maximum over them under every permutation.
int gcre_score_sets_dose(gcre_ctx* c, const gcre_set_input* in, const int32_t* levels, int32_t n_levels, gcre_set_score* out,
                         int64_t cap, int64_t* n_out, gcre_dose_score* dose_out, float* family_max, float* null_max,
                         double* level_scores) {
  DoseStage st({levels, n_levels, dose_out, family_max, null_max, level_scores});
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_dose", &st);
}

int64_t gcre_dose_launches(const gcre_ctx* c) { return c ? c->dose_launches : -1; }

}  // extern "C"

// gcre_host_steps.hip -- gcre_score_sets_prefix and gcre_score_sets_dose (§3.20) on a context: the one stage
// that score_sets_common (gcre_set_stage.h) runs behind the set scores for both.  The plans -- steps, argument checks, slabs
// of whole sets, block table -- are gcre_prefix.h's and gcre_dose.h's, the two row variants gcre_steps.h's, the step rows and
// their picks StepRows' (gcre_step_rows.h); here are the block table, k_prefix_null and the downloads of what it counts.
// Host code only.
#include "gcre_step_rows.h"

namespace {

static_assert(sizeof(gcre_prefix::PrefixWave) == sizeof(PrefixWaveDev) && sizeof(PrefixWaveDev) == 16, "one layout");
static_assert(sizeof(gcre_dose_score) == 48, "the ABI");

template <typename Variant>
struct StepStage final : SetStage {
  Variant v;                 // what the entry takes and returns beside the records
  float* const family_max;   // optional [iterations]
  float* const null_max;     // optional [n_sets][iterations]
  int64_t gcre_ctx::*const counter;   // the entry's own launches
  int K = 0;
  StepStage(const Variant& v_, float* family_max_, float* null_max_, int64_t gcre_ctx::*counter_)
      : v(v_), family_max(family_max_), null_max(null_max_), counter(counter_) {}

  // the argument checks of the variant's plan
  int check(gcre_ctx* c, const gcre_set_input* in, const std::string& who) override {
    K = c->g.K;
    std::string msg;
    if (int rc = v.check(in, K, c->g.method, 2 * c->g.Wp, c->g.Kpad, null_max != nullptr, gcre_prefix::prefix_max_mb(), who, msg))
      return fail(c, rc, msg);
    return GCRE_OK;
  }

  // an invalid set -1 and a NaN row; a NaN score and no best step without a permutation
  void defaults(const gcre_set_input* in, const gcre_set_score* out) override {
    v.defaults(in, out);
    if (family_max) std::fill(family_max, family_max + K, 0.0f);
    if (null_max) std::fill(null_max, null_max + (size_t)in->n_sets * (size_t)K, std::numeric_limits<float>::quiet_NaN());
  }

  bool runs(const gcre_ctx* c) const override { return c->g.K > 0; }

  // Per slab of whole valid sets StepRows builds the step (or level) rows, scores them and takes every set's best step and
  // threshold; k_prefix_null then takes the maxima over the steps under every permutation.  n_ge is an exact count per set
  // and family_max a maximum across the slabs, so no result depends on the slabs.
  void run(const SetScoreRun& r) override {
    gcre_ctx* c = r.c;
    DevScratch& d = r.d;
    const Geometry& g = c->g;
    const int M = g.method;
    int64_t& launches = c->*counter;
    StepRows<Variant> rows(v, r);
    rows.plan(null_max != nullptr, g.Kpad);
    rows.upload(r.in);
    const int64_t max_nv = rows.max_nv;
    const int64_t max_waves = (max_nv + gcre_prefix::kPrefixBlockSets - 1) / gcre_prefix::kPrefixBlockSets * gcre_prefix::kPrefixBlockSets;
    PrefixArgs& a = rows.a;
    PrefixWaveDev* d_waves = d.take<PrefixWaveDev>((size_t)max_waves);
    a.n_ge = d.take<unsigned long long>((size_t)max_nv);
    a.null_max = null_max ? d.take<uint32_t>((size_t)max_nv * (size_t)g.Kpad) : nullptr;
    a.fam_bits = family_max ? d.take<uint32_t>((size_t)g.Kpad) : nullptr;
    if (family_max) d.zero(a.fam_bits, (size_t)g.Kpad);   // once: the maxima run over all slabs
    a.waves = d_waves;
    a.masks = c->d_masks;
    a.t32 = c->d_t32;
    a.d64 = c->d_dmax;
    a.d64n = c->d_dmaxn ? c->d_dmaxn : c->d_dmax;
    a.Kpad = g.Kpad;
    a.K = K;
    a.nkt = (K + kSetPermTile - 1) / kSetPermTile;

    std::vector<int32_t> order;
    std::vector<gcre_prefix::PrefixWave> waves;
    std::vector<unsigned long long> ge((size_t)max_nv);
    for (const auto& sl : rows.slabs) {
      if (!d.ok()) break;
      gcre_prefix::prefix_blocks(rows.vsteps.data() + sl.v0, sl.nv, order, waves);
      a.nblocks = (int)(waves.size() / gcre_prefix::kPrefixBlockSets);
      d.upload(d_waves, (const PrefixWaveDev*)waves.data(), waves.size());
      d.zero(a.n_ge, (size_t)sl.nv);
      rows.build(sl, launches);
      rows.launch(launches, [&] { return launch_prefix_null(a, M, c->stream); });
      rows.fetch(sl);
      d.download(ge.data(), a.n_ge, (size_t)sl.nv);
      for (int64_t e = 0; null_max && e < sl.nv; e++)   // a row at a time, straight into the caller's matrix
        d.download((uint32_t*)null_max + (size_t)rows.which[(size_t)e] * (size_t)K, a.null_max + (size_t)e * (size_t)g.Kpad, (size_t)K);
      d.sync();   // (the host arrays above are reused by the next slab)
      if (!d.ok()) break;
      rows.collect(sl);
      for (int64_t e = 0; e < sl.nv; e++) v.rec[rows.which[(size_t)e]].n_ge = (int64_t)ge[(size_t)e];
    }
    if (family_max && d.ok()) {
      d.download((uint32_t*)family_max, a.fam_bits, (size_t)K);
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
  StepStage<gcre_steps::PrefixRows> st({cut, px_out, step_scores}, family_max, null_max, &gcre_ctx::prefix_launches);
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_prefix", &st);
}

// Multi-hit tests of the given sets: the same over the level rows of every set
int gcre_score_sets_dose(gcre_ctx* c, const gcre_set_input* in, const int32_t* levels, int32_t n_levels, gcre_set_score* out,
                         int64_t cap, int64_t* n_out, gcre_dose_score* dose_out, float* family_max, float* null_max,
                         double* level_scores) {
  StepStage<gcre_steps::DoseRows> st({levels, n_levels, dose_out, level_scores}, family_max, null_max, &gcre_ctx::dose_launches);
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_dose", &st);
}

int64_t gcre_prefix_launches(const gcre_ctx* c) { return c ? c->prefix_launches : -1; }
int64_t gcre_dose_launches(const gcre_ctx* c) { return c ? c->dose_launches : -1; }

}  // extern "C"

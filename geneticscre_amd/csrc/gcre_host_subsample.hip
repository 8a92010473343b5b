// gcre_host_subsample.hip -- gcre_score_sets_subsample on a context: the stage that score_sets_common
// (gcre_set_stage.h) runs behind the set scores.  The plan -- argument checks, draw rule, slab of draws -- is
// gcre_subsample.h's; here are the uploads, the launches of gcre_subsample.hip's kernels and the downloads.  Host code only.
#include "gcre_set_stage.h"
#include "gcre_subsample.h"

namespace {

// What gcre_score_sets_subsample takes and returns beside the records
struct SubsampleOut {
  int32_t m_cases, m_ctrls;
  int64_t draws;
  uint64_t seed;
  const double* table_a;    // [nrow_a][ncol_a]
  int nrow_a, ncol_a;
  const double* table_b;    // [nrow_b][ncol_b] or NULL
  int nrow_b, ncol_b;
  const double* cut;        // [n_sets][n_cut] or NULL
  int32_t n_cut;
  int64_t* n_a;             // [n_sets][n_cut]
  int64_t* n_b;             // optional, with table_b
  int64_t* n_both;          // optional, with table_b
  double* scores_a;         // optional [n_sets][draws]
  double* scores_b;         // optional, with table_b
};

struct SubsampleStage final : SetStage {
  const SubsampleOut so;
  explicit SubsampleStage(const SubsampleOut& o) : so(o) {}

  gcre_subsample::SubsampleAsk ask(const gcre_ctx* c) const {
    return {c->g.n_cases, c->g.n - c->g.n_cases, so.m_cases, so.m_ctrls, so.draws, so.table_a != nullptr, so.nrow_a, so.ncol_a,
            so.table_b != nullptr, so.nrow_b, so.ncol_b, so.cut, so.n_cut, so.n_a != nullptr, so.n_b != nullptr, so.n_both != nullptr,
            so.scores_a != nullptr, so.scores_b != nullptr};
  }

  // the argument checks of gcre_subsample.h, and what the device's 32-bit indices add
  int check(gcre_ctx* c, const gcre_set_input* in, const std::string& who) override {
    std::string msg;
    if (int rc = gcre_subsample::check_subsample_args(in, ask(c), gcre_subsample::subsample_max_mb(), who, msg)) return fail(c, rc, msg);
    if (in->n_sets > 0x7fffffff / (2 * GCRE_SUBSAMPLE_MAX_CUTS)) return fail(c, GCRE_ERR_ARG, who + ": too many sets");
    return GCRE_OK;
  }

  // an invalid set -1 and NaN rows; zeros without a draw
  void defaults(const gcre_set_input* in, const gcre_set_score* out) override {
    const int64_t S = in->n_sets;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t s = 0; s < S; s++)
      for (int32_t j = 0; j < so.n_cut; j++) {
        const size_t at = (size_t)s * so.n_cut + j;
        so.n_a[at] = out[s].valid ? 0 : -1;
        if (so.n_b) so.n_b[at] = so.n_a[at];
        if (so.n_both) so.n_both[at] = so.n_a[at];
      }
    if (so.scores_a) std::fill(so.scores_a, so.scores_a + (size_t)S * (size_t)so.draws, nan);
    if (so.scores_b) std::fill(so.scores_b, so.scores_b + (size_t)S * (size_t)so.draws, nan);
  }

  bool runs(const gcre_ctx*) const override { return so.draws > 0; }

  // The valid sets' union rows are on the device as k_set_null reads them, cnt [V][4] their counts as SetUnion::build gives
  // them.  The two tables go up as they are and become diagonal-major on the device (k_table_to_diag, sized for the half
  // cohorts); then, per slab of whole draw tiles, k_subsample_masks and k_subsample_null.  The counts are exact sums and every
  // draw belongs to one slab, so no result depends on the slabs.
  void run(const SetScoreRun& r) override {
    gcre_ctx* c = r.c;
    DevScratch& d = r.d;
    const std::vector<int64_t>& vset = r.vset;
    const Geometry& g = c->g;
    const int M = g.method, n_cut = so.n_cut;
    const int64_t V = (int64_t)vset.size(), B = so.draws;
    const int nA = so.m_cases + so.m_ctrls, nB = g.n - nA;
    const bool have_b = so.table_b != nullptr;

    // the carriers of every half-row among the cases and among the controls (the (-) half is counted the other way round)
    std::vector<uint32_t> tot((size_t)V * 2 * M);
    for (int64_t v = 0; v < V; v++) {
      const int32_t* k = r.cnt.data() + 4 * v;
      tot[(size_t)v * 2 * M] = (uint32_t)k[0];
      tot[(size_t)v * 2 * M + 1] = (uint32_t)k[1];
      if (M == 2) {
        tot[(size_t)v * 4 + 2] = (uint32_t)k[3];
        tot[(size_t)v * 4 + 3] = (uint32_t)k[2];
      }
    }
    std::vector<double> cuts((size_t)V * std::max(n_cut, 1), 0.0);
    for (int64_t v = 0; v < V && n_cut > 0; v++)
      std::memcpy(cuts.data() + (size_t)v * n_cut, so.cut + (size_t)vset[(size_t)v] * n_cut, (size_t)n_cut * 8);

    auto diag_table = [&](const double* table, int nrow, int ncol, int n_half) -> double* {
      const size_t TD = (size_t)n_half + 1;
      const double* d_raw = d.put(table, (size_t)nrow * (size_t)ncol);
      double* dvt = d.take<double>(TD * (TD + 1) / 2);
      if (d.ok()) {
        d.e = launch_table_to_diag(d_raw, nrow, ncol, 0, n_half, (int)TD, dvt, nullptr, nullptr, nullptr, c->stream);
        if (d.ok()) c->subsample_launches++;
      }
      return dvt;
    };
    SubsampleArgs a{};
    a.dvt_a = diag_table(so.table_a, so.nrow_a, so.ncol_a, nA);
    a.dvt_b = have_b ? diag_table(so.table_b, so.nrow_b, so.ncol_b, nB) : nullptr;
    a.rows = (const uint32_t*)r.d_rows;
    a.tot = d.put(tot.data(), tot.size());
    a.cut = n_cut > 0 ? d.put(cuts.data(), cuts.size()) : nullptr;
    const size_t NC = (size_t)V * (size_t)std::max(n_cut, 1);
    a.n_a = d.take<unsigned long long>(NC);
    a.n_b = have_b ? d.take<unsigned long long>(NC) : nullptr;
    a.n_both = have_b ? d.take<unsigned long long>(NC) : nullptr;
    d.zero(a.n_a, NC);
    if (have_b) {
      d.zero(a.n_b, NC);
      d.zero(a.n_both, NC);
    }
    a.nsets = V;
    a.W32p = 2 * g.Wp;
    a.n_cases = g.n_cases;
    a.n_cut = n_cut;
    const int64_t tpb = set_null_tile_sets(M);
    a.npt = (V + tpb - 1) / tpb;

    const double per_draw = gcre_subsample::subsample_draw_bytes(r.in, ask(c));
    int64_t slab = gcre_subsample::subsample_slab_draws(B, a.W32p, per_draw, gcre_subsample::subsample_max_mb());
    slab = std::min<int64_t>(slab, (int64_t)1 << 30);   // the 32-bit draw index of a slab
    a.Kpad = (int)slab;
    a.stride = slab;
    uint32_t* d_masks = d.take<uint32_t>((size_t)a.W32p * (size_t)slab);
    a.masks = d_masks;
    a.scores_a = so.scores_a ? d.take<double>((size_t)V * (size_t)slab) : nullptr;
    a.scores_b = so.scores_b ? d.take<double>((size_t)V * (size_t)slab) : nullptr;
    std::vector<double> stage;
    const uint64_t seed1 = gcre_subsample::subsample_seed(so.seed);
    for (int64_t b0 = 0; d.ok() && b0 < B; b0 += slab) {
      const int64_t nb = std::min(slab, B - b0);
      a.K = (int)nb;
      a.nkt = (int)((nb + kSetPermTile - 1) / kSetPermTile);
      // one set tile per block while that makes at least ~8 blocks per resident block slot, more per block beyond (k_set_null's rule)
      const int64_t slots = (int64_t)c->cus * 4 * 8;
      const int64_t per = std::max<int64_t>(1, (a.npt * a.nkt) / slots);
      a.pgroups = (int)std::min<int64_t>((a.npt + per - 1) / per, 0x7fffffff / std::max(a.nkt, 1));
      d.e = launch_subsample_masks(seed1, b0, (int)nb, g.n_cases, g.n - g.n_cases, so.m_cases, so.m_ctrls, a.W32p, a.Kpad, d_masks, c->stream);
      if (d.ok()) c->subsample_launches++;
      if (d.ok()) {
        d.e = launch_subsample_null(a, M, c->stream);
        if (d.ok()) c->subsample_launches++;
      }
      for (int half = 0; half < 2; half++) {   // each half's slab of scores at once
        const double* d_sc = half == 0 ? a.scores_a : a.scores_b;
        if (d_sc)
          fetch_rows(d, d_sc, V, slab, V, stage, half == 0 ? so.scores_a : so.scores_b, B, b0, nb, [&](int64_t v) { return vset[(size_t)v]; });
      }
    }
    std::vector<unsigned long long> na(NC), nbv(have_b ? NC : 0), nab(have_b ? NC : 0);
    d.download(na.data(), a.n_a, NC);
    if (have_b) {
      d.download(nbv.data(), a.n_b, NC);
      d.download(nab.data(), a.n_both, NC);
    }
    d.sync();
    if (!d.ok()) return;
    for (int64_t v = 0; v < V; v++)
      for (int j = 0; j < n_cut; j++) {
        const size_t to = (size_t)vset[(size_t)v] * n_cut + j, from = (size_t)v * n_cut + j;
        so.n_a[to] = (int64_t)na[from];
        if (so.n_b) so.n_b[to] = (int64_t)nbv[from];
        if (so.n_both) so.n_both[to] = (int64_t)nab[from];
      }
  }
};

}  // namespace

extern "C" {

// Split-half stability of the given sets: gcre_score_sets, then the same device rows scored on random halves of the cohort
// and on their complements.
int gcre_score_sets_subsample(gcre_ctx* c, const gcre_set_input* in, int32_t m_cases, int32_t m_ctrls, int64_t draws, uint64_t seed,
                              const double* table_a, int nrow_a, int ncol_a, const double* table_b, int nrow_b, int ncol_b,
                              const double* cut, int32_t n_cut, gcre_set_score* out, int64_t cap, int64_t* n_out, int64_t* n_a,
                              int64_t* n_b, int64_t* n_both, double* scores_a, double* scores_b) {
  SubsampleStage st({m_cases, m_ctrls, draws, seed, table_a, nrow_a, ncol_a, table_b, nrow_b, ncol_b, cut, n_cut,
                     n_a, n_b, n_both, scores_a, scores_b});
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_subsample", &st);
}

int64_t gcre_subsample_launches(const gcre_ctx* c) { return c ? c->subsample_launches : -1; }

}  // extern "C"

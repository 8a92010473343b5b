// gcre_host_strata.hip -- gcre_score_sets_strata on a context: the stage that score_sets_common
// (gcre_set_stage.h) runs behind the set scores.  The plan -- stratum counts, argument checks, table offsets, slabs of whole
// sets -- is gcre_strata.h's, the block table gcre_prefix.h's; here are the uploads, the launches of gcre_strata.hip's kernels
// and the downloads.  Host code only.
#include "gcre_set_stage.h"
#include "gcre_prefix.h"
#include "gcre_strata.h"

namespace {

// What gcre_score_sets_strata takes and returns beside the records
struct StrataOut {
  const int32_t* stratum;   // [n]
  int32_t n_strata;
  const double* tables;     // the raw tables, table s at tab_off[s], nrow[s] x ncol[s]
  const int32_t* nrow;
  const int32_t* ncol;
  const int64_t* tab_off;
  gcre_strata_score* px;    // [n_sets]
  double* terms;            // optional [n_sets][n_strata]
  int32_t* counts;          // optional [n_sets][n_strata][4]
  double* null_scores;      // optional [n_sets][iterations]
  double* family_max;       // optional [iterations]
};
static_assert(sizeof(gcre_prefix::PrefixWave) == sizeof(PrefixWaveDev), "one layout");
static_assert(sizeof(gcre_strata_score) == 16, "the layout the header promises");

struct StrataStage final : SetStage {
  const StrataOut so;
  int K = 0;
  std::vector<uint32_t> cases_in, size_of;   // per stratum
  long long violations = 0;                  // > 0: the masks do not keep the strata (the entry refuses)
  std::string who_;
  explicit StrataStage(const StrataOut& o) : so(o) {}

  // the argument checks of gcre_strata.h
  int check(gcre_ctx* c, const gcre_set_input* in, const std::string& who) override {
    K = c->g.K;
    who_ = who;
    const gcre_strata::StrataAsk q{c->g.n, c->g.n_cases, K, c->g.Kpad, so.stratum, so.n_strata, so.tables != nullptr, so.nrow, so.ncol,
                                   so.tab_off, so.px != nullptr, so.null_scores != nullptr, so.family_max != nullptr};
    std::string msg;
    if (int rc = gcre_strata::check_strata_args(in, q, gcre_strata::strata_max_mb(), who, cases_in, size_of, msg)) return fail(c, rc, msg);
    return GCRE_OK;
  }

  // an invalid set -1, NaN scores and rows, zero counts; +0 maxima
  void defaults(const gcre_set_input* in, const gcre_set_score* out) override {
    const int64_t S = in->n_sets;
    const size_t NS = (size_t)so.n_strata;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t s = 0; s < S; s++) {
      so.px[s].score = nan;
      so.px[s].n_ge = out[s].valid ? 0 : -1;
    }
    if (so.terms) std::fill(so.terms, so.terms + (size_t)S * NS, nan);
    if (so.counts) std::fill(so.counts, so.counts + (size_t)S * NS * 4, 0);
    if (so.null_scores) std::fill(so.null_scores, so.null_scores + (size_t)S * (size_t)K, nan);
    if (so.family_max) std::fill(so.family_max, so.family_max + K, 0.0);
  }

  // (without permutations the observed terms are still made)
  bool runs(const gcre_ctx*) const override { return true; }

  // The valid sets' union rows are on the device as k_set_null reads them.  The ids become indicator rows and, with
  // permutations, every resident mask is counted against them: one violation and nothing else runs.  The S tables go up as
  // they are and become diagonal-major on the device (k_table_to_diag, sized for the stratum), one behind the other.  Then,
  // per slab of whole valid sets, k_strata_rows, k_strata_observed and k_strata_null.  n_ge is an exact count per set and
  // family_max a maximum across the slabs, so no result depends on the slabs.
  void run(const SetScoreRun& r) override {
    gcre_ctx* c = r.c;
    DevScratch& d = r.d;
    const std::vector<int64_t>& vset = r.vset;
    const Geometry& g = c->g;
    const int M = g.method, NS = so.n_strata;
    const int64_t V = (int64_t)vset.size();
    const size_t urs = (size_t)M * 2 * g.Wp;   // dwords per union row, and per stratum row
    const bool fam = so.family_max != nullptr && K > 0;
    const bool want_null = so.null_scores != nullptr && K > 0;

    StrataArgs a{};
    a.S = NS;
    a.W32p = 2 * g.Wp;
    a.Kpad = g.Kpad;
    a.K = K;
    a.nkt = (K + kSetPermTile - 1) / kSetPermTile;
    a.n_patients = g.n;
    a.n_cases = g.n_cases;
    a.masks = c->d_masks;
    a.stratum = d.put(so.stratum, (size_t)g.n);
    a.zrows = d.take<uint32_t>((size_t)NS * (size_t)a.W32p);
    a.cases_in = d.put(cases_in.data(), (size_t)NS);
    a.violations = d.take<unsigned int>(1);
    d.zero(a.violations, 1);
    if (d.ok()) {
      d.e = launch_strata_masks(a, c->stream);
      if (d.ok()) c->strata_launches++;
    }
    if (d.ok() && K > 0) {
      d.e = launch_strata_check(a, c->stream);
      if (d.ok()) c->strata_launches++;
      unsigned int bad = 0;
      d.download(&bad, a.violations, 1);
      d.sync();
      if (!d.ok()) return;
      if (bad != 0) {
        violations = (long long)bad;
        return;
      }
    }

    // the tables: raw up, diagonal-major on the device
    std::vector<int64_t> doff;
    gcre_strata::strata_diag_offsets(size_of, doff);
    double* dvt = d.take<double>((size_t)doff[(size_t)NS]);
    for (int s = 0; s < NS && d.ok(); s++) {
      const double* d_raw = d.put(so.tables + so.tab_off[s], (size_t)so.nrow[s] * (size_t)so.ncol[s]);
      if (!d.ok()) break;
      d.e = launch_table_to_diag(d_raw, so.nrow[s], so.ncol[s], 0, (int)size_of[(size_t)s], (int)size_of[(size_t)s] + 1,
                                 dvt + doff[(size_t)s], nullptr, nullptr, nullptr, c->stream);
      if (d.ok()) c->strata_launches++;
    }
    a.dvt = dvt;
    a.doff = d.put(doff.data(), (size_t)NS);

    const int64_t slab = gcre_strata::strata_slab_sets(V, NS, M, a.W32p, g.Kpad, want_null, gcre_strata::strata_max_mb(),
                                                       gcre_strata::strata_slab_sets_env());
    const int64_t max_waves = (slab + gcre_prefix::kPrefixBlockSets - 1) / gcre_prefix::kPrefixBlockSets * gcre_prefix::kPrefixBlockSets;
    const size_t nrows = (size_t)slab * (size_t)NS;
    PrefixWaveDev* d_waves = d.take<PrefixWaveDev>((size_t)max_waves);
    a.waves = d_waves;
    a.rows = d.take<uint32_t>(nrows * urs);
    a.cnt = d.take<int32_t>(nrows * 4);
    a.tot = d.take<uint32_t>(nrows * (size_t)M);
    a.obs = d.take<double>((size_t)slab);
    a.terms = so.terms ? d.take<double>(nrows) : nullptr;
    a.n_ge = d.take<unsigned long long>((size_t)slab);
    a.null_scores = want_null ? d.take<double>((size_t)slab * (size_t)g.Kpad) : nullptr;
    a.fam_bits = fam ? d.take<unsigned long long>((size_t)g.Kpad) : nullptr;
    if (fam) d.zero(a.fam_bits, (size_t)g.Kpad);   // once: the maxima run over all slabs

    std::vector<int64_t> vsteps;
    std::vector<int32_t> order;
    std::vector<gcre_prefix::PrefixWave> waves;
    std::vector<double> obs((size_t)slab), terms(so.terms ? nrows : 0);
    std::vector<unsigned long long> ge((size_t)slab, 0);
    std::vector<int32_t> cnt(so.counts ? nrows * 4 : 0);
    for (int64_t v0 = 0; d.ok() && v0 < V; v0 += slab) {
      const int64_t nv = std::min(slab, V - v0);
      vsteps.assign((size_t)nv, (int64_t)NS);
      gcre_prefix::prefix_blocks(vsteps.data(), nv, order, waves);
      a.nslots = nv;
      a.nblocks = (int)(waves.size() / gcre_prefix::kPrefixBlockSets);
      a.urows = (const uint32_t*)r.d_rows + (size_t)v0 * urs;
      d.upload(d_waves, (const PrefixWaveDev*)waves.data(), waves.size());
      d.zero(a.cnt, (size_t)nv * (size_t)NS * 4);
      d.zero(a.n_ge, (size_t)nv);
      if (d.ok()) {
        d.e = launch_strata_rows(a, M, c->stream);
        if (d.ok()) c->strata_launches++;
      }
      if (d.ok()) {
        d.e = launch_strata_observed(a, M, c->stream);
        if (d.ok()) c->strata_launches++;
      }
      if (d.ok() && K > 0) {
        d.e = launch_strata_null(a, M, c->stream);
        if (d.ok()) c->strata_launches++;
      }
      d.download(obs.data(), a.obs, (size_t)nv);
      if (K > 0) d.download(ge.data(), a.n_ge, (size_t)nv);
      if (so.terms) d.download(terms.data(), a.terms, (size_t)nv * (size_t)NS);
      if (so.counts) d.download(cnt.data(), a.cnt, (size_t)nv * (size_t)NS * 4);
      for (int64_t e = 0; want_null && e < nv; e++)   // a row at a time, straight into the caller's matrix
        d.download(so.null_scores + (size_t)vset[(size_t)(v0 + e)] * (size_t)K, a.null_scores + (size_t)e * (size_t)g.Kpad, (size_t)K);
      d.sync();   // (the host arrays above are reused by the next slab)
      if (!d.ok()) break;
      for (int64_t e = 0; e < nv; e++) {
        const int64_t s = vset[(size_t)(v0 + e)];
        so.px[s].score = obs[(size_t)e];
        so.px[s].n_ge = K > 0 ? (int64_t)ge[(size_t)e] : 0;
        if (so.terms) std::memcpy(so.terms + (size_t)s * NS, terms.data() + (size_t)e * NS, (size_t)NS * 8);
        if (so.counts) std::memcpy(so.counts + (size_t)s * NS * 4, cnt.data() + (size_t)e * NS * 4, (size_t)NS * 16);
      }
    }
    if (fam && d.ok()) {
      d.download((unsigned long long*)so.family_max, a.fam_bits, (size_t)K);
      d.sync();
    }
  }
};

}  // namespace

extern "C" {

// Stratified scores of the given sets: gcre_score_sets, then the same device rows cut by every stratum and scored against
// the stratum's own table under the context's permutations.
int gcre_score_sets_strata(gcre_ctx* c, const gcre_set_input* in, const int32_t* stratum, int32_t n_strata, const double* tables,
                           const int32_t* nrow, const int32_t* ncol, const int64_t* tab_off, gcre_set_score* out, int64_t cap,
                           int64_t* n_out, gcre_strata_score* px_out, double* terms, int32_t* counts, double* null_scores,
                           double* family_max) {
  StrataStage st({stratum, n_strata, tables, nrow, ncol, tab_off, px_out, terms, counts, null_scores, family_max});
  const int rc = score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_strata", &st);
  if (rc == GCRE_OK && st.violations > 0) return fail(c, GCRE_ERR_ARG, gcre_strata::strata_mask_message(st.who_, st.violations));
  return rc;
}

int64_t gcre_strata_launches(const gcre_ctx* c) { return c ? c->strata_launches : -1; }

}  // extern "C"

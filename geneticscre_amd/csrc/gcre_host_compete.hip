// gcre_host_compete.hip -- gcre_score_sets_compete on a context: the stage that score_sets_common
// (gcre_set_stage.h) runs behind the set scores.  The plan -- argument checks, pool table, slab of draws -- is
// gcre_compete.h's; here are the uploads, the launches of k_compete_null (gcre_compete.hip) and the downloads.  Host code only.
#include "gcre_set_stage.h"
#include "gcre_compete.h"

namespace {

// What gcre_score_sets_compete takes and returns beside the records
struct CompeteOut {
  const int32_t* bin;       // [n_rows] or NULL
  int32_t n_bins;
  int64_t draws;
  uint64_t seed;
  int64_t* n_ge;            // [n_sets]
  double* null_scores;      // optional [n_sets][draws]
  int32_t* picks;           // optional [draws][members of the list]
};
static_assert(sizeof(gcre_compete::CompeteMember) == sizeof(CompeteMemberDev) && sizeof(CompeteMemberDev) == 8, "one layout");

struct CompeteStage final : SetStage {
  const CompeteOut co;
  explicit CompeteStage(const CompeteOut& o) : co(o) {}

  // the argument checks of gcre_compete.h, and what the device's 32-bit indices add
  int check(gcre_ctx* c, const gcre_set_input* in, const std::string& who) override {
    std::string msg;
    if (int rc = gcre_compete::check_compete_args(in, co.bin, co.n_bins, co.draws, co.n_ge != nullptr, co.null_scores != nullptr,
                                                  co.picks != nullptr, gcre_compete::compete_max_mb(), who, msg))
      return fail(c, rc, msg);
    if (in->n_sets > 0x7fffffff || (in->n_sets > 0 && in->set_off[in->n_sets] > 0x7fffffff))
      return fail(c, GCRE_ERR_ARG, who + ": too many sets or members");
    return GCRE_OK;
  }

  // an invalid set -1, a NaN row and picks of -1; zeros without a draw
  void defaults(const gcre_set_input* in, const gcre_set_score* out) override {
    const int64_t S = in->n_sets;
    for (int64_t s = 0; s < S; s++) co.n_ge[s] = out[s].valid ? 0 : -1;
    if (co.null_scores)
      std::fill(co.null_scores, co.null_scores + (size_t)S * (size_t)co.draws, std::numeric_limits<double>::quiet_NaN());
    if (co.picks && S > 0) std::fill(co.picks, co.picks + (size_t)co.draws * (size_t)in->set_off[S], -1);
  }

  bool runs(const gcre_ctx*) const override { return co.draws > 0; }

  // The caller's gene rows go up once, padded to whole 16-byte lanes; the pool table and every member's bin as gcre_compete.h
  // lays them out; then k_compete_null per slab of draws against the observed scores the device stage left.  n_ge is an exact
  // count and every draw belongs to one slab, so no result depends on the slabs.
  void run(const SetScoreRun& r) override {
    gcre_ctx* c = r.c;
    DevScratch& d = r.d;
    const gcre_set_input* in = r.in;
    const std::vector<int64_t>& vset = r.vset;
    const Geometry& g = c->g;
    const int64_t V = (int64_t)vset.size(), B = co.draws, TM = in->set_off[in->n_sets];
    std::vector<int32_t> prow, poff;
    gcre_compete::compete_pool(co.bin, in->n_rows, co.n_bins, prow, poff);
    std::vector<gcre_compete::CompeteMember> mem;
    gcre_compete::compete_members(in, co.bin, poff, mem);
    std::vector<CompeteSet> sets((size_t)V);
    int32_t maxk = 0;
    for (int64_t v = 0; v < V; v++) {
      const int64_t s = vset[(size_t)v];
      sets[(size_t)v] = {s, (int32_t)in->set_off[s], (int32_t)(in->set_off[s + 1] - in->set_off[s])};
      maxk = std::max(maxk, sets[(size_t)v].k);
    }
    const int W = g.W, Wq = (W + 1) & ~1;   // 64-bit words of a caller's row, and of a device row
    const size_t n_rows = (size_t)in->n_rows;
    uint64_t* d_rows = d.take<uint64_t>(std::max<size_t>(n_rows * (size_t)Wq, 1));
    if (Wq == W) {
      d.upload(d_rows, in->rows, n_rows * (size_t)W);
    } else {
      d.zero(d_rows, n_rows * (size_t)Wq);
      if (d.ok())
        d.e = hipMemcpy2DAsync(d_rows, (size_t)Wq * 8, in->rows, (size_t)W * 8, (size_t)W * 8, n_rows, hipMemcpyHostToDevice, c->stream);
    }
    CompeteArgs a{};
    a.rows = (const uint32_t*)d_rows;
    a.pool_rows = d.put(prow.data(), std::max<size_t>(prow.size(), 1));
    a.mem = (const CompeteMemberDev*)d.put(mem.data(), (size_t)TM);
    a.signs = g.method == 2 && in->signs ? d.put(in->signs, (size_t)TM) : nullptr;
    a.sets = d.put(sets.data(), (size_t)V);
    a.dvt = c->d_dvt;
    a.obs = r.d_obs;
    a.n_ge = d.take<unsigned long long>((size_t)V);
    d.zero(a.n_ge, (size_t)V);
    a.seed = co.seed;
    a.tm = TM;
    a.V = (int32_t)V;
    a.Wd = 2 * Wq;
    a.n = g.n;
    a.n_cases = g.n_cases;
    a.attempts = gcre_compete::compete_attempts();
    a.maxk = maxk;

    // draws per slab: the optional outputs under the bound, the grid and the 32-bit draw index in range
    const double per_draw = (co.null_scores ? (double)in->n_sets * 8.0 : 0.0) + (co.picks ? (double)TM * 4.0 : 0.0);
    int64_t slab = gcre_compete::compete_slab_draws(B, per_draw, gcre_compete::compete_max_mb());
    slab = std::min<int64_t>(slab, std::min<int64_t>((int64_t)1 << 30, std::max<int64_t>(((int64_t)0x7fffffff * 4) / V, 1)));
    // a wave walks up to 8 draws of its set, fewer while that leaves the device short of waves
    a.dpw = (int32_t)std::min<int64_t>(8, std::max<int64_t>(1, (V * std::min(slab, B)) / ((int64_t)c->cus * 64)));
    a.stride = slab;
    double* d_null = co.null_scores ? d.take<double>((size_t)V * (size_t)slab) : nullptr;
    int32_t* d_picks = co.picks ? d.take<int32_t>((size_t)slab * (size_t)TM) : nullptr;
    if (d_picks && d.ok()) d.e = hipMemsetAsync(d_picks, 0xff, (size_t)slab * (size_t)TM * 4, c->stream);   // -1: members of invalid sets
    a.null_out = d_null;
    a.picks_out = d_picks;
    std::vector<double> stage;
    for (int64_t b0 = 0; d.ok() && b0 < B; b0 += slab) {
      const int64_t nb = std::min(slab, B - b0);
      a.b0 = b0;
      a.nb = (int32_t)nb;
      a.groups = (int32_t)((nb + a.dpw - 1) / a.dpw);
      d.e = launch_compete_null(a, g.method, c->stream);
      if (d.ok()) c->compete_launches++;
      if (d_null)   // the slab's matrix at once
        fetch_rows(d, (const double*)d_null, V, slab, V, stage, co.null_scores, B, b0, nb, [&](int64_t v) { return vset[(size_t)v]; });
      if (d_picks) {
        d.download(co.picks + (size_t)b0 * (size_t)TM, d_picks, (size_t)nb * (size_t)TM);
        d.sync();
      }
    }
    std::vector<unsigned long long> ge((size_t)V);
    d.download(ge.data(), a.n_ge, (size_t)V);
    d.sync();
    if (!d.ok()) return;
    for (int64_t v = 0; v < V; v++) co.n_ge[vset[(size_t)v]] = (int64_t)ge[(size_t)v];
  }
};

}  // namespace

extern "C" {

// Competitive tests of the given sets: gcre_score_sets, then k_compete_null on the caller's gene rows against the observed
// scores the device stage left.
int gcre_score_sets_compete(gcre_ctx* c, const gcre_set_input* in, const int32_t* bin, int32_t n_bins, int64_t draws, uint64_t seed,
                            gcre_set_score* out, int64_t cap, int64_t* n_out, int64_t* n_ge, double* null_scores, int32_t* picks) {
  CompeteStage st({bin, n_bins, draws, seed, n_ge, null_scores, picks});
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_compete", &st);
}

int64_t gcre_compete_launches(const gcre_ctx* c) { return c ? c->compete_launches : -1; }

}  // extern "C"

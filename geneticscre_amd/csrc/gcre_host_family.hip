// gcre_host_family.hip -- gcre_score_sets_family on a context: the stage that score_sets_common
// (gcre_set_stage.h) runs behind the set scores.  The plan -- slab, walk order, finish -- is gcre_family.h's; here are the
// uploads, the launches of gcre_family.hip's kernels and the downloads.  Host code only.
#include "gcre_set_stage.h"
#include "gcre_family.h"

namespace {

// What gcre_score_sets_family returns beside the records
static_assert(kFamilyKmax == GCRE_FAMILY_KMAX, "the header's constant");
struct FamilyOut {
  gcre_family_score* fam;   // [n_sets]
  float* kmax;              // optional [GCRE_FAMILY_KMAX][iterations]
  float* null_scores;       // optional [n_sets][iterations]
};

struct FamilyStage final : SetStage {
  const FamilyOut fo;
  int K = 0;
  int64_t slab_tiles = 0;   // permutation tiles per slab (gcre_family.h)
  explicit FamilyStage(const FamilyOut& o) : fo(o) {}

  int check(gcre_ctx* c, const gcre_set_input* in, const std::string& who) override {
    const int64_t S = in->n_sets;
    K = c->g.K;
    if (S > 0 && !fo.fam) return fail(c, GCRE_ERR_ARG, who + ": NULL argument (fam_out)");
    int64_t V = 0;
    for (int64_t s = 0; s < S; s++) V += set_is_valid(in, s) ? 1 : 0;
    if (V > 0x7fffffff) return fail(c, GCRE_ERR_ARG, who + ": too many sets");
    std::string msg;
    if (int rc = gcre_family::family_slab(V, K, kSetPermTile, gcre_family::family_max_mb(), gcre_family::family_slab_perms(), who,
                                          slab_tiles, msg))
      return fail(c, rc, msg);
    return GCRE_OK;
  }

  // an invalid set -1 / 0 / -1, zeros in kmax and a NaN row; a valid one 0 / 0 / 0 without a permutation
  void defaults(const gcre_set_input* in, const gcre_set_score* out) override {
    const int64_t S = in->n_sets;
    for (int64_t s = 0; s < S; s++) {
      gcre_family_score& f = fo.fam[s];
      f.n_ge_stepdown = f.observed = out[s].valid ? 0 : -1;
      f.exceed = 0;
    }
    if (fo.kmax) std::fill(fo.kmax, fo.kmax + (size_t)kFamilyKmax * (size_t)K, 0.0f);
    if (fo.null_scores) std::fill(fo.null_scores, fo.null_scores + (size_t)S * (size_t)K, std::numeric_limits<float>::quiet_NaN());
  }

  bool runs(const gcre_ctx* c) const override { return c->g.K > 0; }

  // The rows of N are the valid sets in the walk's order; per slab of `slab_tiles` permutation tiles k_family_null fills N,
  // k_family_scan adds the step-down counts and stores the slab's columns of kmax, k_family_hist adds the pooled histogram.
  // Every count is an exact integer and every column belongs to one slab, so no result depends on the slabs.
  void run(const SetScoreRun& r) override {
    gcre_ctx* c = r.c;
    DevScratch& d = r.d;
    const std::vector<int64_t>& vset = r.vset;
    const int M = c->g.method;
    const int64_t V = (int64_t)vset.size();
    gcre_family::FamilyWalk w;
    gcre_family::family_walk(r.obs.data(), V, w);
    const int m = w.m;

    const int64_t tiles = ((int64_t)K + kSetPermTile - 1) / kSetPermTile;
    const int64_t max_stride = slab_tiles * kSetPermTile;
    const uint32_t* d_rank = d.put(w.rank.data(), (size_t)V);
    const uint32_t* d_meta = d.put(w.meta.data(), w.meta.size());
    const uint32_t* d_pat = d.put(w.pat.data(), (size_t)std::max(m, 1));
    uint32_t* d_N = d.take<uint32_t>((size_t)V * (size_t)max_stride);
    uint32_t* d_sd = d.take<uint32_t>((size_t)V);
    unsigned long long* d_hist = d.take<unsigned long long>((size_t)std::max(m, 1));
    uint32_t* d_kmax = fo.kmax ? d.take<uint32_t>((size_t)kFamilyKmax * (size_t)K) : nullptr;
    d.zero(d_sd, (size_t)V);
    d.zero(d_hist, (size_t)std::max(m, 1));
    FamilyNullArgs na{};
    fill_set_launch(na, c, r.d_rows, r.d_tot, V);
    na.rank = d_rank;
    na.N = d_N;
    std::vector<uint32_t> stage;
    for (int64_t kt0 = 0; d.ok() && kt0 < tiles; kt0 += slab_tiles) {
      const int64_t nk = std::min(slab_tiles, tiles - kt0);
      const int64_t stride = nk * kSetPermTile, k0 = kt0 * kSetPermTile;
      const int live = (int)std::min<int64_t>(stride, (int64_t)K - k0);
      na.kt0 = (int)kt0;
      na.nkt = (int)nk;
      na.stride = stride;
      {  // fill_set_launch's rule for the blocks per tile, over the slab's tiles
        const int64_t slots = (int64_t)c->cus * 4 * 8;
        const int64_t per = std::max<int64_t>(1, (na.npt * nk) / slots);
        na.pgroups = (int)std::min<int64_t>((na.npt + per - 1) / per, 0x7fffffff / nk);
      }
      d.e = launch_family_null(na, M, c->stream);
      if (d.ok()) c->family_launches++;
      FamilyScanArgs sa{};
      sa.N = d_N;
      sa.meta = d_meta;
      sa.n_ge = d_sd;
      sa.kmax = d_kmax;
      sa.nsets = V;
      sa.stride = stride;
      sa.kstride = K;
      sa.live = live;
      sa.k0 = (int)k0;
      if (d.ok()) {
        d.e = launch_family_scan(sa, c->stream);
        if (d.ok()) c->family_launches++;
      }
      FamilyHistArgs ha{};
      ha.N = d_N;
      ha.pat = d_pat;
      ha.hist = d_hist;
      ha.nsets = V;
      ha.stride = stride;
      ha.live = live;
      ha.m = m;
      if (d.ok() && m > 0) {
        d.e = launch_family_hist(ha, c->cus, c->stream);
        if (d.ok()) c->family_launches++;
      }
      if (fo.null_scores)   // the optional null matrix: whole rows, at most ~32 MB at a time
        fetch_rows(d, d_N, V, stride, std::max<int64_t>(1, ((int64_t)8 << 20) / stride), stage, (uint32_t*)fo.null_scores, K, k0, live,
                   [&](int64_t i) { return vset[(size_t)w.order[(size_t)i]]; });
    }
    std::vector<uint32_t> sd((size_t)V);
    std::vector<unsigned long long> hist((size_t)std::max(m, 1));
    d.download(sd.data(), d_sd, (size_t)V);
    d.download(hist.data(), d_hist, (size_t)std::max(m, 1));
    if (fo.kmax) d.download((uint32_t*)fo.kmax, d_kmax, (size_t)kFamilyKmax * (size_t)K);
    d.sync();
    if (d.ok()) gcre_family::family_finish(w, vset.data(), sd.data(), hist.data(), fo.fam);
  }
};

}  // namespace

extern "C" {

// Step-down, k-FWER and FDR over the family of the given sets: gcre_score_sets, then the family stage on the same device
// rows.  kmax[0] is the family maximum, so k_set_null is not asked for it.
int gcre_score_sets_family(gcre_ctx* c, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out,
                           gcre_family_score* fam_out, float* kmax, float* null_scores) {
  FamilyStage st({fam_out, kmax, null_scores});
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_family", &st);
}

int64_t gcre_family_launches(const gcre_ctx* c) { return c ? c->family_launches : -1; }

}  // extern "C"

// gcre_host_minp.hip -- gcre_score_sets_minp on a context: the stage that score_sets_common
// (gcre_set_stage.h) runs behind the set scores.  The plan -- slab, walk order, finish -- is gcre_minp.h's; here are the
// uploads, the launches of gcre_minp.hip's kernels (and k_family_null) and the downloads.  Host code only.
#include "gcre_set_stage.h"
#include "gcre_minp.h"

namespace {

// What gcre_score_sets_minp returns beside the records
struct MinpOut {
  gcre_minp_score* mp;      // [n_sets]
  uint32_t* min_count;      // optional [iterations]
  uint32_t* null_counts;    // optional [n_sets][iterations]
};

struct MinpStage final : SetStage {
  const MinpOut mo;
  int K = 0;
  int64_t slab_rows = 0;   // rows of the walk per slab (gcre_minp.h)
  explicit MinpStage(const MinpOut& o) : mo(o) {}

  int check(gcre_ctx* c, const gcre_set_input* in, const std::string& who) override {
    const int64_t S = in->n_sets;
    K = c->g.K;
    if (S > 0 && !mo.mp) return fail(c, GCRE_ERR_ARG, who + ": NULL argument (mp_out)");
    int64_t V = 0;
    for (int64_t s = 0; s < S; s++) V += set_is_valid(in, s) ? 1 : 0;
    if (V > 0x7fffffff) return fail(c, GCRE_ERR_ARG, who + ": too many sets");
    std::string msg;
    if (int rc = gcre_minp::minp_slab(V, K, kSetPermTile, gcre_minp::minp_max_mb(), gcre_minp::minp_slab_sets(), who, slab_rows, msg))
      return fail(c, rc, msg);
    return GCRE_OK;
  }

  // an invalid set -1 / -1 and a row of all ones, no minimum without a valid set or a permutation
  void defaults(const gcre_set_input* in, const gcre_set_score* out) override {
    const int64_t S = in->n_sets;
    for (int64_t s = 0; s < S; s++) mo.mp[s].n_le_minp = mo.mp[s].n_le_stepdown = out[s].valid ? 0 : -1;
    if (mo.min_count) std::fill(mo.min_count, mo.min_count + K, 0xffffffffu);
    if (mo.null_counts) std::fill(mo.null_counts, mo.null_counts + (size_t)S * (size_t)K, 0xffffffffu);
  }

  bool runs(const gcre_ctx* c) const override { return c->g.K > 0; }

  // k_minp_gather copies rows and totals into the walk's order.  Per slab of `slab_rows` rows of the walk k_family_null fills
  // N over all permutation tiles, k_minp_rank turns N into R, k_minp_scan carries the running minimum on and counts at the
  // end of every tie group.  Every count is an exact integer and the minimum is carried across the slabs, so no result
  // depends on them.
  void run(const SetScoreRun& r) override {
    gcre_ctx* c = r.c;
    DevScratch& d = r.d;
    const std::vector<int64_t>& vset = r.vset;
    const Geometry& g = c->g;
    const int M = g.method;
    const int64_t V = (int64_t)vset.size();
    gcre_minp::MinpWalk w;
    gcre_minp::minp_walk(r.obs.data(), r.ge.data(), V, w);
    const int64_t tiles = ((int64_t)K + kSetPermTile - 1) / kSetPermTile;
    const int64_t stride = tiles * kSetPermTile;
    const int rw = M * 2 * g.Wp;
    std::vector<uint32_t> ident((size_t)slab_rows), qinit((size_t)K, 0xffffffffu);
    for (int64_t i = 0; i < slab_rows; i++) ident[(size_t)i] = (uint32_t)i;
    const uint32_t* d_order = d.put(w.order.data(), (size_t)V);
    const uint32_t* d_meta = d.put(w.meta.data(), (size_t)V);
    const uint32_t* d_ident = d.put(ident.data(), (size_t)slab_rows);
    uint32_t* d_q = d.put(qinit.data(), (size_t)K);
    uint32_t* d_grows = d.take<uint32_t>((size_t)V * (size_t)rw);
    uint32_t* d_gtot = d.take<uint32_t>((size_t)V * (size_t)M);
    uint32_t* d_N = d.take<uint32_t>((size_t)slab_rows * (size_t)stride);
    uint32_t* d_R = d.take<uint32_t>((size_t)slab_rows * (size_t)stride);
    uint32_t* d_le = d.take<uint32_t>((size_t)V);
    d.zero(d_le, (size_t)V);
    if (d.ok()) {
      MinpGatherArgs ga{};
      ga.rows = (const uint32_t*)r.d_rows;
      ga.tot = r.d_tot;
      ga.order = d_order;
      ga.rows_out = d_grows;
      ga.tot_out = d_gtot;
      ga.nsets = V;
      ga.rw = rw;
      ga.m = M;
      d.e = launch_minp_gather(ga, c->stream);
      if (d.ok()) c->minp_launches++;
    }
    std::vector<uint32_t> stage;
    for (int64_t r0 = 0; d.ok() && r0 < V; r0 += slab_rows) {
      const int64_t nr = std::min(slab_rows, V - r0);
      FamilyNullArgs na{};
      fill_set_launch(na, c, (const uint64_t*)(d_grows + (size_t)r0 * (size_t)rw), d_gtot + (size_t)r0 * (size_t)M, nr);
      na.rank = d_ident;
      na.N = d_N;
      na.kt0 = 0;
      na.stride = stride;   // (nkt = tiles, pgroups by the rule over all tiles: as fill_set_launch left them)
      d.e = launch_family_null(na, M, c->stream);
      if (d.ok()) c->minp_launches++;
      MinpRankArgs ra{};
      ra.N = d_N;
      ra.R = d_R;
      ra.nsets = nr;
      ra.stride = stride;
      ra.K = K;
      if (d.ok()) {
        d.e = launch_minp_rank(ra, c->stream);
        if (d.ok()) c->minp_launches++;
      }
      if (mo.null_counts)   // whole rows, at most ~32 MB at a time
        fetch_rows(d, d_R, nr, stride, std::max<int64_t>(1, ((int64_t)8 << 20) / stride), stage, mo.null_counts, K, 0, K,
                   [&](int64_t i) { return vset[w.order[(size_t)(r0 + i)]]; });
      MinpScanArgs sa{};
      sa.R = d_R;
      sa.meta = d_meta + r0;
      sa.q = d_q;
      sa.n_le = d_le + r0;
      sa.nsets = nr;
      sa.stride = stride;
      sa.K = K;
      if (d.ok()) {
        d.e = launch_minp_scan(sa, c->stream);
        if (d.ok()) c->minp_launches++;
      }
    }
    std::vector<uint32_t> le((size_t)V), q((size_t)K);
    d.download(le.data(), d_le, (size_t)V);
    d.download(q.data(), d_q, (size_t)K);
    d.sync();
    if (!d.ok()) return;
    if (mo.min_count) std::memcpy(mo.min_count, q.data(), (size_t)K * 4);
    gcre_minp::minp_finish(w, r.obs.data(), r.ge.data(), vset.data(), le.data(), q, mo.mp);
  }
};

}  // namespace

extern "C" {

// Westfall-Young min-P over the family of the given sets: gcre_score_sets, then the min-P stage on the same device rows.
int gcre_score_sets_minp(gcre_ctx* c, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out,
                         gcre_minp_score* mp_out, uint32_t* min_count, uint32_t* null_counts) {
  MinpStage st({mp_out, min_count, null_counts});
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_minp", &st);
}

int64_t gcre_minp_launches(const gcre_ctx* c) { return c ? c->minp_launches : -1; }

}  // extern "C"

// gcre_host_stats.hip -- the entry points of include/gcre_hip.h that use a context but not the join driver: generated
// permutation masks, decorated p-values (gcre_decorated.hip), set scores (gcre_sets.hip, conditional: gcre_given.hip, family-wise: gcre_family.hip, min-P: gcre_minp.hip, competitive: gcre_compete.hip, variable-threshold: gcre_prefix.hip, split-half stability: gcre_subsample.hip) and carrier overlaps
// (gcre_overlap.hip), greedy clumps (gcre_clump.hip), carrier tallies per patient (gcre_patients.hip) and burden tests of per-patient weights (gcre_burden.hip), and the per-gene tally (gcre_genes.hip), the null exceedance counts (gcre_exceed.hip,
// gcre_stepdown.hip) and the hit lists (gcre_hits.hip) as objects.  What a join does with an armed tally, armed counts or
// an armed list -- check_tally, fold_genes, count_exceed, collect_hits -- is in gcre_host.hip.  Host code only.
#include "gcre_host.h"
#include "gcre_setlists.h"
#include "gcre_compete.h"
#include "gcre_prefix.h"
#include "gcre_subsample.h"
#include "gcre_clumporder.h"

namespace {

// The bit pattern of the smallest float x with (double)x >= score, among the non-negative floats null scores are: null
// score r counts (R/ProcessPaths.R:316) iff its bits are >= this -- 0 when every one counts, past +inf when none does (NaN).
uint32_t f32_threshold(double score) {
  if (score != score) return 0x7f800001u;
  if (score <= 0) return 0u;
  float f = (float)score;
  if ((double)f < score) f = std::nextafter(f, std::numeric_limits<float>::infinity());
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

// What gcre_score_sets and gcre_exceed_stepdown refuse before anything is launched (`who` opens the message): a context
// without a table or without masks, then the shape of the set list, then every set's members and signs
int check_sets(gcre_ctx* c, const gcre_set_input* in, const std::string& who) {
  if (!c->have_table || !c->d_dvt) return fail(c, GCRE_ERR_ASSERT, "assertion: " + who + " needs a value table");
  if (c->g.K > 0 && !c->have_perms)
    return fail(c, GCRE_ERR_ASSERT, "assertion: " + who + " needs the permutation masks (iterations > 0, none set)");
  std::string msg;
  int rc = check_set_shape(in, c->g.n, who, msg);
  if (rc == GCRE_OK) rc = check_set_members(in, who, msg);
  return rc == GCRE_OK ? GCRE_OK : fail(c, rc, msg);
}

// The launch geometry of k_set_null and k_stepdown_null (SetNullArgs, StepdownArgs): V sets' union rows [V][M][Wp] words and
// carrier totals against all K permutations -- the window of gcre_set_perm_window is the joins' business
template <typename Args>
void fill_set_launch(Args& a, const gcre_ctx* c, const uint64_t* d_rows, const uint32_t* d_tot, int64_t V) {
  const Geometry& g = c->g;
  a.rows = (const uint32_t*)d_rows;
  a.masks = c->d_masks;
  a.tot = d_tot;
  a.t32 = c->d_t32;
  a.d64 = c->d_dmax;
  a.d64n = c->d_dmaxn ? c->d_dmaxn : c->d_dmax;
  a.nsets = V;
  a.W32p = 2 * g.Wp;
  a.Kpad = g.Kpad;
  a.K = g.K;
  a.nkt = (g.K + kSetPermTile - 1) / kSetPermTile;
  const int64_t tpb = set_null_tile_sets(g.method);
  a.npt = (V + tpb - 1) / tpb;
  // one set tile per block while that makes at least ~8 blocks per resident block slot, more per block beyond
  const int64_t slots = (int64_t)c->cus * 4 * 8;
  const int64_t per = std::max<int64_t>(1, (a.npt * a.nkt) / slots);
  a.pgroups = (int)std::min<int64_t>((a.npt + per - 1) / per, 0x7fffffff / std::max(a.nkt, 1));
}

// The device stage gcre_score_sets and gcre_score_sets_given share.  V sets' union rows [V][M][Wp], counts [V][4] and totals
// [V][M] are on the device: the observed scores (k_set_observed), their f32 thresholds on the host and, with permutations,
// k_set_null.  obs / ge [V] are read back (ge stays as it is without permutations); d_fam [Kpad], zeroed by the caller or
// nullptr, takes the maxima over these sets too and is read back into fam_out [K] where that is given.  Ends synchronised;
// errors stay in `d`.  `launches` (or nullptr) counts the kernels launched.
struct SetStageBufs {
  uint32_t* thr;              // [V]
  double* obs;                // [V]
  unsigned long long* ge;     // [V]
};
void score_set_rows(gcre_ctx* c, DevScratch& d, const uint64_t* d_rows, const int32_t* d_cnt, const uint32_t* d_tot,
                    const SetStageBufs& b, uint32_t* d_fam, int64_t V, double* obs, unsigned long long* ge, uint32_t* fam_out,
                    int64_t* launches) {
  const int K = c->g.K, M = c->g.method;
  if (d.ok()) {
    d.e = launch_set_observed(d_cnt, V, M, c->d_dvt, b.obs, c->stream);
    if (d.ok() && launches) ++*launches;
  }
  d.download(obs, b.obs, (size_t)V);
  d.sync();
  if (d.ok() && K > 0) {
    std::vector<uint32_t> thr((size_t)V);
    for (int64_t v = 0; v < V; v++) thr[(size_t)v] = f32_threshold(obs[(size_t)v]);
    SetNullArgs a{};
    fill_set_launch(a, c, d_rows, d_tot, V);
    a.thr = b.thr;
    a.n_ge = b.ge;
    a.fam_bits = d_fam;
    d.upload(b.thr, thr.data(), (size_t)V);
    d.zero(b.ge, (size_t)V);
    if (d.ok()) {
      d.e = launch_set_null(a, M, c->stream);
      if (d.ok() && launches) ++*launches;
    }
    d.download(ge, b.ge, (size_t)V);
    if (fam_out) d.download(fam_out, d_fam, (size_t)K);
    d.sync();
  }
}

// the counts may have been queued on either stream of the context
int exceed_wait(gcre_ctx* c) {
  (void)hipSetDevice(c->device);
  if (c->stream) HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->insp_stream) HIP_TRY(c, hipStreamSynchronize(c->insp_stream));
  if (c->rec_stream) HIP_TRY(c, hipStreamSynchronize(c->rec_stream));
  return GCRE_OK;
}

// x is one of the context's live objects, or the call is refused
int exceed_alive(gcre_ctx* c, const gcre_exceed* x) {
  const auto& v = c->live_exceeds;
  return std::find(v.begin(), v.end(), x) != v.end() ? GCRE_OK : fail(c, GCRE_ERR_ARG, "exceedance counts do not belong to this context");
}

// h is one of the context's live lists, or the call is refused (a list of another context, or of a destroyed one whose
// memory is gone: the pointer is looked up, never followed)
int hits_alive(gcre_ctx* c, const gcre_hits* h) {
  const auto& v = c->live_hits;
  return std::find(v.begin(), v.end(), h) != v.end() ? GCRE_OK : fail(c, GCRE_ERR_ARG, "hit list does not belong to this context");
}

// 2^26 cells of 4 bytes: 256 MB
constexpr int64_t kExceedPermCells = (int64_t)1 << 26;

}  // namespace

extern "C" {

int gcre_generate_perm_masks(gcre_ctx* c, uint64_t seed, const int32_t* stratum, int n_strata) {
  if (!c || (stratum && n_strata < 1)) return fail(c, GCRE_ERR_ARG, "bad strata");
  (void)hipSetDevice(c->device);
  const Geometry& g = c->g;
  if (g.K == 0) { c->have_perms = true; return GCRE_OK; }
  if (!stratum) n_strata = 1;
  // cases are the first n_cases patient columns (join_base.cpp:50-54): cases and size per stratum
  std::vector<uint32_t> cases_in((size_t)n_strata, 0), size_of((size_t)n_strata, 0);
  for (int q = 0; q < g.n; q++) {
    const int s = stratum ? stratum[q] : 0;
    if (s < 0 || s >= n_strata) return fail(c, GCRE_ERR_RANGE, "stratum id out of range");
    size_of[(size_t)s]++;
    if (q < g.n_cases) cases_in[(size_t)s]++;
  }
  {
    DevScratch d(c->stream);
    const uint32_t* d_cases = d.put(cases_in.data(), (size_t)n_strata);
    const uint32_t* d_size = d.put(size_of.data(), (size_t)n_strata);
    const int32_t* d_str = stratum ? d.put(stratum, (size_t)g.n) : nullptr;
    uint32_t* d_work = d.take<uint32_t>((size_t)g.K * n_strata * 2);
    if (d.ok())
      d.e = launch_generate_masks(seed, g.K, g.n, n_strata, d_str, d_cases, d_size, d_work, 2 * g.Wp, g.Kpad, c->d_masks, c->stream);
    d.sync();
    if (!d.ok()) return fail(c, GCRE_ERR_DEVICE, std::string("generate_perm_masks: ") + hipGetErrorString(d.e));
  }
  if (int rc = build_transposed_masks(c)) return rc;
  c->have_perms = true;
  return GCRE_OK;
}

int gcre_decorated_pvalues(gcre_ctx* c, const gcre_dp_input* in, gcre_dp_split* out, int64_t cap, int64_t* n_out,
                           int32_t* perm_counts) {
  if (!c) return GCRE_ERR_ARG;
  if (!in || !n_out) return fail(c, GCRE_ERR_ARG, "decorated_pvalues: NULL argument");
  const Geometry& g = c->g;
  if (!c->have_table || !c->d_dvt) return fail(c, GCRE_ERR_ASSERT, "assertion: decorated_pvalues needs a value table");
  if (in->method != g.method || in->n_cases != g.n_cases || in->n_cases + in->n_ctrls != g.n)
    return fail(c, GCRE_ERR_ASSERT, "assertion: decorated_pvalues input does not match the context (method, cases, controls)");
  // the host stage: counts and urns (the observed scores come from the device's own table below)
  gcre_dp_input hin = *in;
  std::vector<gcre_dp_stratum> st;
  if (hin.stratum && !hin.strata_out && hin.n_strata > 0 && cap > 0) {
    st.resize((size_t)cap * (size_t)hin.n_strata);
    hin.strata_out = st.data();
  }
  int rc = gcre_decorated_splits(&hin, nullptr, 0, 0, 0, out, cap, n_out);
  if (rc == GCRE_ERR_RANGE) return fail(c, rc, "decorated_pvalues: out of range (row index, stratum id or output capacity)");
  if (rc != GCRE_OK) return fail(c, rc, "decorated_pvalues: bad input");
  const int64_t S = *n_out;
  const int K = in->iterations;
  if (S == 0) return GCRE_OK;
  if (S > 0x7fffffff) return fail(c, GCRE_ERR_ARG, "decorated_pvalues: too many splits");
  // the kernel's view: sub-path-1 counts, observed counts, urns, strata that draw, stream key
  std::vector<DpUrns> urns((size_t)S);
  std::vector<DpStratum> dst;
  for (int64_t i = 0; i < S; i++) {
    const gcre_dp_split& o = out[i];
    DpUrns& u = urns[(size_t)i];
    std::memset(&u, 0, sizeof u);
    u.key = dp_split_key(in->seed, i);
    if (!o.valid) continue;   // counts 0, no draws: p-value NaN below
    u.case_pos1 = o.case_pos1;
    u.ctrl_pos1 = o.ctrl_pos1;
    u.case_neg1 = o.case_neg1;
    u.ctrl_neg1 = o.ctrl_neg1;
    u.case_pos2 = o.case_pos2;
    u.ctrl_pos2 = o.ctrl_pos2;
    u.case_neg2 = o.case_neg2;
    u.ctrl_neg2 = o.ctrl_neg2;
    u.k_pos = o.k_pos;
    u.k_neg = o.k_neg;
    u.pop_pos = o.pop_pos;
    u.succ_pos = o.succ_pos;
    u.pop_neg = o.pop_neg;
    u.succ_neg = o.succ_neg;
    if (o.strata_off >= 0) {
      u.st_off = (int32_t)dst.size();
      for (int s = 0; s < in->n_strata; s++) {
        const gcre_dp_stratum& q = hin.strata_out[o.strata_off + s];
        if (q.k_pos + q.k_neg > 0) dst.push_back({q.pop, q.cases, q.k_pos, q.k_neg});
      }
      u.st_n = (int32_t)dst.size() - u.st_off;
      // every draw of a stratified split happens inside its strata (st_n == 0 with k_pos == k_neg == 0: nothing to draw)
    }
  }
  if (dst.size() > 0x7fffffffu) return fail(c, GCRE_ERR_ARG, "decorated_pvalues: too many strata");
  (void)hipSetDevice(c->device);
  const size_t n_pc = perm_counts ? (size_t)S * (size_t)K * 2 : 0;
  std::vector<double> obs((size_t)S);
  std::vector<unsigned long long> ge((size_t)S, 0);
  DevScratch d(c->stream);
  const DpUrns* d_urns = d.put(urns.data(), (size_t)S);
  DpStratum* d_st = d.take<DpStratum>(std::max<size_t>(dst.size(), 1));
  double* d_obs = d.take<double>((size_t)S);
  unsigned long long* d_ge = d.take<unsigned long long>((size_t)S);
  int32_t* d_pc = n_pc ? d.take<int32_t>(n_pc) : nullptr;
  if (!dst.empty()) d.upload(d_st, dst.data(), dst.size());
  d.zero(d_ge, (size_t)S);
  if (d.ok()) d.e = launch_decorated_observed(d_urns, (int)S, g.method, c->d_dvt, d_obs, c->stream);
  if (d.ok()) d.e = launch_decorated_null(d_urns, d_st, (int)S, K, g.method, c->d_dvt, d_obs, d_ge, d_pc, c->stream);
  d.download(obs.data(), d_obs, (size_t)S);
  d.download(ge.data(), d_ge, (size_t)S);
  if (n_pc) d.download(perm_counts, d_pc, n_pc);
  d.sync();
  if (!d.ok()) return fail(c, GCRE_ERR_DEVICE, std::string("decorated_pvalues: ") + hipGetErrorString(d.e));
  for (int64_t i = 0; i < S; i++) {
    gcre_dp_split& o = out[i];
    if (!o.valid) continue;
    o.score = obs[(size_t)i];
    o.n_ge = (int64_t)ge[(size_t)i];
    o.pvalue = K > 0 ? (double)o.n_ge / (double)K : std::numeric_limits<double>::quiet_NaN();
  }
  return GCRE_OK;
}

}  // extern "C"

namespace {

// What gcre_score_sets_family returns beside the records
static_assert(kFamilyKmax == GCRE_FAMILY_KMAX, "the header's constant");
struct FamilyOut {
  gcre_family_score* fam;   // [n_sets]
  float* kmax;              // optional [GCRE_FAMILY_KMAX][iterations]
  float* null_scores;       // optional [n_sets][iterations]
};

// The slab of gcre_score_sets_family: whole permutation tiles whose null matrix, one row per valid set, stays under
// GCRE_FAMILY_MAX_MB (GCRE_FAMILY_SLAB_PERMS bounds it further: tests).  One row of one tile above the limit is refused.
int check_family(gcre_ctx* c, const gcre_set_input* in, const FamilyOut& fo, const std::string& who, int64_t& slab_tiles) {
  slab_tiles = 0;
  const int64_t S = in->n_sets;
  if (S > 0 && !fo.fam) return fail(c, GCRE_ERR_ARG, who + ": NULL argument (fam_out)");
  int64_t V = 0;
  for (int64_t s = 0; s < S; s++) V += set_is_valid(in, s) ? 1 : 0;
  if (V > 0x7fffffff) return fail(c, GCRE_ERR_ARG, who + ": too many sets");
  const int K = c->g.K;
  if (V == 0 || K == 0) return GCRE_OK;
  double mb = 1024;
  if (const char* e = std::getenv("GCRE_FAMILY_MAX_MB")) mb = std::min(std::max(std::atof(e), 0.0), 1048576.0);   // tests: fractions
  const double tile_bytes = (double)V * kSetPermTile * 4.0;
  if (tile_bytes > mb * 1048576.0)
    return fail(c, GCRE_ERR_ARG, who + ": the null scores of " + std::to_string(V) + " sets under one tile of " +
                                     std::to_string(kSetPermTile) + " permutations exceed GCRE_FAMILY_MAX_MB");
  const int64_t tiles = ((int64_t)K + kSetPermTile - 1) / kSetPermTile;
  slab_tiles = std::min<int64_t>(tiles, (int64_t)(mb * 1048576.0 / tile_bytes));
  if (const char* e = std::getenv("GCRE_FAMILY_SLAB_PERMS"))
    slab_tiles = std::min<int64_t>(slab_tiles, std::max<int64_t>(std::atoll(e) / kSetPermTile, 1));
  return GCRE_OK;
}

// The family stage of gcre_score_sets_family, behind score_set_rows: V valid sets' union rows and totals are on the device,
// obs [V] are their observed scores.  The rows of N are the sets in ascending observed order (NaN first, then as doubles,
// +-0 tie); per slab of `slab_tiles` permutation tiles k_family_null fills N, k_family_scan adds the step-down counts and
// stores the slab's columns of kmax, k_family_hist adds the pooled histogram; the host takes the suffix sums.  Every count is
// an exact integer and every column belongs to one slab, so no result depends on the slabs.  Errors stay in `d`.
void family_stage(gcre_ctx* c, DevScratch& d, const uint64_t* d_rows, const uint32_t* d_tot, const std::vector<int64_t>& vset,
                  const std::vector<double>& obs, int64_t slab_tiles, const FamilyOut& fo) {
  const Geometry& g = c->g;
  const int K = g.K, M = g.method;
  const int64_t V = (int64_t)vset.size();
  std::vector<int64_t> order((size_t)V);
  for (int64_t v = 0; v < V; v++) order[(size_t)v] = v;
  std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
    const double a = obs[(size_t)x], b = obs[(size_t)y];
    const bool na = a != a, nb = b != b;
    return (na || nb) ? (na && !nb) : a < b;
  });
  // per row: the threshold pattern, the end of its tie group, the start of that group, its bin among the distinct patterns
  std::vector<uint32_t> rank((size_t)V), meta((size_t)((V + 63) / 64 * 64), 0u), pat;   // (meta: zeros up to whole 64 rows)
  std::vector<int64_t> gstart((size_t)V), bin((size_t)V, -1);
  for (int64_t i = 0; i < V; i++) {
    const double o = obs[(size_t)order[(size_t)i]];
    rank[(size_t)order[(size_t)i]] = (uint32_t)i;
    const uint32_t thr = f32_threshold(o);
    const bool end = i + 1 == V || !(obs[(size_t)order[(size_t)(i + 1)]] == o);
    meta[(size_t)i] = thr | (end ? 0x80000000u : 0u);
    gstart[(size_t)i] = i > 0 && obs[(size_t)order[(size_t)(i - 1)]] == o ? gstart[(size_t)(i - 1)] : i;
    if (o != o) continue;   // a NaN score reaches nothing and nothing reaches it
    if (pat.empty() || pat.back() != thr) pat.push_back(thr);   // (ascending: the threshold is monotone in the score)
    bin[(size_t)i] = (int64_t)pat.size() - 1;
  }
  const int m = (int)pat.size();   // 0: every score is NaN -- no histogram, and the scan counts nothing
  if (pat.empty()) pat.push_back(0u);

  const int64_t tiles = ((int64_t)K + kSetPermTile - 1) / kSetPermTile;
  const int64_t max_stride = slab_tiles * kSetPermTile;
  const uint32_t* d_rank = d.put(rank.data(), (size_t)V);
  const uint32_t* d_meta = d.put(meta.data(), meta.size());
  const uint32_t* d_pat = d.put(pat.data(), (size_t)std::max(m, 1));
  uint32_t* d_N = d.take<uint32_t>((size_t)V * (size_t)max_stride);
  uint32_t* d_sd = d.take<uint32_t>((size_t)V);
  unsigned long long* d_hist = d.take<unsigned long long>((size_t)std::max(m, 1));
  uint32_t* d_kmax = fo.kmax ? d.take<uint32_t>((size_t)kFamilyKmax * (size_t)K) : nullptr;
  d.zero(d_sd, (size_t)V);
  d.zero(d_hist, (size_t)std::max(m, 1));
  FamilyNullArgs na{};
  fill_set_launch(na, c, d_rows, d_tot, V);
  na.rank = d_rank;
  na.N = d_N;
  // the optional null matrix comes back through a staging buffer of whole rows, at most ~32 MB at a time
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
    if (fo.null_scores) {
      const int64_t rows_at_once = std::max<int64_t>(1, ((int64_t)8 << 20) / stride);
      stage.resize((size_t)std::min(rows_at_once, V) * (size_t)stride);
      for (int64_t r0 = 0; d.ok() && r0 < V; r0 += rows_at_once) {
        const int64_t nr = std::min(rows_at_once, V - r0);
        d.download(stage.data(), d_N + (size_t)r0 * (size_t)stride, (size_t)nr * (size_t)stride);
        d.sync();
        if (!d.ok()) break;
        for (int64_t r = 0; r < nr; r++)
          std::memcpy(fo.null_scores + (size_t)vset[(size_t)order[(size_t)(r0 + r)]] * (size_t)K + (size_t)k0,
                      stage.data() + (size_t)r * (size_t)stride, (size_t)live * 4);
      }
    }
  }
  std::vector<uint32_t> sd((size_t)V);
  std::vector<unsigned long long> hist((size_t)std::max(m, 1));
  d.download(sd.data(), d_sd, (size_t)V);
  d.download(hist.data(), d_hist, (size_t)std::max(m, 1));
  if (fo.kmax) d.download((uint32_t*)fo.kmax, d_kmax, (size_t)kFamilyKmax * (size_t)K);
  d.sync();
  if (!d.ok()) return;
  for (int b = m - 2; b >= 0; b--) hist[(size_t)b] += hist[(size_t)b + 1];   // exceed per bin: the suffix sums
  for (int64_t i = V - 2; i >= 0; i--)   // a tie group's count stands at its last row
    if (!(meta[(size_t)i] >> 31)) sd[(size_t)i] = sd[(size_t)i + 1];
  for (int64_t i = 0; i < V; i++) {
    gcre_family_score& f = fo.fam[vset[(size_t)order[(size_t)i]]];
    if (bin[(size_t)i] < 0) continue;   // a NaN score: 0 / 0 / 0
    f.n_ge_stepdown = (int64_t)sd[(size_t)i];
    f.exceed = hist[(size_t)bin[(size_t)i]];
    f.observed = V - gstart[(size_t)i];
  }
}

// What gcre_score_sets_minp returns beside the records
struct MinpOut {
  gcre_minp_score* mp;      // [n_sets]
  uint32_t* min_count;      // optional [iterations]
  uint32_t* null_counts;    // optional [n_sets][iterations]
};

// The slab of gcre_score_sets_minp: whole rows -- every permutation tile of a valid set, its null scores and its counts, 8
// bytes per column -- under GCRE_MINP_MAX_MB (GCRE_MINP_SLAB_SETS bounds it further: tests).  One row above the limit is refused.
int check_minp(gcre_ctx* c, const gcre_set_input* in, const MinpOut& mo, const std::string& who, int64_t& slab_rows) {
  slab_rows = 0;
  const int64_t S = in->n_sets;
  if (S > 0 && !mo.mp) return fail(c, GCRE_ERR_ARG, who + ": NULL argument (mp_out)");
  int64_t V = 0;
  for (int64_t s = 0; s < S; s++) V += set_is_valid(in, s) ? 1 : 0;
  if (V > 0x7fffffff) return fail(c, GCRE_ERR_ARG, who + ": too many sets");
  const int K = c->g.K;
  if (V == 0 || K == 0) return GCRE_OK;
  double mb = 1024;
  if (const char* e = std::getenv("GCRE_MINP_MAX_MB")) mb = std::min(std::max(std::atof(e), 0.0), 1048576.0);   // tests: fractions
  const int64_t tiles = ((int64_t)K + kSetPermTile - 1) / kSetPermTile;
  const double row_bytes = (double)tiles * kSetPermTile * 8.0;
  if (row_bytes > mb * 1048576.0)
    return fail(c, GCRE_ERR_ARG, who + ": the null scores and counts of one set under " + std::to_string(tiles) + " tiles of " +
                                     std::to_string(kSetPermTile) + " permutations exceed GCRE_MINP_MAX_MB");
  slab_rows = std::min<int64_t>(V, (int64_t)(mb * 1048576.0 / row_bytes));
  if (const char* e = std::getenv("GCRE_MINP_SLAB_SETS")) slab_rows = std::min<int64_t>(slab_rows, std::max<int64_t>(std::atoll(e), 1));
  return GCRE_OK;
}

// The min-P stage of gcre_score_sets_minp, behind score_set_rows: V valid sets' union rows and totals are on the device, obs
// [V] their observed scores and ge [V] their counts c.  The walk order is NaN scores first, then c descending, stable;
// k_minp_gather copies rows and totals into it.  Per slab of `slab_rows` rows of the walk k_family_null fills N over all
// permutation tiles, k_minp_rank turns N into R, k_minp_scan carries the running minimum on and counts at the end of every
// tie group.  Every count is an exact integer and the minimum is carried across the slabs, so no result depends on them.
// Errors stay in `d`.
void minp_stage(gcre_ctx* c, DevScratch& d, const uint64_t* d_rows, const uint32_t* d_tot, const std::vector<int64_t>& vset,
                const std::vector<double>& obs, const std::vector<unsigned long long>& ge, int64_t slab_rows, const MinpOut& mo) {
  const Geometry& g = c->g;
  const int K = g.K, M = g.method;
  const int64_t V = (int64_t)vset.size();
  std::vector<uint32_t> order((size_t)V);
  for (int64_t v = 0; v < V; v++) order[(size_t)v] = (uint32_t)v;
  auto is_nan = [&](uint32_t v) { return obs[v] != obs[v]; };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    const bool nx = is_nan(x), ny = is_nan(y);
    return (nx || ny) ? (nx && !ny) : ge[x] > ge[y];
  });
  // per row of the walk: c, and whether it ends a tie group that is counted (a run of equal c among the scored sets)
  std::vector<uint32_t> meta((size_t)V);
  for (int64_t i = 0; i < V; i++) {
    const uint32_t v = order[(size_t)i];
    const bool end = !is_nan(v) && (i + 1 == V || ge[order[(size_t)(i + 1)]] != ge[v]);   // (NaN rows come first: none follows)
    meta[(size_t)i] = (uint32_t)ge[v] | (end ? 0x80000000u : 0u);                          // c <= K < 2^31
  }
  const int64_t tiles = ((int64_t)K + kSetPermTile - 1) / kSetPermTile;
  const int64_t stride = tiles * kSetPermTile;
  const int rw = M * 2 * g.Wp;
  std::vector<uint32_t> ident((size_t)slab_rows), qinit((size_t)K, 0xffffffffu);
  for (int64_t i = 0; i < slab_rows; i++) ident[(size_t)i] = (uint32_t)i;
  const uint32_t* d_order = d.put(order.data(), (size_t)V);
  const uint32_t* d_meta = d.put(meta.data(), (size_t)V);
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
    ga.rows = (const uint32_t*)d_rows;
    ga.tot = d_tot;
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
    if (mo.null_counts) {   // whole rows through a staging buffer, at most ~32 MB at a time
      const int64_t rows_at_once = std::max<int64_t>(1, ((int64_t)8 << 20) / stride);
      stage.resize((size_t)std::min(rows_at_once, nr) * (size_t)stride);
      for (int64_t q0 = 0; d.ok() && q0 < nr; q0 += rows_at_once) {
        const int64_t nq = std::min(rows_at_once, nr - q0);
        d.download(stage.data(), d_R + (size_t)q0 * (size_t)stride, (size_t)nq * (size_t)stride);
        d.sync();
        if (!d.ok()) break;
        for (int64_t r = 0; r < nq; r++)
          std::memcpy(mo.null_counts + (size_t)vset[order[(size_t)(r0 + q0 + r)]] * (size_t)K, stage.data() + (size_t)r * (size_t)stride,
                      (size_t)K * 4);
      }
    }
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
  std::sort(q.begin(), q.end());
  for (int64_t i = V - 2; i >= 0; i--)   // a tie group's count stands at its last row
    if (!(meta[(size_t)i] >> 31) && !is_nan(order[(size_t)i])) le[(size_t)i] = le[(size_t)i + 1];
  for (int64_t i = 0; i < V; i++) {
    const uint32_t v = order[(size_t)i];
    if (is_nan(v)) continue;   // a NaN score: 0 / 0
    gcre_minp_score& m = mo.mp[vset[v]];
    m.n_le_stepdown = (int64_t)le[(size_t)i];
    m.n_le_minp = (int64_t)(std::upper_bound(q.begin(), q.end(), (uint32_t)ge[v]) - q.begin());
  }
}

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

// the argument checks of gcre_compete.h, and what the device's 32-bit indices add
int check_compete(gcre_ctx* c, const gcre_set_input* in, const CompeteOut& co, const std::string& who) {
  std::string msg;
  if (int rc = gcre_compete::check_compete_args(in, co.bin, co.n_bins, co.draws, co.n_ge != nullptr, co.null_scores != nullptr,
                                                co.picks != nullptr, gcre_compete::compete_max_mb(), who, msg))
    return fail(c, rc, msg);
  if (in->n_sets > 0x7fffffff || (in->n_sets > 0 && in->set_off[in->n_sets] > 0x7fffffff))
    return fail(c, GCRE_ERR_ARG, who + ": too many sets or members");
  return GCRE_OK;
}

// The competitive stage of gcre_score_sets_compete, behind score_set_rows: d_obs [V] are the valid sets' observed scores on
// the device.  The caller's gene rows go up once, padded to whole 16-byte lanes; the pool table and every member's bin as
// gcre_compete.h lays them out; then k_compete_null per slab of draws.  n_ge is an exact count and every draw belongs to
// one slab, so no result depends on the slabs.  Errors stay in `d`.
void compete_stage(gcre_ctx* c, DevScratch& d, const gcre_set_input* in, const double* d_obs, const std::vector<int64_t>& vset,
                   const CompeteOut& co) {
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
  a.obs = d_obs;
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
  std::vector<double> stage(d_null ? (size_t)V * (size_t)slab : 0);
  for (int64_t b0 = 0; d.ok() && b0 < B; b0 += slab) {
    const int64_t nb = std::min(slab, B - b0);
    a.b0 = b0;
    a.nb = (int32_t)nb;
    a.groups = (int32_t)((nb + a.dpw - 1) / a.dpw);
    d.e = launch_compete_null(a, g.method, c->stream);
    if (d.ok()) c->compete_launches++;
    if (d_null) {
      d.download(stage.data(), d_null, (size_t)V * (size_t)slab);
      d.sync();
      if (!d.ok()) break;
      for (int64_t v = 0; v < V; v++)
        std::memcpy(co.null_scores + (size_t)vset[(size_t)v] * (size_t)B + (size_t)b0, stage.data() + (size_t)v * (size_t)slab, (size_t)nb * 8);
    }
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

// the argument checks of gcre_prefix.h; leaves the steps of every set in `st`
int check_prefix(gcre_ctx* c, const gcre_set_input* in, const PrefixOut& po, const std::string& who, gcre_prefix::PrefixSteps& st) {
  if (in->n_sets > 0x7fffffff || (in->n_sets > 0 && in->set_off[in->n_sets] > 0x7fffffff))
    return fail(c, GCRE_ERR_ARG, who + ": too many sets or members");
  gcre_prefix::prefix_steps(in, po.cut, st);
  std::string msg;
  if (int rc = gcre_prefix::check_prefix_args(in, st, po.px != nullptr, c->g.K, c->g.method, 2 * c->g.Wp, c->g.Kpad,
                                              po.null_max != nullptr, gcre_prefix::prefix_max_mb(), who, msg))
    return fail(c, rc, msg);
  return GCRE_OK;
}

// The variable-threshold stage of gcre_score_sets_prefix, behind score_set_rows.  The caller's gene rows, set list and cut
// flags go up once; per slab of whole valid sets (gcre_prefix.h) k_prefix_rows builds the step rows and their counts,
// k_set_observed scores them, k_prefix_pick takes every set's best step and threshold and k_prefix_null the maxima over the
// steps under every permutation.  n_ge is an exact count per set and family_max a maximum across the slabs, so no result
// depends on the slabs.  Errors stay in `d`.
void prefix_stage(gcre_ctx* c, DevScratch& d, const gcre_set_input* in, const std::vector<int64_t>& vset,
                  const gcre_prefix::PrefixSteps& st, const PrefixOut& po) {
  const Geometry& g = c->g;
  const int K = g.K, M = g.method;
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

gcre_subsample::SubsampleAsk subsample_ask(const gcre_ctx* c, const SubsampleOut& so) {
  return {c->g.n_cases, c->g.n - c->g.n_cases, so.m_cases, so.m_ctrls, so.draws, so.table_a != nullptr, so.nrow_a, so.ncol_a,
          so.table_b != nullptr, so.nrow_b, so.ncol_b, so.cut, so.n_cut, so.n_a != nullptr, so.n_b != nullptr, so.n_both != nullptr,
          so.scores_a != nullptr, so.scores_b != nullptr};
}

// the argument checks of gcre_subsample.h, and what the device's 32-bit indices add
int check_subsample(gcre_ctx* c, const gcre_set_input* in, const SubsampleOut& so, const std::string& who) {
  std::string msg;
  if (int rc = gcre_subsample::check_subsample_args(in, subsample_ask(c, so), gcre_subsample::subsample_max_mb(), who, msg))
    return fail(c, rc, msg);
  if (in->n_sets > 0x7fffffff / (2 * GCRE_SUBSAMPLE_MAX_CUTS)) return fail(c, GCRE_ERR_ARG, who + ": too many sets");
  return GCRE_OK;
}

// The subsampling stage of gcre_score_sets_subsample, behind score_set_rows: d_rows are the valid sets' union rows as
// k_set_null reads them, cnt [V][4] their counts as SetUnion::build gives them.  The two tables go up as they are and become
// diagonal-major on the device (k_table_to_diag, sized for the half cohorts); then, per slab of whole draw tiles,
// k_subsample_masks and k_subsample_null.  The counts are exact sums and every draw belongs to one slab, so no result depends
// on the slabs.  Errors stay in `d`.
void subsample_stage(gcre_ctx* c, DevScratch& d, const gcre_set_input* in, const uint64_t* d_rows, const std::vector<int32_t>& cnt,
                     const std::vector<int64_t>& vset, const SubsampleOut& so) {
  const Geometry& g = c->g;
  const int M = g.method, n_cut = so.n_cut;
  const int64_t V = (int64_t)vset.size(), B = so.draws;
  const int nA = so.m_cases + so.m_ctrls, nB = g.n - nA;
  const bool have_b = so.table_b != nullptr;

  // the carriers of every half-row among the cases and among the controls (the (-) half is counted the other way round)
  std::vector<uint32_t> tot((size_t)V * 2 * M);
  for (int64_t v = 0; v < V; v++) {
    const int32_t* k = cnt.data() + 4 * v;
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
  a.rows = (const uint32_t*)d_rows;
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
  const int64_t tpb = subsample_tile_sets(M);
  a.npt = (V + tpb - 1) / tpb;

  const double per_draw = gcre_subsample::subsample_draw_bytes(in, subsample_ask(c, so));
  int64_t slab = gcre_subsample::subsample_slab_draws(B, a.W32p, per_draw, gcre_subsample::subsample_max_mb());
  slab = std::min<int64_t>(slab, (int64_t)1 << 30);   // the 32-bit draw index of a slab
  a.Kpad = (int)slab;
  a.stride = slab;
  uint32_t* d_masks = d.take<uint32_t>((size_t)a.W32p * (size_t)slab);
  a.masks = d_masks;
  a.scores_a = so.scores_a ? d.take<double>((size_t)V * (size_t)slab) : nullptr;
  a.scores_b = so.scores_b ? d.take<double>((size_t)V * (size_t)slab) : nullptr;
  std::vector<double> stage(a.scores_a || a.scores_b ? (size_t)V * (size_t)slab : 0);
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
    for (int half = 0; half < 2; half++) {
      const double* d_sc = half == 0 ? a.scores_a : a.scores_b;
      double* h_sc = half == 0 ? so.scores_a : so.scores_b;
      if (!d_sc) continue;
      d.download(stage.data(), d_sc, (size_t)V * (size_t)slab);
      d.sync();
      if (!d.ok()) break;
      for (int64_t v = 0; v < V; v++)
        std::memcpy(h_sc + (size_t)vset[(size_t)v] * (size_t)B + (size_t)b0, stage.data() + (size_t)v * (size_t)slab, (size_t)nb * 8);
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

// gcre_score_sets, with `fo` gcre_score_sets_family, with `mo` gcre_score_sets_minp, with `co` gcre_score_sets_compete, with
// `po` gcre_score_sets_prefix and with `so` gcre_score_sets_subsample: the same checks, host stage and device stage
int score_sets_common(gcre_ctx* c, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out, float* family_max,
                      const std::string& who, const FamilyOut* fo, const MinpOut* mo = nullptr, const CompeteOut* co = nullptr,
                      const PrefixOut* po = nullptr, const SubsampleOut* so = nullptr) {
  if (!c) return GCRE_ERR_ARG;
  if (!in || !n_out || cap < 0 || (cap > 0 && !out)) return fail(c, GCRE_ERR_ARG, who + ": NULL argument");
  *n_out = 0;
  const Geometry& g = c->g;
  const int K = g.K, M = g.method;
  const int64_t S = in->n_sets;
  if (int rc = check_sets(c, in, who)) return rc;
  *n_out = S;
  if (S > cap)
    return fail(c, GCRE_ERR_RANGE, who + ": " + std::to_string(S) + " sets, room for " + std::to_string(cap) +
                                       " records (out of range)");
  int64_t slab_tiles = 0;
  if (fo)
    if (int rc = check_family(c, in, *fo, who, slab_tiles)) return rc;
  int64_t slab_rows = 0;
  if (mo)
    if (int rc = check_minp(c, in, *mo, who, slab_rows)) return rc;
  if (co)
    if (int rc = check_compete(c, in, *co, who)) return rc;
  gcre_prefix::PrefixSteps steps;
  if (po)
    if (int rc = check_prefix(c, in, *po, who, steps)) return rc;
  if (so)
    if (int rc = check_subsample(c, in, *so, who)) return rc;

  // the host stage: per valid set the OR of its (+) members and of its (-) members (method 1: of all of them), within the
  // n patients, and their counts; the device rows are [valid set][M][Wp] words, the dword view k_set_null reads
  const int Wp = g.Wp;
  const size_t RW = (size_t)M * Wp;
  const SetUnion un(g.W, g.n, g.n_cases);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<int64_t> vset;     // the valid sets, in input order
  std::vector<uint64_t> urows;
  std::vector<int32_t> cnt;      // [valid][4] cases_pos, ctrls_pos, cases_neg, ctrls_neg
  std::vector<uint32_t> tot;     // [valid][M] carriers per half
  for (int64_t s = 0; s < S; s++) {
    gcre_set_score& o = out[s];
    std::memset(&o, 0, sizeof o);
    o.set = s;
    o.score = nan;
    o.pvalue = nan;
    o.valid = set_is_valid(in, s) ? 1 : 0;
    if (!o.valid) continue;
    const size_t v = vset.size();
    vset.push_back(s);
    urows.resize((v + 1) * RW, 0);
    int32_t k[4];
    un.build(in, s, urows.data() + v * RW, (size_t)Wp, M == 2, k);
    o.cases_pos = k[0];
    o.ctrls_pos = k[1];
    o.cases_neg = k[2];
    o.ctrls_neg = k[3];
    o.cases = o.cases_pos + o.cases_neg;
    o.ctrls = o.ctrls_pos + o.ctrls_neg;
    cnt.insert(cnt.end(), k, k + 4);
    tot.push_back((uint32_t)(k[0] + k[1]));
    if (M == 2) tot.push_back((uint32_t)(k[2] + k[3]));
  }
  if (family_max) std::fill(family_max, family_max + K, 0.0f);
  if (fo) {   // what an invalid set, a family without valid sets and a context without permutations keep
    for (int64_t s = 0; s < S; s++) {
      gcre_family_score& f = fo->fam[s];
      f.n_ge_stepdown = f.observed = out[s].valid ? 0 : -1;
      f.exceed = 0;
    }
    if (fo->kmax) std::fill(fo->kmax, fo->kmax + (size_t)kFamilyKmax * (size_t)K, 0.0f);
    if (fo->null_scores) std::fill(fo->null_scores, fo->null_scores + (size_t)S * (size_t)K, std::numeric_limits<float>::quiet_NaN());
  }
  if (mo) {   // as above: an invalid set -1 / -1 and a row of all ones, no minimum without a valid set or a permutation
    for (int64_t s = 0; s < S; s++) mo->mp[s].n_le_minp = mo->mp[s].n_le_stepdown = out[s].valid ? 0 : -1;
    if (mo->min_count) std::fill(mo->min_count, mo->min_count + K, 0xffffffffu);
    if (mo->null_counts) std::fill(mo->null_counts, mo->null_counts + (size_t)S * (size_t)K, 0xffffffffu);
  }
  if (co) {   // an invalid set -1, a NaN row and picks of -1; zeros without a draw
    for (int64_t s = 0; s < S; s++) co->n_ge[s] = out[s].valid ? 0 : -1;
    if (co->null_scores) std::fill(co->null_scores, co->null_scores + (size_t)S * (size_t)co->draws, nan);
    if (co->picks && S > 0) std::fill(co->picks, co->picks + (size_t)co->draws * (size_t)in->set_off[S], -1);
  }
  if (po) {   // an invalid set -1 and a NaN row; a NaN score and no best step without a permutation
    for (int64_t s = 0; s < S; s++) {
      gcre_prefix_score& x = po->px[s];
      std::memset(&x, 0, sizeof x);
      x.score = nan;
      x.n_ge = out[s].valid ? 0 : -1;
      x.best_step = -1;
      x.steps = (int32_t)(steps.off[(size_t)s + 1] - steps.off[(size_t)s]);
    }
    if (po->family_max) std::fill(po->family_max, po->family_max + K, 0.0f);
    if (po->null_max) std::fill(po->null_max, po->null_max + (size_t)S * (size_t)K, std::numeric_limits<float>::quiet_NaN());
    if (po->step_scores && S > 0) std::fill(po->step_scores, po->step_scores + (size_t)in->set_off[S], nan);
  }
  if (so) {   // an invalid set -1 and NaN rows; zeros without a draw
    for (int64_t s = 0; s < S; s++)
      for (int32_t j = 0; j < so->n_cut; j++) {
        const size_t at = (size_t)s * so->n_cut + j;
        so->n_a[at] = out[s].valid ? 0 : -1;
        if (so->n_b) so->n_b[at] = so->n_a[at];
        if (so->n_both) so->n_both[at] = so->n_a[at];
      }
    if (so->scores_a) std::fill(so->scores_a, so->scores_a + (size_t)S * (size_t)so->draws, nan);
    if (so->scores_b) std::fill(so->scores_b, so->scores_b + (size_t)S * (size_t)so->draws, nan);
  }
  const int64_t V = (int64_t)vset.size();
  if (V == 0) return GCRE_OK;

  (void)hipSetDevice(c->device);
  const bool fam = family_max && K > 0;
  std::vector<double> obs((size_t)V);
  std::vector<unsigned long long> ge((size_t)V, 0);
  std::vector<uint32_t> fbits(fam ? (size_t)K : 0);
  DevScratch d(c->stream);
  const uint64_t* d_rows = d.put(urows.data(), urows.size());
  const int32_t* d_cnt = d.put(cnt.data(), cnt.size());
  const uint32_t* d_tot = d.put(tot.data(), tot.size());
  uint32_t* d_thr = d.take<uint32_t>((size_t)V);
  double* d_obs = d.take<double>((size_t)V);
  unsigned long long* d_ge = d.take<unsigned long long>((size_t)V);
  uint32_t* d_fam = fam ? d.take<uint32_t>((size_t)g.Kpad) : nullptr;
  if (fam) d.zero(d_fam, (size_t)g.Kpad);
  score_set_rows(c, d, d_rows, d_cnt, d_tot, {d_thr, d_obs, d_ge}, d_fam, V, obs.data(), ge.data(), fam ? fbits.data() : nullptr,
                 nullptr);
  if (!d.ok()) return fail(c, GCRE_ERR_DEVICE, who + ": " + hipGetErrorString(d.e));
  for (int64_t v = 0; v < V; v++) {
    gcre_set_score& o = out[vset[(size_t)v]];
    o.score = obs[(size_t)v];
    o.n_ge = (int64_t)ge[(size_t)v];
    o.pvalue = K > 0 ? (double)o.n_ge / (double)K : nan;
  }
  if (fam) std::memcpy(family_max, fbits.data(), (size_t)K * 4);
  if (fo && K > 0) {
    family_stage(c, d, d_rows, d_tot, vset, obs, slab_tiles, *fo);
    if (!d.ok()) return fail(c, GCRE_ERR_DEVICE, who + ": " + hipGetErrorString(d.e));
  }
  if (mo && K > 0) {
    minp_stage(c, d, d_rows, d_tot, vset, obs, ge, slab_rows, *mo);
    if (!d.ok()) return fail(c, GCRE_ERR_DEVICE, who + ": " + hipGetErrorString(d.e));
  }
  if (co && co->draws > 0) {
    compete_stage(c, d, in, d_obs, vset, *co);
    if (!d.ok()) return fail(c, GCRE_ERR_DEVICE, who + ": " + hipGetErrorString(d.e));
  }
  if (po && K > 0) {
    prefix_stage(c, d, in, vset, steps, *po);
    if (!d.ok()) return fail(c, GCRE_ERR_DEVICE, who + ": " + hipGetErrorString(d.e));
  }
  if (so && so->draws > 0) {
    subsample_stage(c, d, in, d_rows, cnt, vset, *so);
    if (!d.ok()) return fail(c, GCRE_ERR_DEVICE, who + ": " + hipGetErrorString(d.e));
  }
  return GCRE_OK;
}

}  // namespace

extern "C" {

int gcre_score_sets(gcre_ctx* c, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out,
                    float* family_max) {
  return score_sets_common(c, in, out, cap, n_out, family_max, "score_sets", nullptr);
}

// Step-down, k-FWER and FDR over the family of the given sets: gcre_score_sets, then the family stage on
// the same device rows.  kmax[0] is the family maximum, so k_set_null is not asked for it.
int gcre_score_sets_family(gcre_ctx* c, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out,
                           gcre_family_score* fam_out, float* kmax, float* null_scores) {
  const FamilyOut fo{fam_out, kmax, null_scores};
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_family", &fo);
}

int64_t gcre_family_launches(const gcre_ctx* c) { return c ? c->family_launches : -1; }

// Westfall-Young min-P over the family of the given sets: gcre_score_sets, then the min-P stage on the same
// device rows.
int gcre_score_sets_minp(gcre_ctx* c, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out,
                         gcre_minp_score* mp_out, uint32_t* min_count, uint32_t* null_counts) {
  const MinpOut mo{mp_out, min_count, null_counts};
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_minp", nullptr, &mo);
}

int64_t gcre_minp_launches(const gcre_ctx* c) { return c ? c->minp_launches : -1; }

// Competitive tests of the given sets: gcre_score_sets, then k_compete_null on the caller's gene rows
// against the observed scores the device stage left.
int gcre_score_sets_compete(gcre_ctx* c, const gcre_set_input* in, const int32_t* bin, int32_t n_bins, int64_t draws, uint64_t seed,
                            gcre_set_score* out, int64_t cap, int64_t* n_out, int64_t* n_ge, double* null_scores, int32_t* picks) {
  const CompeteOut co{bin, n_bins, draws, seed, n_ge, null_scores, picks};
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_compete", nullptr, nullptr, &co);
}

int64_t gcre_compete_launches(const gcre_ctx* c) { return c ? c->compete_launches : -1; }

// Variable-threshold tests of the given sets: gcre_score_sets on the full sets, then the step rows of every
// set built on the device and the maximum over them under every permutation.
int gcre_score_sets_prefix(gcre_ctx* c, const gcre_set_input* in, const uint8_t* cut, gcre_set_score* out, int64_t cap, int64_t* n_out,
                           gcre_prefix_score* px_out, float* family_max, float* null_max, double* step_scores) {
  const PrefixOut po{cut, px_out, family_max, null_max, step_scores};
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_prefix", nullptr, nullptr, nullptr, &po);
}

int64_t gcre_prefix_launches(const gcre_ctx* c) { return c ? c->prefix_launches : -1; }

// Split-half stability of the given sets: gcre_score_sets, then the same device rows scored on random halves
// of the cohort and on their complements.
int gcre_score_sets_subsample(gcre_ctx* c, const gcre_set_input* in, int32_t m_cases, int32_t m_ctrls, int64_t draws, uint64_t seed,
                              const double* table_a, int nrow_a, int ncol_a, const double* table_b, int nrow_b, int ncol_b,
                              const double* cut, int32_t n_cut, gcre_set_score* out, int64_t cap, int64_t* n_out, int64_t* n_a,
                              int64_t* n_b, int64_t* n_both, double* scores_a, double* scores_b) {
  const SubsampleOut so{m_cases, m_ctrls, draws, seed, table_a, nrow_a, ncol_a, table_b, nrow_b, ncol_b, cut, n_cut,
                        n_a, n_b, n_both, scores_a, scores_b};
  return score_sets_common(c, in, out, cap, n_out, nullptr, "score_sets_subsample", nullptr, nullptr, nullptr, nullptr, &so);
}

int64_t gcre_subsample_launches(const gcre_ctx* c) { return c ? c->subsample_launches : -1; }

// Conditional set scores: gcre_score_sets on residual union rows that k_set_residual builds on the device
// from the caller's gene rows and set list, uploaded once.  The entries without an NA member are walked in slabs so that the
// device rows stay bounded; every slab goes through score_set_rows, and the family maxima accumulate across the slabs.
int gcre_score_sets_given(gcre_ctx* c, const gcre_set_input* in, const int64_t* which, const int64_t* given, int64_t n_which,
                          gcre_set_score* out, int64_t cap, int64_t* n_out, float* family_max) {
  if (!c) return GCRE_ERR_ARG;
  if (!in || !n_out || cap < 0 || (cap > 0 && !out)) return fail(c, GCRE_ERR_ARG, "score_sets_given: NULL argument");
  *n_out = 0;
  const Geometry& g = c->g;
  const int K = g.K, M = g.method;
  if (int rc = check_sets(c, in, "score_sets_given")) return rc;
  std::string msg;
  if (int rc = check_given_index(in, which, given, n_which, cap, "score_sets_given", msg)) return fail(c, rc, msg);
  *n_out = n_which;
  if (family_max) std::fill(family_max, family_max + K, 0.0f);
  if (n_which == 0) return GCRE_OK;

  // the entries to launch: those whose set has no NA member, in input order
  const int64_t S = in->n_sets;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<signed char> valid((size_t)S, -1);   // -1: not looked at yet
  std::vector<int64_t> ventry, vw, vg;
  for (int64_t i = 0; i < n_which; i++) {
    const int64_t s = which ? which[i] : i;
    if (valid[(size_t)s] < 0) valid[(size_t)s] = set_is_valid(in, s) ? 1 : 0;
    gcre_set_score& o = out[i];
    std::memset(&o, 0, sizeof o);
    o.set = s;
    o.score = nan;
    o.pvalue = nan;
    o.valid = valid[(size_t)s];
    if (!o.valid) continue;
    ventry.push_back(i);
    vw.push_back(s);
    vg.push_back(given ? given[i] : -1);
  }
  const int64_t V = (int64_t)ventry.size();
  if (V == 0) return GCRE_OK;

  // entries per slab: 1 GiB of residual rows, one tile of k_set_null at the least (GCRE_GIVEN_SLAB_SETS: tests)
  const size_t RW = (size_t)M * g.Wp;   // words per entry
  int64_t slab = std::max<int64_t>(((int64_t)1 << 30) / (int64_t)(RW * 8), set_null_tile_sets(M));
  if (const char* e = std::getenv("GCRE_GIVEN_SLAB_SETS")) slab = std::min<int64_t>(std::max<int64_t>(std::atoll(e), 1), (int64_t)1 << 28);
  slab = std::min(slab, V);

  (void)hipSetDevice(c->device);
  const bool fam = family_max && K > 0;
  const bool split = M == 2 && in->signs;
  const int64_t n_members = in->set_off[S];
  std::vector<double> obs((size_t)slab);
  std::vector<unsigned long long> ge((size_t)slab);
  std::vector<int32_t> cnt((size_t)slab * 4);
  std::vector<uint32_t> fbits(fam ? (size_t)K : 0);
  DevScratch d(c->stream);
  SetResidualArgs a{};
  a.rows = (const uint32_t*)d.put(in->rows, std::max<size_t>((size_t)in->n_rows * (size_t)g.W, 1));
  a.set_off = d.put(in->set_off, (size_t)S + 1);
  a.members = d.put(in->members, (size_t)n_members);
  a.signs = split ? d.put(in->signs, (size_t)n_members) : nullptr;
  const int64_t* d_which = d.put(vw.data(), (size_t)V);
  const int64_t* d_given = d.put(vg.data(), (size_t)V);
  uint64_t* d_rows = d.take<uint64_t>((size_t)slab * RW);
  a.out = (uint32_t*)d_rows;
  a.cnt = d.take<int32_t>((size_t)slab * 4);
  a.tot = d.take<uint32_t>((size_t)slab * M);
  a.W2 = 2 * g.W;
  a.W32p = 2 * g.Wp;
  a.n_patients = g.n;
  a.n_cases = g.n_cases;
  const SetStageBufs b{d.take<uint32_t>((size_t)slab), d.take<double>((size_t)slab), d.take<unsigned long long>((size_t)slab)};
  uint32_t* d_fam = fam ? d.take<uint32_t>((size_t)g.Kpad) : nullptr;
  if (fam) d.zero(d_fam, (size_t)g.Kpad);   // once: the maxima run over all slabs
  int64_t slabs = 0;
  for (int64_t v0 = 0; d.ok() && v0 < V; v0 += slab, slabs++) {
    const int64_t nv = std::min(slab, V - v0);
    a.which = d_which + v0;
    a.given = d_given + v0;
    a.n = nv;
    d.e = launch_set_residual(a, M, c->stream);
    if (d.ok()) c->given_launches++;
    d.download(cnt.data(), a.cnt, (size_t)nv * 4);
    std::fill(ge.begin(), ge.begin() + nv, 0ull);
    score_set_rows(c, d, d_rows, a.cnt, a.tot, b, d_fam, nv, obs.data(), ge.data(),
                   fam && v0 + nv == V ? fbits.data() : nullptr, &c->given_launches);
    if (!d.ok()) break;
    for (int64_t v = 0; v < nv; v++) {
      gcre_set_score& o = out[ventry[(size_t)(v0 + v)]];
      const int32_t* k = cnt.data() + 4 * v;
      o.cases_pos = k[0];
      o.ctrls_pos = k[1];
      o.cases_neg = k[2];
      o.ctrls_neg = k[3];
      o.cases = o.cases_pos + o.cases_neg;
      o.ctrls = o.ctrls_pos + o.ctrls_neg;
      o.score = obs[(size_t)v];
      o.n_ge = (int64_t)ge[(size_t)v];
      o.pvalue = K > 0 ? (double)o.n_ge / (double)K : nan;
    }
  }
  if (!d.ok()) return fail(c, GCRE_ERR_DEVICE, std::string("score_sets_given: ") + hipGetErrorString(d.e));
  if (std::getenv("GCRE_GIVEN_STATS"))   // (tools/given_time.py)
    fprintf(stderr, "given entries=%lld launched=%lld slab=%lld slabs=%lld\n", (long long)n_which, (long long)V, (long long)slab,
            (long long)slabs);
  if (fam) std::memcpy(family_max, fbits.data(), (size_t)K * 4);
  return GCRE_OK;
}

int64_t gcre_given_launches(const gcre_ctx* c) { return c ? c->given_launches : -1; }

// Carrier overlaps of caller-given sets: the validation of gcre_score_sets, the OR of every valid set's
// members on the host, then k_set_overlap over the `a` list in slabs whose device output stays under GCRE_OVERLAP_SLAB_MB.
int gcre_set_overlap(gcre_ctx* c, const gcre_set_input* in, const int64_t* a, int64_t na, const int64_t* b, int64_t nb,
                     int32_t* size, int32_t* both) {
  if (!c) return GCRE_ERR_ARG;
  if (!in) return fail(c, GCRE_ERR_ARG, "set_overlap: NULL argument");
  const Geometry& g = c->g;
  std::string msg;
  if (int rc = check_set_shape(in, g.n, "set_overlap", msg)) return fail(c, rc, msg);
  const int64_t S = in->n_sets;
  if (na < 0 || nb < 0 || (!a && na != S) || (!b && nb != S))
    return fail(c, GCRE_ERR_ARG, "set_overlap: bad index list (a negative length, or NULL with a length other than n_sets)");
  if (int rc = check_set_members(in, "set_overlap", msg)) return fail(c, rc, msg);
  for (int side = 0; side < 2; side++) {
    const int64_t* idx = side ? b : a;
    const int64_t cnt = side ? nb : na;
    for (int64_t i = 0; idx && i < cnt; i++)
      if (idx[i] < 0 || idx[i] >= S)
        return fail(c, GCRE_ERR_RANGE, std::string("set_overlap: ") + (side ? "b[" : "a[") + std::to_string(i) + "] = " +
                                           std::to_string(idx[i]) + " out of range (" + std::to_string(S) + " sets)");
  }
  if (S > 0x7fffffff) return fail(c, GCRE_ERR_ARG, "set_overlap: too many sets");
  const bool pairs = both && na > 0 && nb > 0;
  if (!size && !pairs) return GCRE_OK;

  // the host stage: per valid set the OR of all its members within the n patients, as [valid set][Wdp] dwords (zero
  // padded to whole chunks of the kernel), and its case / control counts
  const int W = g.W;
  const int Wdp = (2 * W + kOverlapChunk - 1) / kOverlapChunk * kOverlapChunk;
  const size_t RW = (size_t)Wdp / 2;   // words per device row
  const SetUnion un(W, g.n, g.n_cases);
  std::vector<int32_t> vrow((size_t)S, -1);   // set -> row of urows, -1 = an NA member
  std::vector<uint64_t> urows;
  int64_t V = 0;
  for (int64_t s = 0; s < S; s++) {
    if (!set_is_valid(in, s)) {
      if (size) size[2 * s] = size[2 * s + 1] = -1;
      continue;
    }
    vrow[(size_t)s] = (int32_t)V;
    urows.resize((size_t)(V + 1) * RW, 0);
    int32_t k[4];
    un.build(in, s, urows.data() + (size_t)V * RW, 0, false, size ? k : nullptr);   // all members into one row, whatever their signs
    V++;
    if (size) std::memcpy(size + 2 * s, k, 8);   // cases, controls
  }
  if (!pairs) return GCRE_OK;
  if (V == 0) {   // every set has an NA member: all overlaps are 0
    std::memset(both, 0, (size_t)na * (size_t)nb * 8);
    return GCRE_OK;
  }
  urows.resize((size_t)(V + 1) * RW, 0);   // row V, all zeros: what a set with an NA member and a tile's remainder read
  auto row_of = [&](int64_t s) { return vrow[(size_t)s] < 0 ? (int32_t)V : vrow[(size_t)s]; };
  std::vector<int32_t> ia((size_t)na), ib((size_t)nb);
  for (int64_t i = 0; i < na; i++) ia[(size_t)i] = row_of(a ? a[i] : i);
  for (int64_t j = 0; j < nb; j++) ib[(size_t)j] = row_of(b ? b[j] : j);

  // `a` rows per launch: whole tiles, the output of a launch under the bound (one tile row at the least), the grid in range
  double slab_mb = 256;
  if (const char* e = std::getenv("GCRE_OVERLAP_SLAB_MB")) slab_mb = std::min(std::max(std::atof(e), 0.0), 65536.0);   // tests: fractions
  const int64_t ntb = (nb + kOverlapTile - 1) / kOverlapTile;
  int64_t slab = (int64_t)(slab_mb * 1048576.0) / (nb * 8) / kOverlapTile * kOverlapTile;
  slab = std::max<int64_t>(slab, kOverlapTile);
  slab = std::min<int64_t>(slab, (0x7fffffff / ntb) * kOverlapTile);
  slab = std::min<int64_t>(slab, (na + kOverlapTile - 1) / kOverlapTile * kOverlapTile);
  if (slab < kOverlapTile) return fail(c, GCRE_ERR_ARG, "set_overlap: too many b entries for one launch");

  (void)hipSetDevice(c->device);
  DevScratch d(c->stream);
  const uint64_t* d_rows = d.put(urows.data(), urows.size());
  const int32_t* d_ia = d.put(ia.data(), (size_t)na);
  const int32_t* d_ib = d.put(ib.data(), (size_t)nb);
  int32_t* d_both = d.take<int32_t>((size_t)std::min(slab, na) * (size_t)nb * 2);
  for (int64_t r0 = 0; d.ok() && r0 < na; r0 += slab) {
    OverlapArgs o{};
    o.rows = (const uint32_t*)d_rows;
    o.ia = d_ia + r0;
    o.ib = d_ib;
    o.both = d_both;
    o.na = std::min(slab, na - r0);
    o.nb = nb;
    o.ntb = ntb;
    o.Wdp = Wdp;
    o.n_cases = g.n_cases;
    o.zero_row = (int)V;
    d.e = launch_set_overlap(o, c->stream);
    if (d.ok()) c->overlap_launches++;
    d.download(both + (size_t)r0 * (size_t)nb * 2, d_both, (size_t)o.na * (size_t)nb * 2);
    d.sync();   // the next slab writes d_both again
  }
  if (!d.ok()) return fail(c, GCRE_ERR_DEVICE, std::string("set_overlap: ") + hipGetErrorString(d.e));
  return GCRE_OK;
}

int64_t gcre_overlap_launches(const gcre_ctx* c) { return c ? c->overlap_launches : -1; }

// Greedy clumping of caller-given sets on the device: report.clump_rows without a pair count leaving the
// GPU.  The gene rows and a member table in walk order go up once; k_clump_union makes the union rows; rounds of
// k_clump_leads + k_clump_assign are queued in batches, the 16-byte state of the walk is read once per batch.
int gcre_clump_sets(gcre_ctx* c, const gcre_set_input* in, const int64_t* order, int64_t n_order, double r, int measure,
                    int patients, int32_t* size, int64_t* clump, int64_t* lead, double* value, int32_t* shared) {
  if (!c) return GCRE_ERR_ARG;
  if (!in) return fail(c, GCRE_ERR_ARG, "clump_sets: NULL argument");
  const Geometry& g = c->g;
  std::string msg;
  if (int rc = check_set_shape(in, g.n, "clump_sets", msg)) return fail(c, rc, msg);
  if (int rc = check_set_members(in, "clump_sets", msg)) return fail(c, rc, msg);
  const int64_t S = in->n_sets;
  if (S > 0 && (!clump || !lead || !value || !shared)) return fail(c, GCRE_ERR_ARG, "clump_sets: NULL output");
  if (int rc = check_clump_rule(r, measure, patients, msg)) return fail(c, rc, msg);
  if (int rc = check_clump_order(in, order, n_order, msg)) return fail(c, rc, msg);
  const int W = g.W;
  const int Wdp = (2 * W + kOverlapChunk - 1) / kOverlapChunk * kOverlapChunk;
  if (int rc = check_clump_bytes(n_order, (int64_t)Wdp * 4, clump_max_mb(), msg)) return fail(c, rc, msg);
  if (n_order >= 0x7ffffff0) return fail(c, GCRE_ERR_ARG, "clump_sets: too many rows");

  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t s = 0; s < S; s++) {
    clump[s] = lead[s] = -1;
    value[s] = nan;
    shared[2 * s] = shared[2 * s + 1] = -1;
  }
  // the sizes of the sets outside the walk, as gcre_set_overlap fills them (those inside it come from the device)
  std::vector<unsigned char> walked((size_t)S, 0);
  for (int64_t i = 0; i < n_order; i++) walked[(size_t)order[i]] = 1;
  if (size) {
    const SetUnion un(W, g.n, g.n_cases);
    std::vector<uint64_t> row((size_t)std::max(W, 1));
    for (int64_t s = 0; s < S; s++) {
      if (walked[(size_t)s]) continue;
      if (!set_is_valid(in, s)) {
        size[2 * s] = size[2 * s + 1] = -1;
        continue;
      }
      std::fill(row.begin(), row.end(), 0);
      int32_t k[4];
      un.build(in, s, row.data(), 0, false, k);
      std::memcpy(size + 2 * s, k, 8);
    }
  }
  if (n_order == 0) return GCRE_OK;

  // the member table [n_order][M] in walk order, -1 behind a set's last member
  const int64_t n = n_order;
  int64_t M = 1;
  for (int64_t i = 0; i < n; i++) M = std::max(M, in->set_off[order[i] + 1] - in->set_off[order[i]]);
  if (M > 0x7fffffff / 4 || (double)n * (double)M * 4.0 > clump_max_mb() * 1048576.0)
    return fail(c, GCRE_ERR_ARG, "clump_sets: the member table of " + std::to_string(n) + " rows x " + std::to_string(M) +
                                     " members exceeds GCRE_CLUMP_MAX_MB");
  std::vector<int32_t> table((size_t)n * (size_t)M, -1);
  for (int64_t i = 0; i < n; i++) {
    const int64_t b = in->set_off[order[i]], e = in->set_off[order[i] + 1];
    std::copy(in->members + b, in->members + e, table.begin() + (size_t)i * (size_t)M);
  }

  (void)hipSetDevice(c->device);
  DevScratch d(c->stream);
  ClumpArgs a{};
  ClumpUnionArgs u{};
  u.rows = (const uint32_t*)d.put(in->rows, std::max<size_t>((size_t)in->n_rows * (size_t)W, 1));
  u.members = d.put(table.data(), table.size());
  u.M = (int)M;
  u.W2 = 2 * W;
  u.n_patients = g.n;
  a.U = d.take<uint32_t>((size_t)(n + 1) * (size_t)Wdp);
  a.cnt = d.take<int32_t>((size_t)n * 2);
  a.free_ = d.take<uint32_t>((size_t)n);
  a.clump = d.take<int32_t>((size_t)n);
  a.lead = d.take<int32_t>((size_t)n);
  a.value = d.take<double>((size_t)n);
  a.shared = d.take<int32_t>((size_t)n * 2);
  a.state = d.take<ClumpState>(1);
  a.leads = d.take<int32_t>(kClumpCand);
  a.stats = d.take<unsigned long long>(kClumpStats);
  a.n = n;
  a.Wdp = Wdp;
  a.n_cases = g.n_cases;
  a.measure = measure;
  a.patients = patients;
  a.r = r;
  if (d.ok()) d.zero(a.U + (size_t)n * (size_t)Wdp, (size_t)Wdp);   // the zero row
  d.zero(a.state, 1);
  d.zero(a.stats, kClumpStats);
  if (d.ok()) d.e = launch_clump_union(a, u, c->stream);
  if (d.ok()) c->clump_launches++;
  // rounds in batches: every kernel of a round reads the state and ends at once on an empty round, so a batch may run
  // past the end of the walk; tiles below the cursor the host saw last are not launched at all
  constexpr int kBatch = 16;
  ClumpState st{};
  int64_t batches = 0;
  while (d.ok() && st.cursor < n) {
    const int64_t tile0 = st.cursor / kOverlapTile;
    for (int k = 0; d.ok() && k < kBatch; k++) {
      d.e = launch_clump_round(a, tile0, c->stream);
      if (d.ok()) c->clump_launches += 2;
    }
    d.download(&st, a.state, 1);
    d.sync();
    batches++;
  }
  std::vector<int32_t> cnt((size_t)n * 2), h_clump((size_t)n), h_lead((size_t)n), h_shared((size_t)n * 2);
  std::vector<double> h_value((size_t)n);
  unsigned long long stats[kClumpStats] = {};
  d.download(cnt.data(), a.cnt, cnt.size());
  d.download(h_clump.data(), a.clump, h_clump.size());
  d.download(h_lead.data(), a.lead, h_lead.size());
  d.download(h_value.data(), a.value, h_value.size());
  d.download(h_shared.data(), a.shared, h_shared.size());
  d.download(stats, a.stats, (size_t)kClumpStats);
  d.sync();
  d.release();
  if (!d.ok()) {
    (void)hipGetLastError();
    return fail(c, GCRE_ERR_DEVICE, std::string("clump_sets: ") + hipGetErrorString(d.e));
  }
  if (std::getenv("GCRE_CLUMP_STATS"))   // (tools/clump_time.py)
    fprintf(stderr, "clump rows=%lld rounds=%llu leads=%d batches=%lld tiles_run=%llu tiles_skipped=%llu\n", (long long)n,
            stats[kClumpRounds], st.next_clump, (long long)batches, stats[kClumpTilesRun], stats[kClumpTilesSkipped]);
  for (int64_t i = 0; i < n; i++) {
    const int64_t s = order[i];
    if (size) std::memcpy(size + 2 * s, cnt.data() + 2 * i, 8);
    clump[s] = h_clump[(size_t)i];
    lead[s] = order[h_lead[(size_t)i]];
    value[s] = h_value[(size_t)i];
    shared[2 * s] = h_shared[2 * (size_t)i];
    shared[2 * s + 1] = h_shared[2 * (size_t)i + 1];
  }
  return GCRE_OK;
}

int64_t gcre_clump_launches(const gcre_ctx* c) { return c ? c->clump_launches : -1; }

// Carrier tallies per patient: the validation of gcre_set_overlap, then the kept entries -- group >= 0,
// no NA member -- counting-sorted by group into a member table and cut into segments of one group each; gene rows, table
// and segments go up once, k_set_patient_counts adds into zeroed cells, which come back as they are (a count is below
// n_which < 2^31).
int gcre_set_patient_counts(gcre_ctx* c, const gcre_set_input* in, const int64_t* which, int64_t n_which, const int32_t* group,
                            int32_t n_groups, int by_sign, int32_t* counts, int64_t* group_sets, int64_t* skipped) {
  if (!c) return GCRE_ERR_ARG;
  if (!in) return fail(c, GCRE_ERR_ARG, "set_patient_counts: NULL argument");
  const Geometry& g = c->g;
  const std::string who = "set_patient_counts";
  std::string msg;
  if (int rc = check_set_shape(in, g.n, who, msg)) return fail(c, rc, msg);
  if (int rc = check_set_members(in, who, msg)) return fail(c, rc, msg);
  if (int rc = check_patient_index(in, which, n_which, group, n_groups, by_sign, counts != nullptr, patient_max_mb(), who, msg))
    return fail(c, rc, msg);
  if (by_sign && in->n_rows > (int64_t)kPatientNegBit)
    return fail(c, GCRE_ERR_ARG, who + ": too many gene rows for by_sign (the sign travels in bit 30 of a member)");
  const auto t_begin = std::chrono::steady_clock::now();
  const int H = 1 + by_sign, W = g.W;
  const size_t n_cells = (size_t)n_groups * (size_t)H * (size_t)g.n;
  std::memset(counts, 0, n_cells * sizeof(int32_t));
  if (group_sets) std::memset(group_sets, 0, (size_t)n_groups * sizeof(int64_t));
  if (skipped) *skipped = 0;

  // the kept entries, counting-sorted by group (stable): at[g] = where group g's run begins
  const int64_t S = in->n_sets;
  std::vector<unsigned char> valid((size_t)S);
  for (int64_t s = 0; s < S; s++) valid[(size_t)s] = set_is_valid(in, s);
  std::vector<int64_t> at((size_t)n_groups + 1, 0);
  int64_t n_skipped = 0, M = 1;
  for (int64_t i = 0; i < n_which; i++) {
    const int32_t gi = group ? group[i] : 0;
    if (gi < 0) continue;
    const int64_t s = which ? which[i] : i;
    if (!valid[(size_t)s]) {
      n_skipped++;
      continue;
    }
    at[(size_t)gi + 1]++;
    M = std::max(M, in->set_off[s + 1] - in->set_off[s]);
  }
  if (skipped) *skipped = n_skipped;
  for (int32_t k = 0; k < n_groups; k++) {
    if (group_sets) group_sets[k] = at[(size_t)k + 1];
    at[(size_t)k + 1] += at[(size_t)k];
  }
  const int64_t n = at[(size_t)n_groups];
  if (n == 0 || g.n == 0) return GCRE_OK;
  if (M > 0x7fffffff / 4 || (double)n * (double)M * 4.0 > patient_max_mb() * 1048576.0)
    return fail(c, GCRE_ERR_ARG, who + ": the member table of " + std::to_string(n) + " entries x " + std::to_string(M) +
                                     " members exceeds GCRE_PATIENT_MAX_MB");

  // the member table [M][n] in sorted order -- member m of every entry side by side, which the kernel reads 16 entries at a
  // time -- with -1 behind a set's last member; by_sign: bit 30 marks a (-) member
  std::vector<int32_t> table((size_t)n * (size_t)M, -1), width((size_t)n);
  {
    std::vector<int64_t> next(at.begin(), at.end() - 1);
    for (int64_t i = 0; i < n_which; i++) {
      const int32_t gi = group ? group[i] : 0;
      const int64_t s = which ? which[i] : i;
      if (gi < 0 || !valid[(size_t)s]) continue;
      const int64_t pos = next[(size_t)gi]++, b = in->set_off[s], e = in->set_off[s + 1];
      for (int64_t k = b; k < e; k++)
        table[(size_t)(k - b) * (size_t)n + (size_t)pos] = in->members[k] | (by_sign && in->signs && in->signs[k] == -1 ? kPatientNegBit : 0);
      width[(size_t)pos] = (int32_t)(e - b);
    }
  }
  // segments: every group's run in pieces of at most GCRE_PATIENT_SEG entries; by default as many as spread the (segment,
  // tile) pairs over about 4,096 waves, between 64 (a flush per segment is 32 atomic instructions) and 1,024
  const int64_t tiles = (g.n + kPatientTile - 1) / kPatientTile;
  int64_t seg = std::min<int64_t>(std::max<int64_t>((n * tiles + 4095) / 4096, 64), 1024);
  if (const char* e = std::getenv("GCRE_PATIENT_SEG")) seg = std::min<int64_t>(std::max<int64_t>(std::atoll(e), 1), (int64_t)1 << 30);
  std::vector<PatientSeg> segs;
  for (int32_t k = 0; k < n_groups; k++)
    for (int64_t b = at[(size_t)k]; b < at[(size_t)k + 1]; b += seg) {
      PatientSeg sg{};
      sg.begin = (int32_t)b;
      sg.count = (int32_t)std::min(seg, at[(size_t)k + 1] - b);
      sg.group = k;
      sg.width = *std::max_element(width.begin() + b, width.begin() + b + sg.count);
      segs.push_back(sg);
    }

  // GCRE_PATIENT_STATS (tools/patients_time.py): one line on stderr, with the stages timed between extra synchronisations
  const bool stats = std::getenv("GCRE_PATIENT_STATS") != nullptr;
  const auto now = [] { return std::chrono::steady_clock::now(); };
  const auto ms = [](std::chrono::steady_clock::time_point t0, std::chrono::steady_clock::time_point t1) {
    return std::chrono::duration<double, std::milli>(t1 - t0).count();
  };
  const auto t_host = now();
  (void)hipSetDevice(c->device);
  DevScratch d(c->stream);
  PatientCountArgs a{};
  a.rows = (const uint32_t*)d.put(in->rows, std::max<size_t>((size_t)in->n_rows * (size_t)W, 1));
  a.members = d.put(table.data(), table.size());
  a.segs = d.put(segs.data(), segs.size());
  a.cells = d.take<uint32_t>(n_cells);
  a.n = n;
  a.nseg = (int64_t)segs.size();
  a.M = (int)M;
  a.W2 = 2 * W;
  a.n_patients = g.n;
  a.H = H;
  d.zero(a.cells, n_cells);
  if (stats) d.sync();
  const auto t_up = now();
  if (d.ok()) {
    d.e = launch_set_patient_counts(a, c->stream);
    if (d.ok()) c->patient_launches++;
  }
  d.download((uint32_t*)counts, a.cells, n_cells);
  d.sync();
  d.release();
  if (!d.ok()) {
    (void)hipGetLastError();
    std::memset(counts, 0, n_cells * sizeof(int32_t));
    return fail(c, GCRE_ERR_DEVICE, who + ": " + hipGetErrorString(d.e));
  }
  if (stats)
    fprintf(stderr, "patients entries=%lld members=%lld segments=%lld groups=%d planes=%d upload_bytes=%lld host_ms=%.3f upload_ms=%.3f "
                    "kernel_download_ms=%.3f\n", (long long)n, (long long)M, (long long)segs.size(), n_groups, H,
            (long long)((size_t)in->n_rows * (size_t)W * 8 + table.size() * 4 + segs.size() * sizeof(PatientSeg)), ms(t_begin, t_host),
            ms(t_host, t_up), ms(t_up, now()));
  return GCRE_OK;
}

int64_t gcre_patient_launches(const gcre_ctx* c) { return c ? c->patient_launches : -1; }

// Burden tests of per-patient weights.  check_burden_args gives every row's planes; totals and observed
// sums are the host's.  The rows are walked in slabs whose planes and sums stay under GCRE_BURDEN_MAX_MB; of a slab the
// rows with a non-zero weight are listed, their planes cut into items, and three kernels run: k_burden_planes,
// k_burden_null, k_burden_finish.  Every sum is an exact integer, so no result depends on the slabs.
int gcre_patient_burden(gcre_ctx* c, const int32_t* weights, int64_t n_rows, int32_t n_cols, gcre_burden* out, int64_t* null_sums) {
  if (!c) return GCRE_ERR_ARG;
  const Geometry& g = c->g;
  const std::string who = "patient_burden";
  const int K = g.K, W32p = 2 * g.Wp;
  std::string msg;
  std::vector<int32_t> planes;
  if (int rc = check_burden_args(weights, n_rows, n_cols, g.n, out != nullptr, K, c->have_perms, W32p, g.Kpad, burden_max_mb(), who,
                                 planes, msg))
    return fail(c, rc, msg);
  if (n_rows == 0) return GCRE_OK;
  const auto t_begin = std::chrono::steady_clock::now();
  const int n = g.n;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<int64_t> observed((size_t)n_rows);
  for (int64_t r = 0; r < n_rows; r++) {
    const int32_t* w = weights + (size_t)r * (size_t)n;
    int64_t cases = 0, all = 0;
    for (int q = 0; q < n; q++) {
      all += w[q];
      if (q < g.n_cases) cases += w[q];
    }
    gcre_burden& o = out[r];
    std::memset(&o, 0, sizeof o);
    o.total = all;
    o.observed = observed[(size_t)r] = cases;
    o.planes = planes[(size_t)r];
    // a row of zeros: every sum is 0 = observed, a tie in both tails
    o.n_ge = o.n_le = o.planes == 0 ? K : 0;
    o.p_upper = o.p_lower = K > 0 && o.planes == 0 ? 1.0 : nan;
  }
  if (K == 0) return GCRE_OK;
  if (null_sums) std::memset(null_sums, 0, (size_t)n_rows * (size_t)K * sizeof(int64_t));

  // GCRE_BURDEN_STATS (tools/burden_time.py): one line on stderr
  const bool stats = std::getenv("GCRE_BURDEN_STATS") != nullptr;
  int64_t slab_rows = n_rows, n_slabs = 0, n_items = 0, n_planes = 0;
  if (const char* e = std::getenv("GCRE_BURDEN_SLAB_ROWS")) slab_rows = std::min<int64_t>(std::max<int64_t>(std::atoll(e), 1), n_rows);
  const double cap = burden_max_mb() * 1048576.0;
  (void)hipSetDevice(c->device);
  for (int64_t r0 = 0; r0 < n_rows;) {
    // the slab [r0, r1): rows while their planes and sums fit (one row always does: check_burden_args)
    int64_t r1 = r0;
    double bytes = 0;
    while (r1 < n_rows && r1 - r0 < slab_rows && r1 - r0 < 0x7fffffff) {
      const double more = (double)planes[(size_t)r1] * W32p * 4.0 + (double)g.Kpad * 8.0;
      if (r1 > r0 && bytes + more > cap) break;
      bytes += more;
      r1++;
    }
    const int64_t rows = r1 - r0;
    std::vector<int32_t> act, np, pbase;
    std::vector<int64_t> obs;
    std::vector<BurdenItem> items;
    int32_t at = 0;
    for (int64_t r = r0; r < r1; r++) {
      const int32_t p = planes[(size_t)r];
      if (p == 0) continue;
      act.push_back((int32_t)(r - r0));
      np.push_back(p);
      pbase.push_back(at);
      obs.push_back(observed[(size_t)r]);
      for (int32_t b = 0; b < p; b += kBurdenItemPlanes)
        items.push_back({(int32_t)(r - r0), at + b, std::min<int32_t>(kBurdenItemPlanes, p - b), b});
      at += p;
    }
    r0 = r1;
    if (act.empty()) continue;   // nothing but rows of zeros: nothing is launched
    n_slabs++;
    n_items += (int64_t)items.size();
    n_planes += at;
    const size_t nact = act.size();
    std::vector<unsigned long long> tails(2 * nact);
    DevScratch d(c->stream);
    BurdenPlaneArgs pa{};
    pa.w = d.put(weights + (size_t)(r1 - rows) * (size_t)n, (size_t)rows * (size_t)n);
    pa.act = d.put(act.data(), nact);
    pa.nplanes = d.put(np.data(), nact);
    pa.pbase = d.put(pbase.data(), nact);
    pa.planes = d.take<uint32_t>((size_t)at * (size_t)W32p);
    pa.nact = (int64_t)nact;
    pa.n = n;
    pa.Wp = g.Wp;
    BurdenNullArgs na{};
    na.planes = pa.planes;
    na.masks = c->d_masks;
    na.items = d.put(items.data(), items.size());
    na.sums = d.take<unsigned long long>((size_t)rows * (size_t)g.Kpad);
    na.nitems = (int64_t)items.size();
    na.npt = (na.nitems + 3) / 4;
    na.nkt = (K + kSetPermTile - 1) / kSetPermTile;
    // one item tile per block while that makes at least ~8 blocks per resident block slot, more per block beyond (k_set_null's rule)
    const int64_t per = std::max<int64_t>(1, (na.npt * na.nkt) / ((int64_t)c->cus * 4 * 8));
    na.pgroups = (int)std::min<int64_t>((na.npt + per - 1) / per, 0x7fffffff / std::max(na.nkt, 1));
    na.W32p = W32p;
    na.Kpad = g.Kpad;
    na.K = K;
    BurdenFinishArgs fa{};
    fa.sums = na.sums;
    fa.act = pa.act;
    fa.observed = d.put(obs.data(), nact);
    fa.tails = d.take<unsigned long long>(2 * nact);
    fa.nact = (int64_t)nact;
    fa.Kpad = g.Kpad;
    fa.K = K;
    d.zero(na.sums, (size_t)rows * (size_t)g.Kpad);
    d.zero(fa.tails, 2 * nact);
    if (d.ok()) {
      d.e = launch_burden_planes(pa, c->stream);
      if (d.ok()) c->burden_launches++;
    }
    if (d.ok()) {
      d.e = launch_burden_null(na, c->stream);
      if (d.ok()) c->burden_launches++;
    }
    if (d.ok()) {
      d.e = launch_burden_finish(fa, c->stream);
      if (d.ok()) c->burden_launches++;
    }
    d.download(tails.data(), fa.tails, 2 * nact);
    if (null_sums && d.ok())   // the sums without the padding (a row of zeros: zeros)
      d.e = hipMemcpy2DAsync(null_sums + (size_t)(r1 - rows) * (size_t)K, (size_t)K * 8, na.sums, (size_t)g.Kpad * 8, (size_t)K * 8,
                             (size_t)rows, hipMemcpyDeviceToHost, c->stream);
    d.sync();
    d.release();
    if (!d.ok()) {
      (void)hipGetLastError();
      return fail(c, GCRE_ERR_DEVICE, who + ": " + hipGetErrorString(d.e));
    }
    for (size_t i = 0; i < nact; i++) {
      gcre_burden& o = out[(r1 - rows) + act[i]];
      o.n_ge = (int64_t)tails[2 * i];
      o.n_le = (int64_t)tails[2 * i + 1];
      o.p_upper = (double)o.n_ge / (double)K;
      o.p_lower = (double)o.n_le / (double)K;
    }
  }
  if (stats)
    fprintf(stderr, "burden rows=%lld planes=%lld items=%lld slabs=%lld iterations=%d entry_ms=%.3f\n", (long long)n_rows,
            (long long)n_planes, (long long)n_items, (long long)n_slabs, K,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  return GCRE_OK;
}

int64_t gcre_burden_launches(const gcre_ctx* c) { return c ? c->burden_launches : -1; }

// ---- per-gene best-path tally ----
gcre_gene_tally* gcre_gene_tally_create(gcre_ctx* c, int32_t n_slots, const int32_t* genes0, int64_t n_rows0, int32_t w0,
                                        const int32_t* genes1, int64_t n_rows1, int32_t w1) {
  if (!c) return nullptr;
  auto bad = [&](const std::string& m) -> gcre_gene_tally* {
    fail(c, GCRE_ERR_ARG, "gene tally: " + m);
    return nullptr;
  };
  if (n_slots < 1) return bad("n_slots must be >= 1");
  if (!genes0) { n_rows0 = 0; w0 = 0; }
  if (!genes1) { n_rows1 = 0; w1 = 0; }
  if (n_rows0 < 0 || n_rows1 < 0) return bad("negative row count");
  if ((genes0 && (w0 < 1 || w0 > kGeneWidthMax)) || (genes1 && (w1 < 1 || w1 > kGeneWidthMax)))
    return bad("a table's width must be 1.." + std::to_string(kGeneWidthMax));
  for (int64_t i = 0; i < n_rows0 * w0; i++)
    if (genes0[i] < -1 || genes0[i] >= n_slots) return bad("genes0 holds slot " + std::to_string(genes0[i]) + " outside -1.." + std::to_string(n_slots - 1));
  for (int64_t i = 0; i < n_rows1 * w1; i++)
    if (genes1[i] < -1 || genes1[i] >= n_slots) return bad("genes1 holds slot " + std::to_string(genes1[i]) + " outside -1.." + std::to_string(n_slots - 1));
  (void)hipSetDevice(c->device);
  gcre_gene_tally* t = new gcre_gene_tally();
  t->ctx = c;
  t->n_slots = n_slots;
  t->n_rows0 = n_rows0;
  t->n_rows1 = n_rows1;
  t->w0 = w0;
  t->w1 = w1;
  c->live_tallies.push_back(t);
  const size_t n = (size_t)n_slots, g0 = (size_t)(n_rows0 * w0), g1 = (size_t)(n_rows1 * w1);
  struct { void** p; size_t bytes; int fill; } tabs[] = {   // fill -1: the table comes from the host
      {(void**)&t->d_genes0, g0 * 4, -1}, {(void**)&t->d_genes1, g1 * 4, -1}, {(void**)&t->d_ck, n * 8, 0},
      {(void**)&t->d_cidx, n * 4, 0xff},  {(void**)&t->d_bkey, n * 8, 0},     {(void**)&t->d_bord, n * 8, 0xff},   // ordinal -1
      {(void**)&t->d_bsrc, n * 4, 0xff},  {(void**)&t->d_btrg, n * 4, 0xff},  {(void**)&t->d_bcases, n * 4, 0},
      {(void**)&t->d_bctrls, n * 4, 0}};
  hipError_t e = hipSuccess;
  for (auto& b : tabs)
    if (e == hipSuccess) e = hipMalloc(b.p, std::max<size_t>(b.bytes, 8));
  if (e == hipSuccess && g0) e = hipMemcpyAsync(t->d_genes0, genes0, g0 * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && g1) e = hipMemcpyAsync(t->d_genes1, genes1, g1 * 4, hipMemcpyHostToDevice, c->stream);
  for (auto& b : tabs)
    if (e == hipSuccess && b.fill >= 0) e = hipMemsetAsync(*b.p, b.fill, b.bytes, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (the host tables may go once the call returns)
  if (e != hipSuccess) {
    (void)hipGetLastError();
    gcre_gene_tally_free(t);
    fail(c, GCRE_ERR_DEVICE, std::string("gene tally: ") + hipGetErrorString(e));
    return nullptr;
  }
  t->last = c->stream;
  return t;
}

int gcre_join_set_tally(gcre_ctx* c, gcre_gene_tally* t) {
  if (!c) return GCRE_ERR_ARG;
  if (t && t->ctx != c) return fail(c, GCRE_ERR_ARG, "gene tally does not belong to this context");
  c->armed_tally = t;
  return GCRE_OK;
}

int gcre_process_paths_set_tally(gcre_ctx* c, int level, gcre_gene_tally* t) {
  if (!c) return GCRE_ERR_ARG;
  if (level < 0 || level > 5) return fail(c, GCRE_ERR_ARG, "gene tally: level index must be 0..5");
  if (t && t->ctx != c) return fail(c, GCRE_ERR_ARG, "gene tally does not belong to this context");
  c->pp_tally[level] = t;
  return GCRE_OK;
}

int gcre_gene_tally_read(gcre_gene_tally* t, double* score, int64_t* ordinal, int32_t* src, int32_t* trg, int32_t* cases,
                         int32_t* ctrls) {
  if (!t || !t->ctx) return GCRE_ERR_ARG;
  gcre_ctx* c = t->ctx;
  (void)hipSetDevice(c->device);
  if (t->last) HIP_TRY(c, hipStreamSynchronize(t->last));
  const size_t n = (size_t)t->n_slots;
  std::vector<uint64_t> key(n);
  HIP_TRY(c, hipMemcpy(key.data(), t->d_bkey, n * 8, hipMemcpyDeviceToHost));
  if (score)
    for (size_t g = 0; g < n; g++) score[g] = key[g] ? key_to_score(key[g]) : -std::numeric_limits<double>::infinity();
  if (ordinal) HIP_TRY(c, hipMemcpy(ordinal, t->d_bord, n * 8, hipMemcpyDeviceToHost));
  if (src) HIP_TRY(c, hipMemcpy(src, t->d_bsrc, n * 4, hipMemcpyDeviceToHost));
  if (trg) HIP_TRY(c, hipMemcpy(trg, t->d_btrg, n * 4, hipMemcpyDeviceToHost));
  if (cases) HIP_TRY(c, hipMemcpy(cases, t->d_bcases, n * 4, hipMemcpyDeviceToHost));
  if (ctrls) HIP_TRY(c, hipMemcpy(ctrls, t->d_bctrls, n * 4, hipMemcpyDeviceToHost));
  return GCRE_OK;
}

void gcre_gene_tally_free(gcre_gene_tally* t) {
  if (!t) return;
  if (gcre_ctx* c = t->ctx) {
    (void)hipSetDevice(c->device);
    if (t->last) (void)hipStreamSynchronize(t->last);
    if (c->armed_tally == t) c->armed_tally = nullptr;
    for (auto& p : c->pp_tally)
      if (p == t) p = nullptr;
    auto& v = c->live_tallies;
    v.erase(std::remove(v.begin(), v.end(), t), v.end());
  }
  for (void* p : {(void*)t->d_genes0, (void*)t->d_genes1, (void*)t->d_ck, (void*)t->d_cidx, (void*)t->d_bkey, (void*)t->d_bord,
                  (void*)t->d_bsrc, (void*)t->d_btrg, (void*)t->d_bcases, (void*)t->d_bctrls})
    if (p) (void)hipFree(p);
  delete t;
}

// ---- null exceedance counts ----
gcre_exceed* gcre_exceed_create(gcre_ctx* c, const double* thresholds, int32_t m) {
  if (!c) return nullptr;
  auto bad = [&](const std::string& msg) -> gcre_exceed* {
    fail(c, GCRE_ERR_ARG, "exceedance counts: " + msg);
    return nullptr;
  };
  if (!thresholds) return bad("NULL thresholds");
  if (m < 1 || m > kExceedMax) return bad("the number of thresholds must be 1.." + std::to_string(kExceedMax) + ", not " + std::to_string(m));
  for (int32_t i = 0; i < m; i++)
    if (thresholds[i] != thresholds[i]) return bad("threshold " + std::to_string(i) + " is NaN");
  (void)hipSetDevice(c->device);
  gcre_exceed* x = new gcre_exceed();
  x->ctx = c;
  x->m = m;
  x->thr.assign(thresholds, thresholds + m);
  x->order.resize((size_t)m);
  for (int32_t i = 0; i < m; i++) x->order[(size_t)i] = i;
  std::stable_sort(x->order.begin(), x->order.end(), [&](int32_t a, int32_t b) { return thresholds[a] < thresholds[b]; });
  // both images are monotone in the threshold: one order serves both.  Observed scores are compared as score keys
  // (gcre_kernels.hip: score_key); a zero threshold takes the key of -0.0, so that a score of either zero reaches it, and
  // -inf the smallest key a score can have
  std::vector<uint32_t> pat((size_t)m);
  std::vector<uint64_t> tkey((size_t)m);
  for (int32_t j = 0; j < m; j++) {
    double t = thresholds[x->order[(size_t)j]];
    pat[(size_t)j] = f32_threshold(t);
    if (t == 0) t = -0.0;
    uint64_t b;
    std::memcpy(&b, &t, 8);
    const uint64_t k = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    tkey[(size_t)j] = t > -std::numeric_limits<double>::infinity() ? k : 1;
  }
  c->live_exceeds.push_back(x);
  hipError_t e = hipMalloc((void**)&x->d_pat, (size_t)m * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&x->d_tkey, (size_t)m * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&x->d_hist, (size_t)m * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&x->d_ohist, (size_t)m * 8);
  if (e == hipSuccess) e = hipMemcpyAsync(x->d_pat, pat.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(x->d_tkey, tkey.data(), (size_t)m * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(x->d_hist, 0, (size_t)m * 8, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(x->d_ohist, 0, (size_t)m * 8, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (the vectors are locals)
  if (e != hipSuccess) {
    (void)hipGetLastError();
    gcre_exceed_free(x);
    fail(c, GCRE_ERR_DEVICE, std::string("exceedance counts: ") + hipGetErrorString(e));
    return nullptr;
  }
  return x;
}

int gcre_join_set_exceed(gcre_ctx* c, gcre_exceed* x) {
  if (!c) return GCRE_ERR_ARG;
  if (x && x->ctx != c) return fail(c, GCRE_ERR_ARG, "exceedance counts do not belong to this context");
  c->armed_exceed = x;
  return GCRE_OK;
}

int gcre_process_paths_set_exceed(gcre_ctx* c, int level, gcre_exceed* x) {
  if (!c) return GCRE_ERR_ARG;
  if (level < 0 || level > 5) return fail(c, GCRE_ERR_ARG, "exceedance counts: level index must be 0..5");
  if (x && x->ctx != c) return fail(c, GCRE_ERR_ARG, "exceedance counts do not belong to this context");
  c->pp_exceed[level] = x;
  return GCRE_OK;
}

int gcre_exceed_read(gcre_exceed* x, uint64_t* exceed, uint64_t* observed, int64_t* perms_counted, int64_t* paths_counted) {
  if (!x || !x->ctx) return GCRE_ERR_ARG;
  gcre_ctx* c = x->ctx;
  if (int rc = exceed_wait(c)) return rc;
  const size_t m = (size_t)x->m;
  std::vector<unsigned long long> h(m);
  for (int which = 0; which < 2; which++) {
    uint64_t* out = which ? observed : exceed;
    if (!out) continue;
    HIP_TRY(c, hipMemcpy(h.data(), which ? x->d_ohist : x->d_hist, m * 8, hipMemcpyDeviceToHost));
    uint64_t run = 0;
    for (size_t j = m; j-- > 0;) {   // a value in bin j reaches thresholds 0..j of the ascending order
      run += h[j];
      out[(size_t)x->order[j]] = run;
    }
  }
  if (perms_counted) *perms_counted = x->perms;
  if (paths_counted) *paths_counted = x->paths;
  return GCRE_OK;
}

int gcre_exceed_reset(gcre_exceed* x) {
  if (!x || !x->ctx) return GCRE_ERR_ARG;
  gcre_ctx* c = x->ctx;
  if (int rc = exceed_wait(c)) return rc;
  HIP_TRY(c, hipMemset(x->d_hist, 0, (size_t)x->m * 8));
  HIP_TRY(c, hipMemset(x->d_ohist, 0, (size_t)x->m * 8));
  if (x->d_pc) HIP_TRY(c, hipMemset(x->d_pc, 0, (size_t)x->m * (size_t)x->pc_stride * 4));
  std::fill(x->pc_load.begin(), x->pc_load.end(), 0);
  x->perms = x->paths = 0;
  return GCRE_OK;
}

int gcre_exceed_keep_perm_counts(gcre_exceed* x, int on) {
  if (!x || !x->ctx) return GCRE_ERR_ARG;
  gcre_ctx* c = x->ctx;
  if (int rc = exceed_alive(c, x)) return rc;
  if (int rc = exceed_wait(c)) return rc;
  if (!on) {
    if (x->d_pc) (void)hipFree(x->d_pc);
    x->d_pc = nullptr;
    x->pc_stride = 0;
    x->pc_load.clear();
    return GCRE_OK;
  }
  if (x->d_pc) return GCRE_OK;
  if (x->perms != 0 || x->paths != 0)
    return fail(c, GCRE_ERR_ARG, "exceedance counts: per-permutation counts cannot be switched on after something was counted (" +
                                 std::to_string(x->perms) + " permutations, " + std::to_string(x->paths) + " joined paths): reset first");
  const int64_t K = c->g.K;
  if (K <= 0) return fail(c, GCRE_ERR_ARG, "exceedance counts: per-permutation counts need a context with permutations (it has 0 iterations)");
  if ((int64_t)x->m * K > kExceedPermCells)
    return fail(c, GCRE_ERR_ARG, "exceedance counts: per-permutation counts of " + std::to_string(x->m) + " thresholds x " + std::to_string(K) +
                                 " iterations exceed the limit of 2^26 = 67108864 cells (256 MB)");
  const size_t bytes = (size_t)x->m * (size_t)c->g.Kpad * 4;
  hipError_t e = hipMalloc((void**)&x->d_pc, bytes);
  if (e == hipSuccess) e = hipMemset(x->d_pc, 0, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (x->d_pc) (void)hipFree(x->d_pc);
    x->d_pc = nullptr;
    return fail(c, GCRE_ERR_DEVICE, std::string("exceedance counts: per-permutation counts: ") + hipGetErrorString(e));
  }
  x->pc_stride = c->g.Kpad;
  x->pc_load.assign((size_t)(c->g.Kpad / kPermTileMax), 0);
  return GCRE_OK;
}

int gcre_exceed_read_perm_counts(gcre_exceed* x, uint64_t* out) {
  if (!x || !x->ctx) return GCRE_ERR_ARG;
  gcre_ctx* c = x->ctx;
  if (!x->d_pc) return fail(c, GCRE_ERR_ARG, "exceedance counts: the object keeps no per-permutation counts (gcre_exceed_keep_perm_counts)");
  if (!out) return fail(c, GCRE_ERR_ARG, "exceedance counts: NULL output");
  if (int rc = exceed_wait(c)) return rc;
  const size_t m = (size_t)x->m, K = (size_t)c->g.K, stride = (size_t)x->pc_stride;
  std::vector<uint32_t> h(m * stride);
  HIP_TRY(c, hipMemcpy(h.data(), x->d_pc, m * stride * 4, hipMemcpyDeviceToHost));
  std::vector<uint64_t> run(K, 0);
  for (size_t j = m; j-- > 0;) {   // as gcre_exceed_read: a value in bin j reaches thresholds 0..j of the ascending order
    const uint32_t* row = h.data() + j * stride;
    uint64_t* dst = out + (size_t)x->order[j] * K;
    for (size_t r = 0; r < K; r++) {
      run[r] += row[r];
      dst[r] = run[r];
    }
  }
  return GCRE_OK;
}

// Step-down max-T.  Set j is the joined path whose observed score is threshold j: its null values, found
// in the bins of the thresholds strictly below it, are what the join's per-permutation counts hold too many of once the
// better rows are taken out of the family.
int gcre_exceed_stepdown(gcre_exceed* x, const gcre_set_input* in, int64_t* n_ge) {
  if (!x || !x->ctx) return GCRE_ERR_ARG;
  gcre_ctx* c = x->ctx;
  if (int rc = exceed_alive(c, x)) return rc;
  if (!in || !n_ge) return fail(c, GCRE_ERR_ARG, "stepdown: NULL argument");
  if (!x->d_pc)
    return fail(c, GCRE_ERR_ARG, "stepdown: the object keeps no per-permutation counts (gcre_exceed_keep_perm_counts)");
  const Geometry& g = c->g;
  const int K = g.K, M = g.method, m = x->m;
  if (x->perms != K || x->paths <= 0)
    return fail(c, GCRE_ERR_ARG, "stepdown: the object must hold exactly one full pass of one join (" + std::to_string(x->perms) +
                                     " permutations of " + std::to_string(x->paths) + " joined paths counted, the context has " +
                                     std::to_string(K) + " iterations)");
  if (in->n_sets != m)
    return fail(c, GCRE_ERR_ARG, "stepdown: " + std::to_string(in->n_sets) + " sets for " + std::to_string(m) + " thresholds");
  for (int j = 0; j < m; j++)
    if (!std::isfinite(x->thr[(size_t)j])) return fail(c, GCRE_ERR_ARG, "stepdown: threshold " + std::to_string(j) + " is not finite");
  if (int rc = check_sets(c, in, "stepdown")) return rc;
  for (int64_t s = 0; s < m; s++)
    if (!set_is_valid(in, s)) return fail(c, GCRE_ERR_ARG, "stepdown: set " + std::to_string(s) + " has an NA member");
  if (int rc = exceed_wait(c)) return rc;

  // the host stage of gcre_score_sets: per set its union rows and counts
  const int Wp = g.Wp;
  const size_t RW = (size_t)M * Wp;
  const SetUnion un(g.W, g.n, g.n_cases);
  std::vector<uint64_t> urows((size_t)m * RW, 0);
  std::vector<int32_t> cnt((size_t)m * 4, 0);   // cases_pos, ctrls_pos, cases_neg, ctrls_neg
  std::vector<uint32_t> tot((size_t)m * M);
  for (int64_t s = 0; s < m; s++) {
    int32_t* k = cnt.data() + 4 * s;
    un.build(in, s, urows.data() + (size_t)s * RW, (size_t)Wp, M == 2, k);
    tot[(size_t)s * M] = (uint32_t)(k[0] + k[1]);
    if (M == 2) tot[(size_t)s * M + 1] = (uint32_t)(k[2] + k[3]);
  }
  // cap[j] = the last sorted index strictly below threshold j (compared as f64: tied rows do not exclude one another)
  std::vector<int32_t> cap((size_t)m);
  for (int b = 0, first = 0; b < m; b++) {
    if (x->thr[(size_t)x->order[(size_t)b]] > x->thr[(size_t)x->order[(size_t)first]]) first = b;
    cap[(size_t)x->order[(size_t)b]] = first - 1;
  }

  (void)hipSetDevice(c->device);
  const size_t stride = (size_t)x->pc_stride, cells = (size_t)m * stride;
  std::vector<double> obs((size_t)m);
  std::vector<uint32_t> got((size_t)m + 1, 0);
  int64_t off_set = -1;   // the first set whose observed score is not its threshold, bit for bit
  DevScratch d(c->stream);
  const uint64_t* d_rows = d.put(urows.data(), urows.size());
  const int32_t* d_cnt = d.put(cnt.data(), cnt.size());
  const uint32_t* d_tot = d.put(tot.data(), tot.size());
  const int32_t* d_cap = d.put(cap.data(), (size_t)m);
  double* d_obs = d.take<double>((size_t)m);
  uint32_t* d_out = d.take<uint32_t>((size_t)m + 1);   // n_ge per sorted threshold, then the bad counter
  if (d.ok()) d.e = launch_set_observed(d_cnt, m, M, c->d_dvt, d_obs, c->stream);
  d.download(obs.data(), d_obs, (size_t)m);
  d.sync();
  for (int64_t s = 0; d.ok() && s < m && off_set < 0; s++)
    if (std::memcmp(&obs[(size_t)s], &x->thr[(size_t)s], 8) != 0) off_set = s;
  if (d.ok() && off_set < 0) {
    uint32_t* d_E = d.take<uint32_t>(cells);
    d.zero(d_E, cells);
    d.zero(d_out, (size_t)m + 1);
    StepdownArgs a{};
    fill_set_launch(a, c, d_rows, d_tot, m);
    a.pat = x->d_pat;
    a.cap = d_cap;
    a.E = d_E;
    a.m = m;
    a.stride = (int)stride;
    const StepdownFinishArgs f{x->d_pc, d_E, d_out, d_out + m, m, (int)stride, K};
    if (d.ok()) d.e = launch_stepdown_null(a, M, c->stream);
    if (d.ok()) c->stepdown_launches++;
    if (d.ok()) d.e = launch_stepdown_finish(f, c->stream);
    if (d.ok()) c->stepdown_launches++;
    d.download(got.data(), d_out, (size_t)m + 1);
    d.sync();
  }
  d.release();   // (before the error state is cleared, as ever)
  if (!d.ok()) {
    (void)hipGetLastError();
    return fail(c, GCRE_ERR_DEVICE, std::string("stepdown: ") + hipGetErrorString(d.e));
  }
  if (off_set >= 0) {
    char buf[256];
    std::snprintf(buf, sizeof buf, ": its observed score is %.17g, threshold %lld is %.17g (the rows must be the rows the thresholds came from)",
                  obs[(size_t)off_set], (long long)off_set, x->thr[(size_t)off_set]);
    return fail(c, GCRE_ERR_ARG, "stepdown: set " + std::to_string(off_set) + buf);
  }
  if (got[(size_t)m] != 0)
    return fail(c, GCRE_ERR_ASSERT, "assertion: stepdown: the sets are not distinct joined paths of the counted join (" +
                                        std::to_string(got[(size_t)m]) + " permutations count more top rows than joined paths at a threshold)");
  for (int b = 0; b < m; b++) n_ge[(size_t)x->order[(size_t)b]] = (int64_t)got[(size_t)b];
  return GCRE_OK;
}

int64_t gcre_stepdown_launches(const gcre_ctx* c) { return c ? c->stepdown_launches : -1; }

// ---- hit lists ----
gcre_hits* gcre_hits_create(gcre_ctx* c, double cutoff, int64_t cap) {
  if (!c) return nullptr;
  auto bad = [&](const std::string& msg) -> gcre_hits* {
    fail(c, GCRE_ERR_ARG, "hit list: " + msg);
    return nullptr;
  };
  if (cutoff != cutoff) return bad("the cut-off is NaN");
  if (cap < 1 || cap > kHitsCapMax) return bad("cap must be 1.." + std::to_string(kHitsCapMax) + " (2^26), not " + std::to_string(cap));
  (void)hipSetDevice(c->device);
  gcre_hits* h = new gcre_hits();
  h->ctx = c;
  h->cutoff = cutoff;
  h->cap = cap;
  // the threshold key as gcre_exceed_create makes its own: a zero cut-off takes the key of -0.0, so that a score of either
  // zero reaches it, and -inf the smallest key a score can have
  double t = cutoff == 0 ? -0.0 : cutoff;
  uint64_t b;
  std::memcpy(&b, &t, 8);
  const uint64_t k = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  h->tkey = t > -std::numeric_limits<double>::infinity() ? k : 1;
  c->live_hits.push_back(h);
  hipError_t e = hipMalloc((void**)&h->d_cursor, 8);
  if (e == hipSuccess) e = hipMalloc(&h->d_rec, (size_t)cap * 32);
  if (e == hipSuccess) e = hipMemsetAsync(h->d_cursor, 0, 8, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    gcre_hits_free(h);
    fail(c, GCRE_ERR_DEVICE, std::string("hit list: ") + hipGetErrorString(e));
    return nullptr;
  }
  return h;
}

int gcre_join_set_hits(gcre_ctx* c, gcre_hits* h) {
  if (!c) return GCRE_ERR_ARG;
  if (h && hits_alive(c, h) != GCRE_OK) return c->last_code;
  c->armed_hits = h;
  return GCRE_OK;
}

int gcre_process_paths_set_hits(gcre_ctx* c, int level, gcre_hits* h) {
  if (!c) return GCRE_ERR_ARG;
  if (level < 0 || level > 5) return fail(c, GCRE_ERR_ARG, "hit list: level index must be 0..5");
  if (h && hits_alive(c, h) != GCRE_OK) return c->last_code;
  c->pp_hits[level] = h;
  return GCRE_OK;
}

int gcre_hits_count(gcre_hits* h, int64_t* found, int64_t* paths) {
  if (!h || !h->ctx) return GCRE_ERR_ARG;
  gcre_ctx* c = h->ctx;
  if (int rc = exceed_wait(c)) return rc;
  if (found) {
    unsigned long long n = 0;
    HIP_TRY(c, hipMemcpy(&n, h->d_cursor, 8, hipMemcpyDeviceToHost));
    *found = (int64_t)n;
  }
  if (paths) *paths = h->paths;
  return GCRE_OK;
}

int gcre_hits_read(gcre_hits* h, int64_t n, double* score, int64_t* ordinal, int32_t* src, int32_t* trg, int32_t* cases,
                   int32_t* ctrls) {
  if (!h || !h->ctx) return GCRE_ERR_ARG;
  gcre_ctx* c = h->ctx;
  int64_t found = 0;
  if (int rc = gcre_hits_count(h, &found, nullptr)) return rc;
  if (n != found)
    return fail(c, GCRE_ERR_ARG, "hit list: n = " + std::to_string(n) + ", the list found " + std::to_string(found) + " (gcre_hits_count)");
  if (found > h->cap)
    return fail(c, GCRE_ERR_RANGE, "hit list: " + std::to_string(found) + " joined paths reach the cut-off, the list holds " +
                                       std::to_string(h->cap) + ": reset it or make a larger one, and collect again");
  const size_t m = (size_t)found;
  if (m == 0) return GCRE_OK;
  std::vector<int64_t> ord(m);
  std::vector<uint64_t> key(m);
  HIP_TRY(c, hipMemcpy(ord.data(), h->ord(), m * 8, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(key.data(), h->key(), m * 8, hipMemcpyDeviceToHost));
  // best first: the key with the two zeros made one (they are equal as doubles) descending, then the ordinal ascending
  auto tie = [](uint64_t k) { return k == kKeyMinusZero ? kKeyPlusZero : k; };
  std::vector<uint32_t> perm(m);
  for (size_t i = 0; i < m; i++) perm[i] = (uint32_t)i;
  std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
    const uint64_t ka = tie(key[a]), kb = tie(key[b]);
    return ka != kb ? ka > kb : ord[a] < ord[b];
  });
  if (score)
    for (size_t i = 0; i < m; i++) score[i] = key_to_score(key[perm[i]]);
  if (ordinal)
    for (size_t i = 0; i < m; i++) ordinal[i] = ord[perm[i]];
  std::vector<int32_t> f(m);
  int32_t* outs[4] = {src, trg, cases, ctrls};
  for (int k = 0; k < 4; k++) {
    if (!outs[k]) continue;
    HIP_TRY(c, hipMemcpy(f.data(), h->field(k), m * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < m; i++) outs[k][i] = f[perm[i]];
  }
  return GCRE_OK;
}

int gcre_hits_reset(gcre_hits* h) {
  if (!h || !h->ctx) return GCRE_ERR_ARG;
  gcre_ctx* c = h->ctx;
  if (int rc = exceed_wait(c)) return rc;
  HIP_TRY(c, hipMemset(h->d_cursor, 0, 8));
  h->paths = 0;
  return GCRE_OK;
}

int64_t gcre_hits_launches(const gcre_ctx* c) { return c ? c->hits_launches : -1; }

void gcre_hits_free(gcre_hits* h) {
  if (!h) return;
  if (gcre_ctx* c = h->ctx) {
    (void)exceed_wait(c);
    if (c->armed_hits == h) c->armed_hits = nullptr;
    for (auto& p : c->pp_hits)
      if (p == h) p = nullptr;
    auto& v = c->live_hits;
    v.erase(std::remove(v.begin(), v.end(), h), v.end());
  }
  for (void* p : {(void*)h->d_cursor, h->d_rec})
    if (p) (void)hipFree(p);
  delete h;
}

void gcre_exceed_free(gcre_exceed* x) {
  if (!x) return;
  if (gcre_ctx* c = x->ctx) {
    (void)exceed_wait(c);
    if (c->armed_exceed == x) c->armed_exceed = nullptr;
    for (auto& p : c->pp_exceed)
      if (p == x) p = nullptr;
    auto& v = c->live_exceeds;
    v.erase(std::remove(v.begin(), v.end(), x), v.end());
  }
  for (void* p : {(void*)x->d_pat, (void*)x->d_tkey, (void*)x->d_hist, (void*)x->d_ohist, (void*)x->d_pc})
    if (p) (void)hipFree(p);
  delete x;
}

}  // extern "C"

// gcre_host_weighted.hip -- gcre_generate_weighted_masks on a context and the host-only gcre_weighted_thresholds (DESIGN.md
// §3.23).  The plan -- strata, refusals, thresholds, expected attempts -- is gcre_weighted.h's; here are the uploads, the two
// launches of gcre_weighted.hip and what follows a refusal.  Host code only.
#include "gcre_host.h"
#include "gcre_weighted.h"

extern "C" {

int gcre_weighted_thresholds(int32_t n, int32_t n_cases, const double* odds, const int32_t* stratum, int32_t n_strata,
                             uint32_t* thr_out, double* expected_attempts_out) {
  const std::string who = "weighted_thresholds";
  if (!thr_out) return fail(nullptr, GCRE_ERR_ARG, who + ": NULL argument (thr_out)");
  gcre_weighted::WeightedPlan pl;
  std::string msg;
  if (int rc = gcre_weighted::weighted_plan(n, n_cases, odds, stratum, n_strata, who, pl, msg)) return fail(nullptr, rc, msg);
  std::copy(pl.thr.begin(), pl.thr.end(), thr_out);
  if (expected_attempts_out) std::copy(pl.expected.begin(), pl.expected.end(), expected_attempts_out);
  return GCRE_OK;
}

int gcre_generate_weighted_masks(gcre_ctx* c, uint64_t seed, const double* odds, const int32_t* stratum, int32_t n_strata,
                                 int64_t max_attempts, uint32_t* attempts_out) {
  if (!c) return GCRE_ERR_ARG;
  const std::string who = "generate_weighted_masks";
  const Geometry& g = c->g;
  gcre_weighted::WeightedPlan pl;
  std::string msg;
  uint32_t cap = 0;
  if (int rc = gcre_weighted::weighted_plan(g.n, g.n_cases, odds, stratum, n_strata, who, pl, msg)) return fail(c, rc, msg);
  if (int rc = gcre_weighted::weighted_cap(max_attempts, who, cap, msg)) return fail(c, rc, msg);
  if (int rc = gcre_weighted::weighted_plan_fits(pl, cap, who, msg)) return fail(c, rc, msg);
  (void)hipSetDevice(c->device);
  if (g.K == 0) { c->have_perms = true; return GCRE_OK; }
  const int S = pl.ns;
  // per stratum, one behind the other: the columns and their thresholds
  std::vector<uint32_t> soff((size_t)S + 1, 0u);
  for (int s = 0; s < S; s++) soff[(size_t)s + 1] = soff[(size_t)s] + pl.size_of[(size_t)s];
  std::vector<int32_t> cols((size_t)g.n + 1);   // (never empty)
  std::vector<uint32_t> cthr((size_t)g.n + 1);
  {
    std::vector<uint32_t> at(soff.begin(), soff.end() - 1);
    for (int32_t q = 0; q < g.n; q++) {
      const uint32_t i = at[(size_t)(stratum ? stratum[q] : 0)]++;
      cols[i] = q;
      cthr[i] = pl.thr[(size_t)q];
    }
  }
  std::vector<uint32_t> att(attempts_out ? (size_t)S * (size_t)g.K : 0);
  unsigned int left = 0;
  {
    DevScratch d(c->stream);
    WeightedArgs a{};
    a.seed1 = gcre_weighted::wt_seed(seed);
    a.cols = d.put(cols.data(), cols.size());
    a.cthr = d.put(cthr.data(), cthr.size());
    a.soff = d.put(soff.data(), soff.size());
    a.cases_in = d.put(pl.cases_in.data(), (size_t)S);
    a.att = d.take<uint32_t>((size_t)S * (size_t)g.K);
    a.left = d.take<unsigned int>(1);
    d.zero(a.left, 1);
    a.cap = cap;
    a.stratum = stratum ? d.put(stratum, (size_t)g.n) : nullptr;
    a.thr = d.put(pl.thr.data(), (size_t)g.n);
    a.masks = c->d_masks;
    a.S = S;
    a.K = g.K;
    a.n = g.n;
    a.W32p = 2 * g.Wp;
    a.Kpad = g.Kpad;
    if (d.ok()) {
      d.e = launch_weighted_search(a, c->stream);
      if (d.ok()) c->weighted_launches++;
    }
    d.download(&left, a.left, 1);
    d.sync();
    if (d.ok() && left == 0) {
      d.e = launch_weighted_write(a, c->stream);
      if (d.ok()) c->weighted_launches++;
      if (attempts_out) d.download(att.data(), a.att, att.size());
      d.sync();
    } else if (d.ok()) {   // the permutations behind the pairs, for the message
      att.resize((size_t)S * (size_t)g.K);
      d.download(att.data(), a.att, att.size());
      d.sync();
    }
    if (!d.ok()) return fail(c, GCRE_ERR_DEVICE, who + ": " + hipGetErrorString(d.e));
  }
  if (left != 0) {
    long long perms = 0;
    for (int r = 0; r < g.K; r++) {
      bool none = false;
      for (int s = 0; s < S; s++) none = none || att[(size_t)s * (size_t)g.K + (size_t)r] == gcre_weighted::kWeightedNone;
      perms += none ? 1 : 0;
    }
    return fail(c, GCRE_ERR_RANGE, gcre_weighted::weighted_left_message(who, perms, g.K, cap));
  }
  if (attempts_out)   // [S][K] on the device, [K][n_strata] for the caller
    for (int r = 0; r < g.K; r++)
      for (int s = 0; s < S; s++) attempts_out[(size_t)r * (size_t)S + (size_t)s] = att[(size_t)s * (size_t)g.K + (size_t)r];
  if (int rc = build_transposed_masks(c)) return rc;
  c->have_perms = true;
  return GCRE_OK;
}

int64_t gcre_weighted_launches(const gcre_ctx* c) { return c ? c->weighted_launches : -1; }

}  // extern "C"

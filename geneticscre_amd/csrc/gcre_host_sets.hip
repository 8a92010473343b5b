// gcre_host_sets.hip -- the set scores of include/gcre_hip.h on a context: what gcre_set_stage.h
// declares -- the checks, the device stage behind k_set_observed and k_set_null (gcre_sets.hip) and the driver that every
// entry with a stage of its own goes through -- and the two entries without one, gcre_score_sets and gcre_score_sets_given
// (gcre_given.hip).  Host code only.
#include "gcre_set_stage.h"

int gcre_host::check_sets(gcre_ctx* c, const gcre_set_input* in, const std::string& who) {
  if (!c->have_table || !c->d_dvt) return fail(c, GCRE_ERR_ASSERT, "assertion: " + who + " needs a value table");
  if (c->g.K > 0 && !c->have_perms)
    return fail(c, GCRE_ERR_ASSERT, "assertion: " + who + " needs the permutation masks (iterations > 0, none set)");
  std::string msg;
  int rc = check_set_shape(in, c->g.n, who, msg);
  if (rc == GCRE_OK) rc = check_set_members(in, who, msg);
  return rc == GCRE_OK ? GCRE_OK : fail(c, rc, msg);
}

void gcre_host::score_set_rows(gcre_ctx* c, DevScratch& d, const uint64_t* d_rows, const int32_t* d_cnt, const uint32_t* d_tot,
                               const SetStageBufs& b, uint32_t* d_fam, int64_t V, double* obs, unsigned long long* ge,
                               uint32_t* fam_out, int64_t* launches) {
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

void gcre_host::init_set_record(gcre_set_score& o, int64_t set, bool valid) {
  std::memset(&o, 0, sizeof o);
  o.set = set;
  o.score = o.pvalue = std::numeric_limits<double>::quiet_NaN();
  o.valid = valid ? 1 : 0;
}

void gcre_host::fill_set_counts(gcre_set_score& o, const int32_t* k) {
  o.cases_pos = k[0];
  o.ctrls_pos = k[1];
  o.cases_neg = k[2];
  o.ctrls_neg = k[3];
  o.cases = o.cases_pos + o.cases_neg;
  o.ctrls = o.ctrls_pos + o.ctrls_neg;
}

void gcre_host::fill_set_record(gcre_set_score& o, const int32_t* k, double obs, unsigned long long ge, int K) {
  if (k) fill_set_counts(o, k);
  o.score = obs;
  o.n_ge = (int64_t)ge;
  o.pvalue = K > 0 ? (double)o.n_ge / (double)K : std::numeric_limits<double>::quiet_NaN();
}

int gcre_host::score_sets_common(gcre_ctx* c, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out,
                                 float* family_max, const std::string& who, SetStage* stage) {
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
  if (stage)
    if (int rc = stage->check(c, in, who)) return rc;

  // the host stage: per valid set the OR of its (+) members and of its (-) members (method 1: of all of them), within the
  // n patients, and their counts; the device rows are [valid set][M][Wp] words, the dword view k_set_null reads
  const int Wp = g.Wp;
  const size_t RW = (size_t)M * Wp;
  const SetUnion un(g.W, g.n, g.n_cases);
  std::vector<int64_t> vset;     // the valid sets, in input order
  std::vector<uint64_t> urows;
  std::vector<int32_t> cnt;      // [valid][4] cases_pos, ctrls_pos, cases_neg, ctrls_neg
  std::vector<uint32_t> tot;     // [valid][M] carriers per half
  for (int64_t s = 0; s < S; s++) {
    gcre_set_score& o = out[s];
    init_set_record(o, s, set_is_valid(in, s));
    if (!o.valid) continue;
    const size_t v = vset.size();
    vset.push_back(s);
    urows.resize((v + 1) * RW, 0);
    int32_t k[4];
    un.build(in, s, urows.data() + v * RW, (size_t)Wp, M == 2, k);
    fill_set_counts(o, k);   // (they stand whatever the device does)
    cnt.insert(cnt.end(), k, k + 4);
    tot.push_back((uint32_t)(k[0] + k[1]));
    if (M == 2) tot.push_back((uint32_t)(k[2] + k[3]));
  }
  if (family_max) std::fill(family_max, family_max + K, 0.0f);
  if (stage) stage->defaults(in, out);
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
  if (d.ok()) {
    for (int64_t v = 0; v < V; v++) fill_set_record(out[vset[(size_t)v]], nullptr, obs[(size_t)v], ge[(size_t)v], K);
    if (fam) std::memcpy(family_max, fbits.data(), (size_t)K * 4);
    if (stage && stage->runs(c)) stage->run({c, d, in, vset, d_rows, d_tot, d_obs, cnt, obs, ge});
  }
  if (!d.ok()) return fail(c, GCRE_ERR_DEVICE, who + ": " + hipGetErrorString(d.e));
  return GCRE_OK;
}

extern "C" {

int gcre_score_sets(gcre_ctx* c, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out,
                    float* family_max) {
  return score_sets_common(c, in, out, cap, n_out, family_max, "score_sets", nullptr);
}

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
  std::vector<signed char> valid((size_t)S, -1);   // -1: not looked at yet
  std::vector<int64_t> ventry, vw, vg;
  for (int64_t i = 0; i < n_which; i++) {
    const int64_t s = which ? which[i] : i;
    if (valid[(size_t)s] < 0) valid[(size_t)s] = set_is_valid(in, s) ? 1 : 0;
    init_set_record(out[i], s, valid[(size_t)s] != 0);
    if (!valid[(size_t)s]) continue;
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
    for (int64_t v = 0; v < nv; v++)
      fill_set_record(out[ventry[(size_t)(v0 + v)]], cnt.data() + 4 * v, obs[(size_t)v], ge[(size_t)v], K);
  }
  if (!d.ok()) return fail(c, GCRE_ERR_DEVICE, std::string("score_sets_given: ") + hipGetErrorString(d.e));
  if (std::getenv("GCRE_GIVEN_STATS"))   // (tools/given_time.py)
    fprintf(stderr, "given entries=%lld launched=%lld slab=%lld slabs=%lld\n", (long long)n_which, (long long)V, (long long)slab,
            (long long)slabs);
  if (fam) std::memcpy(family_max, fbits.data(), (size_t)K * 4);
  return GCRE_OK;
}

int64_t gcre_given_launches(const gcre_ctx* c) { return c ? c->given_launches : -1; }

}  // extern "C"

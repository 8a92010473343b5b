// gcre_host_stats.hip -- the entry points of include/gcre_hip.h that use a context but neither the join driver nor the set
// scores' driver (gcre_host_sets.hip and the stage files beside it): generated permutation masks, decorated p-values
// (gcre_decorated.hip), carrier overlaps (gcre_overlap.hip), greedy clumps (gcre_clump.hip), carrier tallies per patient
// (gcre_patients.hip) and burden tests of per-patient weights (gcre_burden.hip), and the per-gene tally (gcre_genes.hip), the
// null exceedance counts (gcre_exceed.hip, gcre_stepdown.hip) and the hit lists (gcre_hits.hip) as objects.  What a join does
// with an armed tally, armed counts or an armed list -- check_tally, fold_genes, count_exceed, collect_hits -- is in
// gcre_host.hip.  Host code only.
#include "gcre_set_stage.h"   // check_sets, fill_set_launch and f32_threshold for gcre_exceed_stepdown
#include "gcre_clumporder.h"

namespace {

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

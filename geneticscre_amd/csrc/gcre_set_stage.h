// gcre_set_stage.h -- what the host files of the set scores share (hipcc only): gcre_host_sets.hip defines the checks, the
// device stage of gcre_score_sets and its driver, score_sets_common; every entry that adds a statistic of its own to the
// records (gcre_host_family.hip, _minp, _compete, _steps, _subsample, _sequential, _seq_prefix, _strata) hands the driver one SetStage.
// Nothing here is part of the ABI.
#pragma once
#include "gcre_host.h"
#include "gcre_setlists.h"
#include "gcre_threshold.h"   // f32_threshold

namespace gcre_host __attribute__((visibility("hidden"))) {

// What gcre_score_sets and gcre_exceed_stepdown refuse before anything is launched (`who` opens the message): a context
// without a table or without masks, then the shape of the set list, then every set's members and signs
int check_sets(gcre_ctx* c, const gcre_set_input* in, const std::string& who);

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
                    int64_t* launches);

// One record before the device has run: its set, NaN score and p-value, valid or not, everything else zero -- what an invalid
// set keeps.  And what a valid one gets: the counts k = cases_pos, ctrls_pos, cases_neg, ctrls_neg (fill_set_counts; or
// through fill_set_record, k nullptr: they stand as they are), the observed score and its count among K permutations.
void init_set_record(gcre_set_score& o, int64_t set, bool valid);
void fill_set_counts(gcre_set_score& o, const int32_t* k);
void fill_set_record(gcre_set_score& o, const int32_t* k, double obs, unsigned long long ge, int K);

// What score_sets_common has on the device and on the host once score_set_rows has returned: the valid sets in input order
// (vset), their union rows [V][M][Wp], carrier totals [V][M] and observed scores [V] on the device; their counts [V][4],
// observed scores and counts among the permutations on the host.
struct SetScoreRun {
  gcre_ctx* c;
  DevScratch& d;
  const gcre_set_input* in;
  const std::vector<int64_t>& vset;
  const uint64_t* d_rows;
  const uint32_t* d_tot;
  const double* d_obs;
  const std::vector<int32_t>& cnt;
  const std::vector<double>& obs;
  const std::vector<unsigned long long>& ge;
};

// A statistic computed behind gcre_score_sets on the same sets.  The driver calls check after its own checks and before
// anything is written or launched (it refuses through fail() and keeps the plan it computed); defaults after the records are
// initialised (out[s].valid stands): what invalid sets, a list without a valid set and a context without permutations or
// draws keep; and, with a valid set and where runs() says so, run behind score_set_rows -- errors stay in `d`.
struct SetStage {
  virtual int check(gcre_ctx* c, const gcre_set_input* in, const std::string& who) = 0;
  virtual void defaults(const gcre_set_input* in, const gcre_set_score* out) = 0;
  virtual bool runs(const gcre_ctx* c) const = 0;
  virtual void run(const SetScoreRun& r) = 0;
};

// gcre_score_sets (`stage` nullptr) and every entry that adds a stage to it: the same checks, host stage and device stage
int score_sets_common(gcre_ctx* c, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out, float* family_max,
                      const std::string& who, SetStage* stage);

// Reads `nrows` device rows of `src_stride` elements back, `chunk_rows` at a time through `stage` (grown as needed), one
// synchronisation per chunk, and copies the first `live` elements of row r to dst + row_of(r) * dst_stride + col0.  Errors
// stay in `d`; nothing is copied from a chunk that did not arrive.
template <typename T, typename RowOf>
void fetch_rows(DevScratch& d, const T* src, int64_t nrows, int64_t src_stride, int64_t chunk_rows, std::vector<T>& stage, T* dst,
                int64_t dst_stride, int64_t col0, int64_t live, RowOf row_of) {
  const size_t need = (size_t)std::min(chunk_rows, nrows) * (size_t)src_stride;
  if (stage.size() < need) stage.resize(need);
  for (int64_t r0 = 0; d.ok() && r0 < nrows; r0 += chunk_rows) {
    const int64_t nr = std::min(chunk_rows, nrows - r0);
    d.download(stage.data(), src + (size_t)r0 * (size_t)src_stride, (size_t)nr * (size_t)src_stride);
    d.sync();
    if (!d.ok()) return;
    for (int64_t r = 0; r < nr; r++)
      std::memcpy(dst + (size_t)row_of(r0 + r) * (size_t)dst_stride + (size_t)col0, stage.data() + (size_t)r * (size_t)src_stride,
                  (size_t)live * sizeof(T));
  }
}

}  // namespace gcre_host

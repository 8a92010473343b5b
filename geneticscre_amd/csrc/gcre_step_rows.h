// gcre_step_rows.h -- the step rows of the variable-threshold and multi-hit tests on the device (hipcc only; DESIGN.md §3.18,
// §3.20, §3.25): what gcre_host_steps.hip (the resident entries) and gcre_host_seq_prefix.hip (the sequential ones) share.
// StepRows sizes the slabs of whole valid sets (gcre_prefix.h), uploads the caller's set list once and per slab builds the
// rows (k_prefix_rows or k_dose_rows), scores them (k_set_observed), takes every set's best step (k_prefix_pick) and turns the
// picks into the variant's records (gcre_steps.h).  What runs behind the picks -- k_prefix_null, or the sequential loop -- is
// the stage's.  Nothing here is part of the ABI.
#pragma once
#include "gcre_set_stage.h"
#include "gcre_steps.h"

namespace gcre_host __attribute__((visibility("hidden"))) {

static_assert(sizeof(PrefixPick) == 32, "the layout the host reads");

// The one rows launch of a variant over the slab in `a`
inline hipError_t launch_rows(const gcre_steps::PrefixRows&, const PrefixArgs& a, int method, hipStream_t stream) {
  return launch_prefix_rows(a, method, stream);
}
inline hipError_t launch_rows(const gcre_steps::DoseRows& v, const PrefixArgs& a, int method, hipStream_t stream) {
  DoseArgs b{};
  b.gene_rows = a.gene_rows;
  b.set_off = a.set_off;
  b.members = a.members;
  b.signs = a.signs;
  b.which = a.which;
  b.rows = a.rows;   // slot e: rows [e L, e L + L), the running sum of row0
  b.cnt = a.cnt;
  b.levels = gcre_dose::pack_levels(v.levels, v.n_levels);
  b.nslots = a.nslots;
  b.n_levels = v.n_levels;
  b.W2 = a.W2;
  b.W32p = a.W32p;
  b.n_patients = a.n_patients;
  b.n_cases = a.n_cases;
  return launch_dose_rows(b, method, stream);
}

template <typename Variant>
struct StepRows {
  const Variant& v;
  gcre_ctx* const c;
  DevScratch& d;
  const std::vector<int64_t>& vset;
  std::vector<int64_t> vsteps;                  // [valid sets]
  std::vector<gcre_prefix::PrefixSlab> slabs;
  int64_t max_nv = 0, max_rows = 0;             // over the slabs
  PrefixArgs a{};                               // the slab on the device; the stage adds what its own kernel reads
  int64_t *d_which = nullptr, *d_row0 = nullptr;
  double* d_obs = nullptr;
  // one slab on the host, reused by the next
  std::vector<int64_t> which, row0;             // [nv] the set of every slot, [nv + 1] its first step row
  std::vector<PrefixPick> pick;                 // [nv]
  std::vector<double> obs;                      // [rows], where the variant's scores are asked for
  std::vector<uint8_t> score_nan;               // [nv] the slot's best observed score is NaN (first_active of gcre_seq_prefix.h)

  StepRows(const Variant& v_, const SetScoreRun& r) : v(v_), c(r.c), d(r.d), vset(r.vset) {}

  // the slabs: with `want_null` a set's null_max row of Kpad floats counts beside its step rows
  void plan(bool want_null, int32_t Kpad) {
    v.vsteps(vset, vsteps);
    gcre_prefix::prefix_slabs(vsteps, c->g.method, 2 * c->g.Wp, Kpad, want_null, gcre_prefix::prefix_max_mb(),
                              gcre_prefix::prefix_slab_sets(), slabs);
    for (const auto& sl : slabs) {
      max_nv = std::max(max_nv, sl.nv);
      max_rows = std::max(max_rows, sl.steps);
    }
  }

  // the caller's gene rows, set list and cut flags go up once; the buffers of the largest slab
  void upload(const gcre_set_input* in) {
    const Geometry& g = c->g;
    const int M = g.method;
    const int64_t S = in->n_sets, TM = in->set_off[S];
    a.gene_rows = (const uint32_t*)d.put(in->rows, std::max<size_t>((size_t)in->n_rows * (size_t)g.W, 1));
    a.set_off = d.put(in->set_off, (size_t)S + 1);
    a.members = d.put(in->members, (size_t)TM);
    a.signs = M == 2 && in->signs ? d.put(in->signs, (size_t)TM) : nullptr;
    a.cut = v.cut ? d.put(v.cut, (size_t)TM) : nullptr;
    a.which = d_which = d.take<int64_t>((size_t)max_nv);
    a.row0 = d_row0 = d.take<int64_t>((size_t)max_nv + 1);
    a.rows = d.take<uint32_t>((size_t)max_rows * (size_t)M * 2 * g.Wp);
    a.cnt = d.take<int32_t>((size_t)max_rows * 4);
    a.obs = d_obs = d.take<double>((size_t)max_rows);
    a.tot = d.take<uint32_t>((size_t)max_rows * M);
    a.thr = d.take<uint32_t>((size_t)max_nv);
    a.pick = d.take<PrefixPick>((size_t)max_nv);
    a.W2 = 2 * g.W;
    a.W32p = 2 * g.Wp;
    a.n_patients = g.n;
    a.n_cases = g.n_cases;
    pick.resize((size_t)max_nv);
    obs.resize(v.scores ? (size_t)max_rows : 0);
  }

  // one kernel of the call: nothing is launched behind an error, and `counter` counts what was
  template <typename Launch>
  void launch(int64_t& counter, Launch f) {
    if (!d.ok()) return;
    d.e = f();
    if (d.ok()) counter++;
  }

  // the slab's rows and their counts, their observed scores, every slot's best step and threshold: three kernels
  void build(const gcre_prefix::PrefixSlab& sl, int64_t& counter) {
    const int M = c->g.method;
    which.assign(vset.begin() + sl.v0, vset.begin() + sl.v0 + sl.nv);
    gcre_steps::slab_row0(vsteps, sl.v0, sl.nv, row0);
    a.nslots = sl.nv;
    a.nrows = sl.steps;
    d.upload(d_which, which.data(), (size_t)sl.nv);
    d.upload(d_row0, row0.data(), (size_t)sl.nv + 1);
    d.zero(a.cnt, (size_t)sl.steps * 4);
    launch(counter, [&] { return launch_rows(v, a, M, c->stream); });
    launch(counter, [&] { return launch_set_observed(a.cnt, sl.steps, M, c->d_dvt, d_obs, c->stream); });
    launch(counter, [&] { return launch_prefix_pick(a, M, c->stream); });
  }

  // queues the read-back of the picks (and the observed scores); the caller synchronises
  void fetch(const gcre_prefix::PrefixSlab& sl) {
    d.download(pick.data(), a.pick, (size_t)sl.nv);
    if (!obs.empty()) d.download(obs.data(), d_obs, (size_t)sl.steps);
  }

  // behind the synchronisation: the records of the slab's sets
  void collect(const gcre_prefix::PrefixSlab& sl) {
    score_nan.assign((size_t)sl.nv, 0);
    for (int64_t e = 0; e < sl.nv; e++) {
      const PrefixPick& p = pick[(size_t)e];
      score_nan[(size_t)e] = p.score != p.score;
      v.write(which[(size_t)e], p, obs.empty() ? nullptr : obs.data() + row0[(size_t)e]);
    }
  }
};

}  // namespace gcre_host

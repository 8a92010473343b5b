// gcre_host_pipeline.hip -- the one-call pipeline of libgcre_hip.so: gcre_process_paths (the ProcessPaths sequence,
// reference src/wrapper.cpp:216-276, over permutation windows) and gcre_process_paths_devices (the same call on several
// GPUs from one process, what the .Call shim resolves), with everything of RCCL.  Host code around the join driver of
// gcre_host.hip (join_once and the few helpers gcre_host.h declares); what needs only numbers and host arrays is in
// gcre_pipeline.h.
#include "gcre_host.h"

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is dlopen'ed where several devices are used (RcclApi)

#include <utility>

static_assert(kWindowTile == kSparseTile, "gcre_pipeline.h rounds windows to the tiles of the count planes");

namespace {

std::atomic<int64_t> g_rccl_collectives{0};   // RCCL collectives issued by this process (gcre_rccl_collectives)

// RCCL, loaded on first use (gcre_process_paths_devices with several distinct devices, gcre_rccl_selftest): the library
// does not link librccl, so a one-GPU user -- the R drop-in's default -- never needs it.  north_star: "RCCL all-reduce over
// xGMI of the per-permutation null maxima": ncclAllReduce(ncclMax) on each device's stream, in place on the device, for
// the thresholds shared inside a join and for the per-level merge; the host hub (ExchangeHub) stays the fallback (RCCL
// missing, a device listed twice) and the place where the device threads meet under a deadline before every collective.
struct RcclApi {
  void* so = nullptr;
  decltype(&ncclCommInitAll) comm_init_all = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclAllReduce) all_reduce = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
  bool ok = false;
  static RcclApi& get() {
    static RcclApi api = [] {
      RcclApi a;
      const char* off = std::getenv("GCRE_RCCL");
      if (off && std::strcmp(off, "0") == 0) return a;   // GCRE_RCCL=0: host hub only
      for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
        a.so = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (a.so) break;
      }
      if (!a.so) return a;
      a.comm_init_all = (decltype(a.comm_init_all))dlsym(a.so, "ncclCommInitAll");
      a.comm_destroy = (decltype(a.comm_destroy))dlsym(a.so, "ncclCommDestroy");
      a.all_reduce = (decltype(a.all_reduce))dlsym(a.so, "ncclAllReduce");
      a.error_string = (decltype(a.error_string))dlsym(a.so, "ncclGetErrorString");
      a.ok = a.comm_init_all && a.comm_destroy && a.all_reduce && a.error_string;
      return a;
    }();
    return api;
  }
};

void add_profile(gcre_profile& total, const gcre_profile& p) {
  total.null_kernel_ms += p.null_kernel_ms;
  total.null_kernel_launches += p.null_kernel_launches;
  total.stats_kernel_ms += p.stats_kernel_ms;
  total.select_ms += p.select_ms;
  total.total_ms += p.total_ms;
  total.paths += p.paths;
  total.scores += p.scores;
  total.null_alg_bytes += p.null_alg_bytes;
  total.null_row_loads += p.null_row_loads;
  total.ie_launches += p.ie_launches;
  total.ie_overlap_lists += p.ie_overlap_lists;
  total.ie_hinted_joins += p.ie_hinted_joins;
  total.ie_plane_joins += p.ie_plane_joins;
  total.ie_lookup_tiles += p.ie_lookup_tiles;
  total.prepare_ms += p.prepare_ms;
  total.inspect_ms += p.inspect_ms;
}

void clear_result(gcre_result* r) {
  std::memset(r, 0, sizeof *r);
  r->n = -1;   // NULL list entry, wrapper.cpp:223
}

// One gcre_process_paths call: what it was handed, what it has made so far, and what it changed on the context.  The
// destructor releases everything the call owns and, unless the call got to its end, frees the results it had filled and puts
// the context's permutation window and inspection-cache flag back.
struct PipelineRun {
  gcre_ctx* const c;
  const gcre_pp_input* const in;
  gcre_result* const out;
  const int L, Kall, ncol;
  // the tallies, exceedance counts and hit lists armed for this call (gcre_process_paths_set_tally, ...): taken at once,
  // so that every road out leaves none armed
  gcre_gene_tally* tallies[6];
  gcre_exceed* exceeds[6];
  gcre_hits* hit_lists[6];
  bool any_armed[3] = {false, false, false};
  gcre_profile total{};
  int window = 0;              // permutations per window (choose_window)
  bool first_window = true;
  std::vector<float> null_all[5];   // the null maxima of the windows walked so far, per result
  bool finished = false;
  // -- owned --
  // the operands: made in the first window, the same rows serve every window
  gcre_pathset *parsed1 = nullptr, *parsed2 = nullptr, *paths1 = nullptr, *paths2 = nullptr, *paths3 = nullptr;
  gcre_pathset *zero1 = nullptr, *input1 = nullptr, *zero2 = nullptr, *input2 = nullptr, *input_l2 = nullptr, *input_l3 = nullptr;
  // The join index of a level is uploaded once and serves every permutation window (the last level's may come from
  // prefetch_last_level, with its helper thread)
  gcre_uids* level_uids[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  gcre_result wout[5];         // the results of the window being walked, from the second window on
  bool cache_saved = false, cache_before = false;   // insp_cache was switched for several windows
  bool window_narrowed = false;                     // gcre_set_perm_window was called

  PipelineRun(gcre_ctx* c_, const gcre_pp_input* in_, gcre_result* out_)
      : c(c_), in(in_), out(out_), L(in_->path_length), Kall(c_->g.K), ncol(c_->g.n) {
    for (int i = 0; i < 5; i++) {
      clear_result(&out[i]);
      clear_result(&wout[i]);
    }
    for (int i = 0; i < 6; i++) {
      any_armed[0] |= (tallies[i] = std::exchange(c->pp_tally[i], nullptr)) != nullptr;
      any_armed[1] |= (exceeds[i] = std::exchange(c->pp_exceed[i], nullptr)) != nullptr;
      any_armed[2] |= (hit_lists[i] = std::exchange(c->pp_hits[i], nullptr)) != nullptr;
    }
  }
  ~PipelineRun() {
    if (cache_saved) c->insp_cache = cache_before;
    for (gcre_uids* u : level_uids) free_uids(u);
    free_sets({&zero1, &input1, &zero2, &input2, &input_l2, &input_l3, &parsed1, &parsed2, &paths1, &paths2, &paths3});
    if (finished) return;
    for (int i = 0; i < 5; i++) {
      gcre_result_free(&wout[i]);
      gcre_result_free(&out[i]);
      clear_result(&out[i]);
    }
    if (window_narrowed) (void)gcre_set_perm_window(c, 0, Kall);
  }
  gcre_result* out_w() { return first_window ? out : wout; }
  void announce(int level) const {
    if (!c->quiet && first_window) std::printf("Processing Path Length: %d\n", level);
  }
  static void free_sets(std::initializer_list<gcre_pathset**> sets) {
    for (gcre_pathset** p : sets) {
      gcre_pathset_free(*p);
      *p = nullptr;
    }
  }
};

// GCRE_OK when `made` is there, else the code of the call that should have made it
int made(const gcre_ctx* c, const void* p) {
  if (p) return GCRE_OK;
  return c->last_code != GCRE_OK ? c->last_code : GCRE_ERR_DEVICE;
}

// an operand that is made in the first window and serves every one after it
template <typename Make>
int once(gcre_ctx* c, gcre_pathset*& slot, Make make) {
  if (!slot) slot = make();
  return made(c, slot);
}

// Large permutation counts run in windows of whole 2048-permutation tiles: the count planes of the kept sets are per
// tile, and a window is as many tiles as fit next to the rows.  Scores and top-k lists do not depend on the window (the
// first window's are returned); the null maxima of the windows are concatenated.
int choose_window(gcre_ctx* c, const gcre_pp_input* in, const std::vector<int64_t>& rows) {
  const int Kall = c->g.K;
  int win = std::max(1, gcre_plan_perm_window(c, rows.data(), (int)rows.size()));
  if (in->window_perms > 0) {
    win = round_window_perms(in->window_perms, Kall);
  } else if (Kall > kSparseTile && sparse_enabled(c)) {
    // A context without a pooled plane buffer of the full size (the R shim makes a fresh context per call, as the
    // reference does) has to hipMalloc the planes: ~40 ms per GB here, 3 KB per kept row and tile.  Against ~25 ms of
    // repeated inspector work per extra window, few tiles per window win: w* = sqrt(25 ms * tiles / (ms per tile)).
    // (A set above the recipe limit stores no planes.)
    const int nkt_all = (Kall + kSparseTile - 1) / kSparseTile;
    int64_t biggest = 0;
    for (size_t i = 2; i < rows.size(); i++) {
      const double full = (double)rows[i] * c->g.method * 3072.0 * nkt_all;
      if (full <= (double)c->planes_out_max) biggest = std::max(biggest, rows[i]);
    }
    const double ms_per_tile = (double)biggest * c->g.method * 3072.0 / 1e9 * 40.0;
    const size_t full_bytes = (size_t)biggest * c->g.method * 3072 * (size_t)((win + kSparseTile - 1) / kSparseTile);
    bool pooled = false;
    for (const auto& pb : c->plane_pool) pooled = pooled || pb.bytes >= full_bytes;
    if (ms_per_tile > 1.0 && !pooled) {
      const int w = std::max(1, (int)std::sqrt(25.0 * nkt_all / ms_per_tile));
      win = std::min(win, w * kSparseTile);
    }
  }
  return std::max(1, std::min(win, std::max(Kall, 1)));
}

// The last level's segment table and quads (tens of milliseconds of host work at 2.5 M uids) depend on its join index
// only: a helper thread builds them while the first levels run (GCRE_PREFETCH_TABLES=0: built when the join asks)
int prefetch_last_level(PipelineRun& R) {
  gcre_ctx* c = R.c;
  const int L = R.L;
  if (!(L >= 3 && R.Kall > 0 && R.in->shard_world <= 1 && sparse_enabled(c) && (c->null_kernel == 0 || c->null_kernel == 3)) ||
      (std::getenv("GCRE_PREFETCH_TABLES") && std::atoi(std::getenv("GCRE_PREFETCH_TABLES")) == 0))
    return GCRE_OK;
  const gcre_level& lv = R.in->level[L];
  const int64_t P = total_paths(lv);
  if (!(lv.n_uids > 100000 && P > 0 && P <= c->chunk_paths)) return GCRE_OK;
  R.level_uids[L] = make_uids(c, L, lv.uid_count, lv.uid_location, lv.n_uids, lv.signs, lv.n_signs);
  if (!R.level_uids[L]) return c->last_code;
  start_table_prefetch(c, R.level_uids[L], P, R.window);
  return GCRE_OK;
}

// The exchange of a sharded join as the join driver calls it (JoinPlan::exchange): MAX over the devices of the running
// maxima [k0, k1) in d_null.  With RCCL the maxima never leave the devices: the threads meet first (same level, window and
// exchange on every device, under the hub's deadline), then each issues the in-place MAX all-reduce on its stream.
int exchange_maxima(void* user, void* d_null, int32_t k0, int32_t k1) {
  gcre_ctx* cc = (gcre_ctx*)user;
  std::vector<float> v((size_t)std::max(k1 - k0, 0));
  if (v.empty()) return 0;
  const uint64_t tag = hub_tag(cc->hub_level, k0, cc->hub_round++);
  if (cc->comm) {
    if (cc->hub->meet(tag) != 0) return 1;
    const ncclResult_t nr = RcclApi::get().all_reduce(d_null, d_null, v.size(), ncclFloat32, ncclMax, cc->comm, cc->stream);
    cc->rccl_calls++;
    g_rccl_collectives++;
    if (nr != ncclSuccess || hipStreamSynchronize(cc->stream) != hipSuccess) { cc->hub->fail(); return 1; }
    return 0;
  }
  if (hipMemcpy(v.data(), d_null, v.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { cc->hub->fail(); return 1; }
  if (cc->hub->reduce(v, tag) != 0) return 1;
  return hipMemcpy(d_null, v.data(), v.size() * 4, hipMemcpyHostToDevice) == hipSuccess ? 0 : 1;
}

// The devices of this call share their running maxima during the join of level `lvi` (0..5 = levels 1a, 1b, 2, 3, 4, 5)
// when it is large enough (exchange_count): unit, count, buffer, level and round
int arm_exchange(PipelineRun& R, const gcre_uids* u, int lvi, JoinPlan& jp) {
  gcre_ctx* c = R.c;
  double unit = 2e6, most = 8.0;
  if (const char* e = std::getenv("GCRE_EXCHANGE_UNIT")) unit = std::atof(e);
  if (const char* e = std::getenv("GCRE_EXCHANGE_MAX")) most = std::min(std::max(std::atof(e), 1.0), 32.0);
  const int exchanges = exchange_count(u->total, R.in->shard_world, R.window, unit, most);
  if (exchanges == 0) return GCRE_OK;
  // the number of exchanges must be the same on every device BY CONSTRUCTION: a device that cannot get its buffer
  // fails the call (its thread then fails the hub) instead of silently joining with none -- the others would wait
  // for it for ever, or pair their round with its next join
  if (c->d_hub_null.reserve((size_t)c->g.Kpad + 64) != hipSuccess) return fail(c, GCRE_ERR_DEVICE, "no memory for the exchange buffer");
  jp.exchanges = exchanges;
  jp.d_null_out = c->d_hub_null.p;
  jp.exchange_user = c;
  jp.exchange = exchange_maxima;
  c->hub_level = lvi;
  c->hub_round = 0;
  return GCRE_OK;
}

// merge_scores across devices (src/methods.h:34-37) over RCCL: element-wise MAX all-reduce of this window's f32 null
// maxima, in place on the device -- exact for any sharding (f32 max is associative, the values are f32-rounded).
// Every device then returns the merged maxima; the caller's host-side MAX over devices changes nothing any more.
int merge_level_maxima(gcre_ctx* c, int lvi, gcre_result* res) {
  if (c->hub->meet(hub_tag(lvi, c->win_k0, 0xffff)) != 0) return fail(c, GCRE_ERR_DEVICE, "the devices did not meet for the level's RCCL merge");
  float* d = (float*)(c->d_null + c->win_k0);
  const ncclResult_t nr = RcclApi::get().all_reduce(d, d, (size_t)c->win_K, ncclFloat32, ncclMax, c->comm, c->stream);
  c->rccl_calls++;
  g_rccl_collectives++;
  hipError_t he = nr == ncclSuccess ? hipMemcpyAsync(res->null_max, d, (size_t)c->win_K * 4, hipMemcpyDeviceToHost, c->stream) : hipErrorUnknown;
  if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
  if (he == hipSuccess) return GCRE_OK;
  c->hub->fail();
  return fail(c, GCRE_ERR_DEVICE, std::string("RCCL all-reduce of the null maxima failed: ") + (nr != ncclSuccess ? RcclApi::get().error_string(nr) : hipGetErrorString(he)));
}

// One join of the sequence: level `lvi` of the input joins p0 with p1 into res (or keeps no rows), the result goes to `o` (or
// is discarded).  red/red_index: what the join really adds to paths0 (gcre_uids_set_reduced) -- checked per join, never trusted.
int level_join(PipelineRun& R, int plen, int lvi, const gcre_pathset* p0, const gcre_pathset* p1, gcre_pathset* res,
               gcre_result* o, const gcre_pathset* red, const int32_t* red_index, int64_t n_red) {
  gcre_ctx* c = R.c;
  const gcre_pp_input* in = R.in;
  const gcre_level& lv = in->level[lvi];
  gcre_uids*& u = R.level_uids[lvi];
  if (!u) {
    u = make_uids(c, plen, lv.uid_count, lv.uid_location, lv.n_uids, lv.signs, lv.n_signs);
    if (!u) return c->last_code;
  }
  if (!u->red && red && red_index && n_red >= p1->nrows) {   // once: the operand outlives the windows
    bool in_range = true;
    for (int64_t i = 0; i < n_red && in_range; i++) in_range = (int64_t)((uint32_t)red_index[i] & 0x7fffffffu) < red->nrows;
    if (in_range && gcre_uids_set_reduced(u, red, red_index, n_red) != GCRE_OK) return c->last_code;
  }
  JoinPlan jp{u, p0, p1, res, false, 0, 0, nullptr};
  jp.tally = R.tallies[lvi];   // (every permutation window folds the same observed scores: harmless)
  jp.exceed = R.exceeds[lvi];
  jp.exceed_observed = c->win_k0 == 0;   // the observed scores once per call, the null values of every window
  jp.hits = c->win_k0 == 0 ? R.hit_lists[lvi] : nullptr;   // (the same rule: a list appends)
  if (in->shard_world > 1) {   // one device of several: its slice of the joined paths, every kept row
    jp.sharded = true;
    shard_bounds(u->total, in->shard_rank, in->shard_world, &jp.shard_begin, &jp.shard_end);
    if (c->hub && c->win_K > 0)
      if (int rc = arm_exchange(R, u, lvi, jp)) return rc;
  }
  gcre_result tmp;
  int rc = join_once(c, jp, &tmp);
  // (the 1a join's result is discarded: nothing to merge)
  if (rc == GCRE_OK && o && c->comm && c->hub && c->win_K > 0 && tmp.null_max) rc = merge_level_maxima(c, lvi, &tmp);
  if (rc != GCRE_OK) {
    gcre_result_free(&tmp);
    return rc;
  }
  add_profile(R.total, c->prof);
  if (o) *o = tmp; else gcre_result_free(&tmp);
  return GCRE_OK;
}

// ---- the five levels: which operand is made, what the hint is, whether a result is kept ----

int level_1(PipelineRun& R) {   // wrapper.cpp:225-244
  gcre_ctx* c = R.c;
  const gcre_pp_input* in = R.in;
  R.announce(1);
  if (int rc = once(c, R.paths1, [&] { return new_pathset(c, total_paths(in->level[0]), true); })) return rc;
  if (int rc = once(c, R.zero1, [&] { return gcre_pathset_zeros(c, in->n_data_inds[0]); })) return rc;
  if (int rc = once(c, R.input1, [&] { return gcre_pathset_select(c, R.parsed1, in->data_inds[0], in->n_data_inds[0]); })) return rc;
  // result discarded, wrapper.cpp:233
  if (int rc = level_join(R, 1, 0, R.zero1, R.input1, R.paths1, nullptr, R.parsed1, in->data_inds[0], in->n_data_inds[0])) return rc;

  R.announce(1);
  if (int rc = once(c, R.zero2, [&] { return gcre_pathset_zeros(c, in->n_data_inds[1]); })) return rc;
  if (int rc = once(c, R.parsed2, [&] { return gcre_pathset_from_dense(c, in->data2, in->data2_rows, R.ncol, in->data_col_major); })) return rc;
  if (int rc = once(c, R.input2, [&] { return gcre_pathset_select(c, R.parsed2, in->data_inds[1], in->n_data_inds[1]); })) return rc;
  return level_join(R, 1, 1, R.zero2, R.input2, nullptr, &R.out_w()[0], R.parsed2, in->data_inds[1], in->n_data_inds[1]);
}

int level_2(PipelineRun& R) {   // wrapper.cpp:246-253
  gcre_ctx* c = R.c;
  const gcre_pp_input* in = R.in;
  R.announce(2);
  if (int rc = once(c, R.paths2, [&] { return new_pathset(c, total_paths(in->level[2]), true); })) return rc;
  // the sequence is known here: when level 3's rows are too many to leave with count planes they leave with a recipe
  // whose operand is this set -- which then must not be recipe-only itself (it would be rebuilt from bit lists)
  if (R.L >= 4 && plane_bytes(c, total_paths(in->level[3]), 2) > c->planes_out_max) R.paths2->planes_wanted = true;
  if (R.L >= 5) R.paths2->planes_wanted = true;   // level 5 adds rows of this set: their planes are read per joined path
  // the reference reads data_idx2 from r_data_inds3 (wrapper.cpp:207); R passes identical vectors
  if (int rc = once(c, R.input_l2, [&] { return gcre_pathset_select(c, R.parsed1, in->data_inds[3], in->n_data_inds[3]); })) return rc;
  return level_join(R, 2, 2, R.paths1, R.input_l2, R.paths2, &R.out_w()[1], R.parsed1, in->data_inds[3], in->n_data_inds[3]);
}

int level_3(PipelineRun& R) {   // wrapper.cpp:255-262
  gcre_ctx* c = R.c;
  const gcre_pp_input* in = R.in;
  R.announce(3);
  if (int rc = once(c, R.paths3, [&] { return new_pathset(c, total_paths(in->level[3]), true); })) return rc;
  if (int rc = once(c, R.input_l3, [&] { return gcre_pathset_select(c, R.parsed1, in->data_inds[3], in->n_data_inds[3]); })) return rc;
  return level_join(R, 3, 3, R.paths2, R.input_l3, R.paths3, &R.out_w()[2], R.parsed1, in->data_inds[3], in->n_data_inds[3]);
}

int level_4(PipelineRun& R) {   // wrapper.cpp:264-269
  const gcre_pp_input* in = R.in;
  R.announce(4);
  const std::vector<int32_t> added = added_rows_hint(R.c->g.method, in->data_inds[3], in->n_data_inds[3], in->level[2]);
  return level_join(R, 4, 4, R.paths3, R.paths2, nullptr, &R.out_w()[3], R.parsed1, added.data(), (int64_t)added.size());
}

int level_5(PipelineRun& R) {   // wrapper.cpp:271-276
  R.announce(5);
  const std::vector<int32_t> second = second_relation_hint(R.c->g.method, R.in->level[3]);
  return level_join(R, 5, 5, R.paths3, R.paths3, nullptr, &R.out_w()[4], R.paths2, second.data(), (int64_t)second.size());
}

// permutations [k0, k0 + window) of every level; this window's maxima go behind the ones we have (later windows only
// contribute maxima)
int run_window(PipelineRun& R, int k0) {
  gcre_ctx* c = R.c;
  const gcre_pp_input* in = R.in;
  R.first_window = k0 == 0;
  if (R.Kall > 0) {
    R.window_narrowed = true;
    if (int rc = gcre_set_perm_window(c, k0, std::min(R.Kall, k0 + R.window))) return rc;
  }
  // wrapper.cpp:216-217
  if (int rc = once(c, R.parsed1, [&] { return gcre_pathset_from_dense(c, in->data1, in->data1_rows, R.ncol, in->data_col_major); })) return rc;
  int rc = R.L >= 1 ? level_1(R) : GCRE_OK;
  if (rc == GCRE_OK && R.L >= 2) rc = level_2(R);
  if (rc == GCRE_OK && R.L >= 3) rc = level_3(R);
  if (rc == GCRE_OK && R.L >= 4) rc = level_4(R);
  if (rc == GCRE_OK && R.L >= 5) rc = level_5(R);
  if (rc != GCRE_OK) return rc;
  gcre_result* const out_w = R.out_w();
  for (int i = 0; i < 5; i++) {
    if (out_w[i].n < 0) continue;
    R.null_all[i].insert(R.null_all[i].end(), out_w[i].null_max, out_w[i].null_max + out_w[i].n_perm);
    if (!R.first_window) {
      gcre_result_free(&out_w[i]);
      clear_result(&out_w[i]);
    }
  }
  return GCRE_OK;
}

// every window is walked: the context gets its settings back, the results the maxima of all windows
int finish_pipeline(PipelineRun& R) {
  gcre_ctx* c = R.c;
  R.free_sets({&R.zero1, &R.input1, &R.zero2, &R.input2, &R.input_l2, &R.input_l3});   // the operand copies (the same rows served every window)
  if (R.cache_saved) {
    c->insp_cache = R.cache_before;
    R.cache_saved = false;
    if (!R.cache_before) (void)gcre_drop_inspections(c, 1);
  }
  if (R.Kall > 0)
    if (int rc = gcre_set_perm_window(c, 0, R.Kall)) return rc;
  for (int i = 0; i < 5; i++) {
    if (R.out[i].n < 0 || R.Kall == 0) continue;
    std::free(R.out[i].null_max);
    R.out[i].n_perm = R.Kall;
    R.out[i].null_max = (float*)std::calloc((size_t)R.Kall, sizeof(float));
    std::memcpy(R.out[i].null_max, R.null_all[i].data(), (size_t)R.Kall * sizeof(float));
  }
  if (!c->quiet) std::printf("[success]\n");   // wrapper.cpp:278
  R.finished = true;
  c->prof = R.total;
  return GCRE_OK;
}

// ---- several devices, one process ----

void say(char* err, size_t errlen, const std::string& m) {
  if (err && errlen) std::snprintf(err, errlen, "%s", m.c_str());
}

// One gcre_process_paths_devices call: a context, a communicator (or none) and a table of results per device, and the hub
// where the device threads MAX-merge their running maxima during the large joins
struct DevicesRun {
  std::vector<int> dev;
  std::vector<gcre_ctx*> ctx;
  std::vector<ncclComm_t> comms;
  std::vector<std::array<gcre_result, 5>> part;
  std::vector<int> rcs;
  ExchangeHub hub;
  int N() const { return (int)dev.size(); }
  ~DevicesRun() {
    for (ncclComm_t cm : comms)
      if (cm) (void)RcclApi::get().comm_destroy(cm);
    for (int r = 0; r < N(); r++) {
      for (gcre_result& p : part[(size_t)r])   // (a device that failed left none)
        if (p.n >= 0 || p.null_max) gcre_result_free(&p);
      if (ctx[(size_t)r]) {
        (void)hipSetDevice(dev[(size_t)r]);
        gcre_destroy(ctx[(size_t)r]);
      }
    }
  }
};

// contexts first (one per device), so that every device can be asked for its window before anybody starts
int make_contexts(DevicesRun& D, int method, int n_cases, int n_ctrls, int iterations, int top_k, char* err, size_t errlen) {
  for (int r = 0; r < D.N(); r++) {
    gcre_ctx*& c = D.ctx[(size_t)r];
    c = gcre_create(method, n_cases, n_ctrls, iterations, D.dev[(size_t)r]);
    if (!c) { say(err, errlen, gcre_last_error(nullptr)); return GCRE_ERR_DEVICE; }
    c->quiet = c->quiet || r > 0;   // the reference's progress lines once
    if (int rc = gcre_set_top_k(c, top_k)) { say(err, errlen, gcre_last_error(c)); return rc; }
  }
  return GCRE_OK;
}

// the smallest window any device plans: all of them walk the same windows (their maxima are merged per window)
int agreed_window(DevicesRun& D, const gcre_pp_input* in, int iterations) {
  const std::vector<int64_t> rows = set_rows(in);
  int window = iterations;
  for (int r = 0; r < D.N(); r++) {
    (void)hipSetDevice(D.dev[(size_t)r]);
    window = std::min(window, std::max(1, gcre_plan_perm_window(D.ctx[(size_t)r], rows.data(), (int)rows.size())));
  }
  return window;
}

// RCCL communicators, one per device, when every device is listed once (RCCL refuses a device twice: the one-GPU
// rehearsal stays on the host hub) and the library loads.  GCRE_RCCL=0: never; GCRE_RCCL=force: also for one device
// (one-rank collectives: what a one-GPU box can exercise of this path).
void make_communicators(DevicesRun& D, int iterations) {
  const int N = D.N();
  const char* mode = std::getenv("GCRE_RCCL");
  const bool force = mode && std::strcmp(mode, "force") == 0;
  bool distinct = true;
  for (int a = 0; a < N; a++)
    for (int b = a + 1; b < N; b++) distinct = distinct && D.dev[(size_t)a] != D.dev[(size_t)b];
  if (!(distinct && (N > 1 || force) && iterations > 0 && RcclApi::get().ok)) return;
  D.comms.assign((size_t)N, nullptr);
  if (RcclApi::get().comm_init_all(D.comms.data(), N, D.dev.data()) != ncclSuccess) {
    D.comms.clear();   // (no communicator: the host hub serves the call)
    (void)hipGetLastError();
  }
}

// one host thread per device, each with its shard of every level; the first failure is the call's
int run_devices(DevicesRun& D, const gcre_pp_input* in, int window, char* err, size_t errlen) {
  const int N = D.N();
  auto work = [&](int r) {
    gcre_ctx* c = D.ctx[(size_t)r];
    gcre_pp_input mine = *in;
    mine.shard_rank = N > 1 ? r : 0;
    mine.shard_world = N > 1 ? N : 0;
    mine.window_perms = N > 1 ? window : in->window_perms;
    c->hub = (N > 1 || !D.comms.empty()) ? &D.hub : nullptr;
    c->comm = D.comms.empty() ? nullptr : D.comms[(size_t)r];
    D.rcs[(size_t)r] = gcre_process_paths(c, &mine, D.part[(size_t)r].data());
    c->hub = nullptr;
    c->comm = nullptr;
    if (D.rcs[(size_t)r] != GCRE_OK) D.hub.fail();   // nobody waits for a device that has given up
  };
  std::vector<std::thread> th;
  for (int r = 1; r < N; r++) th.emplace_back(work, r);
  work(0);
  for (auto& t : th) t.join();
  for (int r = 0; r < N; r++)
    if (D.rcs[(size_t)r] != GCRE_OK) {
      say(err, errlen, "device " + std::to_string(D.dev[(size_t)r]) + ": " + gcre_last_error(D.ctx[(size_t)r]) +
                           (D.hub.timed_out ? " (a device waited longer than GCRE_HUB_TIMEOUT_S for the others at a threshold exchange)" : ""));
      return D.rcs[(size_t)r];
    }
  return GCRE_OK;
}

// merge_scores / format_result (methods.h:25-39, join_base.cpp:138-154) across devices: f32 MAX of the maxima (exact
// for any sharding: f32 max is associative, every device holds f32-rounded values), best top_k of all tables with the
// canonical tie rule (smaller joined-path ordinal = smaller (idx, loc)), the sentinel when fewer than top_k exist
void merge_devices(const DevicesRun& D, int top_k, gcre_result out[5]) {
  for (int lv = 0; lv < 5; lv++) {
    if (D.part[0][(size_t)lv].n < 0) continue;
    gcre_result& o = out[lv];
    const int K = D.part[0][(size_t)lv].n_perm;
    o.n_perm = K;
    o.null_max = (float*)std::calloc((size_t)std::max(K, 1), sizeof(float));
    std::vector<Candidate> cands;
    for (int r = 0; r < D.N(); r++) {
      const gcre_result& p = D.part[(size_t)r][(size_t)lv];
      for (int k = 0; k < K; k++) o.null_max[k] = std::max(o.null_max[k], p.null_max[k]);
      for (int i = 0; i < p.n; i++)
        if (p.src[i] >= 0) cands.push_back(Candidate{p.scores[i], ((int64_t)p.src[i] << 32) | (uint32_t)p.trg[i], p.src[i], p.trg[i], p.cases[i], p.ctrls[i]});
    }
    merge_candidates(cands, top_k, &o);
  }
}

}  // namespace

extern "C" {

int gcre_process_paths(gcre_ctx* c, const gcre_pp_input* in, gcre_result out[5]) {
  if (!c || !in || !out) return fail(c, GCRE_ERR_ARG, "bad process_paths arguments");
  (void)hipSetDevice(c->device);
  PipelineRun R(c, in, out);
  static const char* const refusal[3] = {
      "a gene tally cannot be armed for one device of several: merging tallies across devices is not supported",
      "exceedance counts cannot be armed for one device of several: add the counts of whole runs on the host",
      "a hit list cannot be armed for one device of several: merging lists across devices is not supported"};
  for (int k = 0; k < 3; k++)
    if (R.any_armed[k] && in->shard_world > 1) return fail(c, GCRE_ERR_ARG, refusal[k]);
  if (int rc = gcre_set_value_table(c, in->value_table, in->vt_rows, in->vt_cols, in->vt_col_major)) return rc;   // wrapper.cpp:213
  // a context whose masks were generated on the device (gcre_generate_perm_masks) or uploaded packed keeps them
  // when the caller passes no matrix; otherwise wrapper.cpp:214
  if (!(in->perm_cases == nullptr && in->perm_rows == 0 && c->have_perms))
    if (int rc = gcre_set_perm_cases(c, in->perm_cases, in->perm_rows, c->g.n, in->perm_col_major)) return rc;
  R.window = choose_window(c, in, set_rows(in));
  if (int rc = prefetch_last_level(R)) return rc;
  // several windows: the joins of the 2nd..nth window start at their null kernels (inspection cache; the operands
  // are made once, so that every window joins the same sets)
  if (R.Kall > R.window) {
    R.cache_saved = true;
    R.cache_before = c->insp_cache;
    c->insp_cache = inspect_cache_allowed();
  }
  for (int k0 = 0; k0 < std::max(R.Kall, 1); k0 += R.window)
    if (int rc = run_window(R, k0)) return rc;
  return finish_pipeline(R);
}

int gcre_process_paths_devices(int method, int n_cases, int n_ctrls, int iterations, int top_k, const int* devices,
                               int n_devices, const gcre_pp_input* in, gcre_result out[5], char* err, size_t errlen) {
  if (!in || !out) { say(err, errlen, "bad arguments"); return GCRE_ERR_ARG; }
  for (int i = 0; i < 5; i++) clear_result(&out[i]);
  int visible = 0;
  if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0) { say(err, errlen, "no HIP device: libgcre_hip has no CPU fallback"); return GCRE_ERR_DEVICE; }
  DevicesRun D;
  if (n_devices <= 0) n_devices = visible;
  for (int i = 0; i < n_devices; i++) D.dev.push_back(devices ? devices[i] : i % visible);
  const int N = D.N();
  D.ctx.assign((size_t)N, nullptr);
  D.part.resize((size_t)N);
  D.rcs.assign((size_t)N, GCRE_OK);
  D.hub.n = N;
  if (const char* e = std::getenv("GCRE_HUB_TIMEOUT_S")) D.hub.timeout_s = std::max(0.01, std::atof(e));

  if (int rc = make_contexts(D, method, n_cases, n_ctrls, iterations, top_k, err, errlen)) return rc;
  const int window = (N > 1 && iterations > 0) ? agreed_window(D, in, iterations) : 0;
  make_communicators(D, iterations);
  if (int rc = run_devices(D, in, window, err, errlen)) return rc;
  merge_devices(D, top_k, out);
  return GCRE_OK;
}

int64_t gcre_rccl_collectives(void) { return g_rccl_collectives.load(); }

int gcre_rccl_selftest(int device, char* err, size_t errlen) {
  RcclApi& api = RcclApi::get();
  if (!api.ok) { say(err, errlen, "librccl.so not found (or GCRE_RCCL=0)"); return GCRE_ERR_DEVICE; }
  if (hipSetDevice(device) != hipSuccess) { say(err, errlen, "no such device"); return GCRE_ERR_DEVICE; }
  ncclComm_t comm = nullptr;
  ncclResult_t nr = api.comm_init_all(&comm, 1, &device);
  if (nr != ncclSuccess) { say(err, errlen, std::string("ncclCommInitAll: ") + api.error_string(nr)); return GCRE_ERR_DEVICE; }
  const size_t n = 4096;
  std::vector<float> h(n), back(n);
  for (size_t i = 0; i < n; i++) h[i] = (float)((i * 2654435761u) % 1000u) / 8.0f;
  float* d = nullptr;
  hipStream_t st = nullptr;
  int rc = GCRE_OK;
  if (hipMalloc((void**)&d, n * 4) != hipSuccess || hipStreamCreate(&st) != hipSuccess) rc = GCRE_ERR_DEVICE;
  if (rc == GCRE_OK && hipMemcpyAsync(d, h.data(), n * 4, hipMemcpyHostToDevice, st) != hipSuccess) rc = GCRE_ERR_DEVICE;
  if (rc == GCRE_OK) {
    nr = api.all_reduce(d, d, n, ncclFloat32, ncclMax, comm, st);   // one rank: MAX over {x} = x
    g_rccl_collectives++;
    if (nr != ncclSuccess) { say(err, errlen, std::string("ncclAllReduce: ") + api.error_string(nr)); rc = GCRE_ERR_DEVICE; }
  }
  if (rc == GCRE_OK && (hipMemcpyAsync(back.data(), d, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess))
    rc = GCRE_ERR_DEVICE;
  if (rc == GCRE_OK && std::memcmp(h.data(), back.data(), n * 4) != 0) { say(err, errlen, "one-rank MAX all-reduce changed the data"); rc = GCRE_ERR_DEVICE; }
  if (d) (void)hipFree(d);
  if (st) (void)hipStreamDestroy(st);
  (void)api.comm_destroy(comm);
  return rc;
}

}  // extern "C"

// gcre_host.h -- private to the host side of libgcre_hip.so: the state behind the handles of include/gcre_hip.h and the
// few helpers that its translation units share.  gcre_host.hip holds the join driver and everything that feeds it,
// gcre_host_sets.hip the set scores and their driver (gcre_set_stage.h), with one file per stage behind them
// (gcre_host_family.hip, _minp, _compete, _steps, _subsample, _sequential, _strata), gcre_host_stats.hip the other entry points that only use a
// context (decorated p-values, overlaps, clumps, tallies, burden tests, the gene tally, the exceedance counts and the hit lists
// as objects), gcre_host_pipeline.hip the one-call pipeline on one device and on several (and with it everything of RCCL).
// Nothing here is part of the ABI.
#pragma once
#include "../../include/gcre_hip.h"
#include "gcre_kernels.h"
#include "gcre_pipeline.h"   // Candidate and merge_candidates; ExchangeHub, which a context only points to

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <string>
#include <unordered_map>
#include <thread>
#include <functional>
#include <deque>
#include <vector>

using namespace gcre;

struct ncclComm;   // RCCL's communicator, opaque here (ncclComm_t is a pointer to it): only gcre_host_pipeline.hip includes rccl.h

// What the host files see of each other stays out of the dynamic symbol table
namespace gcre_host __attribute__((visibility("hidden"))) {

// The piece table of the range check (RangePiece): range r = rows loc[r] .. loc[r] + cnt[r] - 1 of paths1, whole when it has at
// most `piece_rows` rows, otherwise cut into pieces of that many and listed in `cut`.  Returns the rows in all.
inline int64_t build_range_pieces(const std::vector<int64_t>& loc, const std::vector<int32_t>& cnt, std::vector<RangePiece>& pieces,
                                  std::vector<int32_t>& cut, int32_t piece_rows = kRangePieceRows) {
  int64_t rows = 0;
  for (size_t r = 0; r < loc.size(); r++) {
    rows += cnt[r];
    if (cnt[r] <= piece_rows) {
      pieces.push_back(RangePiece{loc[r], (int32_t)r, cnt[r]});
      continue;
    }
    cut.push_back((int32_t)r);
    for (int32_t t = 0; t < cnt[r]; t += piece_rows)
      pieces.push_back(RangePiece{loc[r] + t, (int32_t)r, (int32_t)(std::min(piece_rows, cnt[r] - t) | 0x80000000)});
  }
  return rows;
}

template <typename T>
struct DevBuf {   // grow-only device scratch
  T* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
  // room for n elements (at least one), filled from the host
  hipError_t upload(const T* src, size_t n, hipStream_t stream) {
    hipError_t e = reserve(std::max<size_t>(n, 1));
    if (e == hipSuccess && n) e = hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, stream);
    return e;
  }
  // grow and keep the first `keep` elements
  hipError_t grow_keep(size_t n, size_t keep, hipStream_t stream) {
    if (n <= cap) return hipSuccess;
    T* q = nullptr;
    hipError_t e = hipMalloc((void**)&q, n * sizeof(T));
    if (e != hipSuccess) return e;
    if (p && keep) {
      e = hipMemcpyAsync(q, p, std::min(keep, cap) * sizeof(T), hipMemcpyDeviceToDevice, stream);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
    }
    if (p) (void)hipFree(p);
    p = q;
    cap = n;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// top-k of a chunk: indices chosen by the radix select, their keys / counts / rows gathered and copied out
struct Winners {
  std::vector<uint32_t> sel, cases, ctrls, r0, r1;
  std::vector<uint64_t> key;
  std::vector<uint64_t> pack;   // where the device's copy lands: n keys, then cases, ctrls, r0, r1 as 32-bit words (unpack_winners)
  uint32_t n = 0;
};

// The buffers a chunk's inspector writes and its permutation kernel and top-k selection read: the context's scratch, or
// (inspection cache on) a chunk entry's own
struct ChunkBufs {
  DevBuf<uint32_t> row0, row1, tot, cases, ctrls, dcnt, dlist, rowz, linfo, lover, dover;
  DevBuf<uint64_t> key;
  void release() {
    for (auto* b : {&row0, &row1, &tot, &cases, &ctrls, &dcnt, &dlist, &rowz, &linfo, &lover, &dover}) b->release();
    key.release();
  }
};

// What the inspector of one chunk of a join left behind -- expanded row numbers, statistics, score keys, lists, flags
// and the chunk's top-k winners.  None of it depends on the permutation masks: with the inspection cache on
// (gcre_set_inspect_cache) the buffers belong to the join index instead of the context's scratch, and the next
// permutation window of the same join starts at the null kernel.
struct ChunkInsp {
  int64_t cb = -1, n = 0, s0 = 0, s1 = 0;
  int64_t padded = 0;         // rows / totals are zero up to here (whole path tiles of the dense kernel)
  bool inspected = false;     // rows / statistics / keys (and kept rows) are those of this chunk
  bool with_lists = false;    // ... written by the inclusion-exclusion inspector: lists, rowz, linfo
  bool in_recipe = false;     // ... into the kept set's recipe (not into the buffers below)
  bool flags_valid = false;   // host copy of the inspector's flag block
  bool win_valid = false;     // top-k winners
  // An inspection that ran ahead leaves its selection OPEN (GCRE_SELECT_DEFER): the digit passes are queued on the selection
  // stream, their state lands in h_state, and whoever replays the chunk next -- the launch, behind its null kernels, or the
  // join's own call -- closes it.  A launch leaves the winners' copies PENDING in `win`: the join's own call unpacks them
  bool sel_open = false;
  bool win_pending = false;
  SelectState* h_state = nullptr;   // pinned: the state's copy must not hold the host, and must not move with the entry
  uint32_t flags[kFlagWords] = {};
  Winners win;
  ChunkBufs bufs;
  // the entry describes nothing any more (the buffers stay).  Not while win_pending: drop_launch waits for the copies first
  void forget() { inspected = with_lists = flags_valid = win_valid = sel_open = false; }
  void release() {
    bufs.release();
    if (h_state) (void)hipHostFree(h_state);
    h_state = nullptr;
    forget();
  }
};

struct InspKey {
  uint64_t p0_id = 0, p0_ver = 0, p1_id = 0, p1_ver = 0, red_id = 0, red_ver = 0, res_id = 0, obs_epoch = 0;
  int64_t sb = 0, se = 0, keep_begin = 0, keep_end = 0, chunk_paths = 0;
  int keep_mode = 0, top_k = 0, null_kernel = 0;
  bool operator==(const InspKey& o) const {
    return p0_id == o.p0_id && p0_ver == o.p0_ver && p1_id == o.p1_id && p1_ver == o.p1_ver && red_id == o.red_id &&
           red_ver == o.red_ver && res_id == o.res_id && obs_epoch == o.obs_epoch && sb == o.sb && se == o.se &&
           keep_begin == o.keep_begin && keep_end == o.keep_end && chunk_paths == o.chunk_paths && keep_mode == o.keep_mode &&
           top_k == o.top_k && null_kernel == o.null_kernel;
  }
};

inline double key_to_score(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double d;
  std::memcpy(&d, &b, sizeof d);
  return d;
}

// One join as the driver runs it: operands, the shard, what is kept, and the objects it feeds
struct JoinPlan {
  const gcre_uids* u;
  const gcre_pathset* p0;
  const gcre_pathset* p1;
  gcre_pathset* res;
  bool sharded;
  int64_t shard_begin, shard_end;
  void* d_null_out;
  bool keep_ranged = false;        // rows outside [keep_begin, keep_end) and the shard are not produced at all
  bool planes_ranged = false;      // every row is produced, count planes only for [keep_begin, keep_end) and the shard
  int64_t keep_begin = 0, keep_end = 0;
  // thresholds shared with the other devices during the join (gcre_join_opts.exchange)
  int exchanges = 0;
  int (*exchange)(void*, void*, int32_t, int32_t) = nullptr;
  void* exchange_user = nullptr;
  gcre_gene_tally* tally = nullptr;   // the join's scored paths are folded into it (never set on a registered later join)
  gcre_exceed* exceed = nullptr;      // the join's null values and observed scores are counted into it (the same)
  bool exceed_observed = true;        // ... the observed scores too (false: a later permutation window of the same join)
  gcre_hits* hits = nullptr;          // the join's scored paths at or above the list's cut-off are appended to it (the same)
  void take(const gcre_join_opts* o) {
    if (!o) return;
    if (o->keep_ranged) {
      keep_ranged = o->keep_ranged == 1;
      planes_ranged = o->keep_ranged == 2;
      keep_begin = o->keep_begin;
      keep_end = o->keep_end;
    }
    if (o->exchange && o->exchanges > 0 && o->d_null_out) {
      exchanges = o->exchanges;
      exchange = o->exchange;
      exchange_user = o->exchange_user;
    }
  }
};

// records the message and the code on the context (without one: for gcre_last_error(NULL)) and returns the code
int fail(gcre_ctx* c, int code, const std::string& msg);
// d_mt from d_masks as they are now, where the sparse kernel will read it: every entry that writes the masks ends here
int build_transposed_masks(gcre_ctx* c);

#define HIP_TRY(ctx, expr)                                                                            \
  do {                                                                                                \
    hipError_t e__ = (expr);                                                                          \
    if (e__ != hipSuccess)                                                                            \
      return fail((ctx), GCRE_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__));        \
  } while (0)

// The device scratch of one call: typed arrays that are freed when it ends, and the first HIP error of the call.  Once an
// error is set every further step does nothing, so a call queues its steps in order and looks at `e` where it used to.
struct DevScratch {
  hipStream_t st;
  hipError_t e = hipSuccess;
  std::vector<void*> held;
  explicit DevScratch(hipStream_t stream) : st(stream) {}
  DevScratch(const DevScratch&) = delete;
  DevScratch& operator=(const DevScratch&) = delete;
  ~DevScratch() { release(); }
  bool ok() const { return e == hipSuccess; }
  void release() {
    for (void* p : held) (void)hipFree(p);
    held.clear();
  }
  template <typename T>
  T* take(size_t n) {
    void* p = nullptr;
    if (ok()) e = hipMalloc(&p, n * sizeof(T));
    if (p) held.push_back(p);
    return (T*)p;
  }
  template <typename T>
  void upload(T* dst, const T* src, size_t n) { if (ok()) e = hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, st); }
  template <typename T>
  T* put(const T* src, size_t n) {   // take + upload
    T* dst = take<T>(n);
    upload(dst, src, n);
    return dst;
  }
  template <typename T>
  void download(T* dst, const T* src, size_t n) { if (ok()) e = hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, st); }
  template <typename T>
  void zero(T* dst, size_t n) { if (ok()) e = hipMemsetAsync(dst, 0, n * sizeof(T), st); }
  void sync() { if (ok()) e = hipStreamSynchronize(st); }
};

}  // namespace gcre_host
using namespace gcre_host;

struct gcre_ctx {
  Geometry g{};
  int device = 0;
  int top_k = 12;   // JoinExec::top_k, gcre.h:120
  hipStream_t stream = nullptr;
  // the top-k selection of a chunk only reads the keys its inspector wrote: it runs beside the warm-up slice and the
  // null kernel on a stream of its own (GCRE_SELECT_STREAM=0: on the main stream, as in round 1)
  hipStream_t sel_stream = nullptr;
  hipEvent_t ev_sel = nullptr, ev_sel_done = nullptr;
  bool sel_async = true;
  // GCRE_SELECT_DEFER=0: an ahead inspection closes its selection itself, before its join is launched (the order until the
  // launch learned to close it behind its null kernels; A/B runs, tests)
  bool sel_defer = true;
  // keys the radix select's candidate buffer holds (GCRE_SELECT_CAND; 256 KB): after two digit passes the keys that still
  // matter are copied there and the other six passes read them instead of every key.  0, or GCRE_SELECT_PASSES=8: eight
  // passes over all keys (A/B runs, tests)
  int sel_cand = 32768;
  // The recipe gather of a pruned method-1 launch (k_fill_rec_segs) is read by the pruned kernels only, not by the warm-up
  // slice in front of them: it runs beside the slice on a stream of its own (GCRE_REC_STREAM=0: on the join's stream, in
  // front of the slice).  ev_rec_in: on the join's stream where the gather is queued -- behind the recipe copies, the
  // segment-table upload and every earlier pruned launch, all of which are on that stream; ev_rec_done: behind the gather
  hipStream_t rec_stream = nullptr;
  hipEvent_t ev_rec_in = nullptr, ev_rec_done = nullptr;
  bool rec_async = true;
  // Inspect-ahead (gcre_join_ahead, round 4).  The inspector of the NEXT join of a sequence only needs what the current
  // join's inspector wrote (kept rows, recipe) -- not its permutation kernel -- so it runs on a stream of its own while
  // that kernel is in flight, into the next join's inspection cache; the next join then starts at its null kernel.
  hipStream_t insp_stream = nullptr;
  hipEvent_t ev_insp_done = nullptr;    // recorded on insp_stream when an ahead inspection has queued all its work
  hipEvent_t ev_insp_main = nullptr;    // recorded on the main stream behind the last inspector that ran there
  hipEvent_t ev_tail = nullptr;         // behind a join's own result copies, before the chain it launches
  uint32_t* d_max_tot_b = nullptr;      // the flag block of ahead inspections (the null kernel in flight owns d_max_tot)
  std::vector<JoinPlan>* ahead = nullptr;   // the registered later joins of the sequence, consumed by the next join call
  bool ahead_closed = false;            // a join that cannot run ahead was offered: nothing behind it is registered either
  bool ahead_on = true;                 // GCRE_AHEAD=0 turns gcre_join_ahead into a no-op.  The caller decides which joins to register:
                                        // measured, the chain is worth 8 % on configs[1] (host gaps between small joins) and
                                        // 0.5 % on configs[2] -- there the next level's inspector and this level's permutation
                                        // kernel each fill the GPU (26.1 + 9.9 ms of kernel time inside 31.1 ms instead of
                                        // 23.0 + 6.0 one after the other)
  SelectState h_sel{};               // where the digit passes' state lands (outlives any one chunk: the copy is asynchronous)
  std::string err;
  int last_code = GCRE_OK;
  bool quiet = false;
  bool have_table = false, have_perms = false;
  int64_t chunk_paths = int64_t(1) << 25;
  int null_blocks_per_cu = 12;
  int cus = 256;                     // compute units of the device (read once at gcre_create)
  int64_t overlap_launches = 0;      // k_set_overlap launches of this context (gcre_overlap_launches)
  int64_t stepdown_launches = 0;     // k_stepdown_null / k_stepdown_finish launches of this context (gcre_stepdown_launches)
  int64_t clump_launches = 0;        // kernels gcre_clump_sets launched on this context (gcre_clump_launches)
  int64_t given_launches = 0;        // kernels gcre_score_sets_given launched on this context (gcre_given_launches)
  int64_t patient_launches = 0;      // kernels gcre_set_patient_counts launched on this context (gcre_patient_launches)
  int64_t burden_launches = 0;       // kernels gcre_patient_burden launched on this context (gcre_burden_launches)
  int64_t family_launches = 0;       // k_family_null / _scan / _hist launches of this context (gcre_family_launches)
  int64_t minp_launches = 0;         // k_minp_gather / k_family_null / k_minp_rank / _scan launches of gcre_score_sets_minp
  int64_t compete_launches = 0;      // k_compete_null launches of gcre_score_sets_compete (gcre_compete_launches)
  int64_t prefix_launches = 0;       // kernels gcre_score_sets_prefix launched for its own stage (gcre_prefix_launches)
  int64_t subsample_launches = 0;    // kernels gcre_score_sets_subsample launched for its own stage (gcre_subsample_launches)
  int64_t dose_launches = 0;         // kernels gcre_score_sets_dose launched for its own stage (gcre_dose_launches)
  int64_t sequential_launches = 0;   // kernels gcre_score_sets_sequential launched for its own stage (gcre_sequential_launches)
  int64_t seq_prefix_launches = 0;   // kernels gcre_score_sets_prefix_sequential / _dose_sequential launched for their own stage (gcre_seq_prefix_launches)
  int64_t strata_launches = 0;       // kernels gcre_score_sets_strata launched for its own stage (gcre_strata_launches)
  int64_t weighted_launches = 0;     // k_weighted_search / k_weighted_write launches of this context (gcre_weighted_launches)

  // resident inputs
  uint64_t* d_case_mask = nullptr;   // [Wp]
  uint32_t* d_masks = nullptr;       // [W32p][Kpad]
  float* d_t32 = nullptr;            // method 1 null table
  double* d_dvt = nullptr;           // observed-score table
  double* d_dmax = nullptr;          // method 2 null table (vtmax)
  double* d_dmaxn = nullptr;         // its mirror image, only where vtmax is not symmetric (a NaN on one side of the diagonal)
  uint32_t* d_null = nullptr;        // [Kpad]
  uint32_t* d_mt = nullptr;          // transposed masks for the sparse kernel [nkt][64*Wp + 1][64]
  bool mt_stale = false;             // d_masks changed while the sparse kernel was off: d_mt (if any) holds older masks
  int ieq_batch = 0;                 // GCRE_IEQ_BATCH: quads per ticket of the quad kernel (0: twice ie_batch)
  int ie_quad = 1;                   // GCRE_IE_QUAD=0: the pruned method-1 launches stay on k_null_ie_m1 (cross-check)
  int ie_flagq = 1;                  // GCRE_IE_FLAGQ=0: the quad kernel's second look + exact pass instead of the flag queue (A/B runs, tests)
  int stats_ie_counts = 1;           // GCRE_STATS_IE_COUNTS=0: the method-1 inspector counts every joined row's words (A/B runs, tests)
  int ie_zwide = 0;                  // GCRE_IE_ZWIDE=1: the quad kernel reaches every added row through a descriptor of its own (tests)
  int ie_warm_items = 4;             // (segment, tile) items per wave of the warm-up launch (GCRE_IE_WARM_ITEMS)
  int ie_warm_div = 4096;            // the slice grows with the join as scored segments / this (GCRE_IE_WARM_DIV; warm_segments)
  int ie_warm_cap_div = 8;           // ... and is at most scored segments / this, at least 256 (GCRE_IE_WARM_CAP_DIV; warm_segments)
  int exchange_tail = 0;             // slices of the pruned launch that are equal steps at its end (GCRE_EXCHANGE_TAIL; -1: half of them; 0: doubling slices only)
  int ie_warm_segs = 1024;           // least number of segments in the warm-up slice (GCRE_IE_WARM; 2048 until round 3: the filter's second look made early thresholds matter less)
  int ie_small_join_tiles = 8;       // GCRE_IE_SJT (tuning)
  int ie_batch = 2;                  // segments per ticket (GCRE_IE_BATCH)
  uint32_t* d_queue = nullptr;       // ticket counters of the pruned kernels' work queues (8 x 16 words)
  uint32_t* d_max_tot = nullptr;     // the flag block of the inspectors (FlagWord, gcre_kernels.h)
  uint32_t* d_ladder = nullptr;      // method 1: pruning ladder of the null table [kLadderLevels][TD]
  uint32_t g00_rows = 0xffffffffu;   // method 2: vtmax[0][0] in ladder rows, rounded up (IeArgs::g00_rows)
  int null_kernel = 0;               // 0 auto, 1 dense, 2 sparse, 3 ie (GCRE_NULL_KERNEL)
  int sparse_waves_per_cu = 32;
  int ie_prune = 1;                  // GCRE_IE_PRUNE=0 looks every count up (diagnostics)
  uint64_t mask_epoch = 0;           // bumped whenever the permutation masks change: count planes are per epoch
  uint64_t obs_epoch = 0;            // bumped whenever the value table changes: observed scores (keys, winners) are per epoch
  bool insp_cache = false;           // gcre_set_inspect_cache: a join's inspector output stays with its join index
  ExchangeHub* hub = nullptr;        // set by gcre_process_paths_devices for the duration of a call
  struct ncclComm* comm = nullptr;   // ... and this device's RCCL communicator when the devices are distinct and RCCL loads
  int64_t rccl_calls = 0;            // collectives this context issued during the call (diagnostics, tests)
  DevBuf<float> d_hub_null;          // the maxima this device hands to the hub
  int hub_level = 0, hub_round = 0;  // what the next exchange of this device is: part of the hub's round tag
  // permutation window [win_k0, win_k0 + win_K): what a join scores.  The whole range by default; gcre_set_perm_window
  // narrows it so that the count planes of the kept sets (one per 2048-permutation tile) fit in device memory
  int win_k0 = 0, win_K = 0;
  int win_K_nominal = 0;   // the largest window since the masks were set: whether a kept set leaves with planes or with a recipe
                           // is decided for THAT size, so that a short last window does not flip the decision (and hipMalloc
                           // gigabytes of planes for one window: 120-460 ms on a fresh context)

  // per-join scratch
  ChunkBufs scratch;                 // a chunk's buffers when the inspection cache is off
  DevBuf<uint32_t> d_sel, d_small, d_chunk, d_rec_segs;
  DevBuf<uint64_t> d_wkey, d_cand, d_doff, d_scan, d_excess, d_excess_b;
  DevBuf<uint64_t> d_ie_timing;      // GCRE_IE_TIMING: the section counters of a diagnostics build's pruned kernels

  // count-plane buffers of freed path sets, kept for the next set that needs one (hipMalloc of tens of GB costs
  // ~40 ms per GB on this platform, hipFree nothing)
  struct PlaneBuf { uint32_t* p; size_t bytes; };
  std::vector<PlaneBuf> plane_pool;
  // live path sets by id: a recipe names its operands by id + version, never by pointer alone
  std::unordered_map<uint64_t, const gcre_pathset*> live_sets;
  std::vector<gcre_uids*> live_uids;   // join indices created on this context (gcre_destroy releases what is still alive)
  // per-gene best-path tallies (gcre_gene_tally): the ones alive on this context, the one the next join
  // folds into (gcre_join_set_tally), and the ones the next gcre_process_paths hands to its levels
  std::vector<gcre_gene_tally*> live_tallies;
  gcre_gene_tally* armed_tally = nullptr;
  gcre_gene_tally* pp_tally[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // null exceedance counts (gcre_exceed): alive, armed for the next join, armed for the next gcre_process_paths
  std::vector<gcre_exceed*> live_exceeds;
  gcre_exceed* armed_exceed = nullptr;
  gcre_exceed* pp_exceed[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // hit lists (gcre_hits): the same three, and the k_hits_collect launches since gcre_create
  std::vector<gcre_hits*> live_hits;
  gcre_hits* armed_hits = nullptr;
  gcre_hits* pp_hits[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int64_t hits_launches = 0;
  uint64_t next_set_id = 0;
  size_t planes_out_max = (size_t)8 << 30;   // kept sets (method 1) whose planes are larger keep a recipe only

  gcre_profile prof{};
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_null, ev_stats;
  std::vector<hipEvent_t> ev_pool;
};

// How a kept path set was made: row r = row row0[r] of set A | row rowz[r] of set Z, with the producing
// join's list (the overlap of the two rows, or what Z adds) as its inspector left it.  Enough to rebuild the count
// planes of any row for any permutation tile from the planes of A and Z, so the set's own planes (3 KB per row and
// tile) need not be stored, written or read.  Independent of the masks.
struct gcre_recipe {
  uint64_t a_id = 0, z_id = 0;     // the operands: path-set ids and the versions of their rows
  uint64_t a_ver = 0, z_ver = 0;
  DevBuf<uint32_t> row0, rowz, linfo, lover, slot, over, tot;   // tot: carriers of every kept row
  uint32_t max_len = 0;            // longest list (padded) the producing join's inspector wrote
  bool valid = false;
  void release() {
    for (auto* b : {&row0, &rowz, &linfo, &lover, &slot, &over, &tot}) b->release();
    valid = false;
  }
};

struct gcre_pathset {
  gcre_ctx* ctx;
  int64_t nrows;
  uint64_t* d_rows;   // max(nrows,1) x S words
  uint64_t id = 0;                 // never reused inside a context
  mutable uint64_t version = 0;    // bumped when the rows are rewritten
  mutable gcre_recipe* rec = nullptr;
  // CSR bit lists for the sparse kernel, built on first use and dropped whenever the rows are rewritten
  mutable uint64_t* d_loff = nullptr;
  mutable uint32_t* d_lidx = nullptr;
  mutable std::vector<uint64_t> h_loff;   // host copy of the offsets (sizes the work of a sparse launch)
  mutable uint32_t max_bits = 0;          // longest list (entries incl. padding): bounds the carriers of any row
  mutable bool max_known = false;
  mutable int one_sided = -1;             // method 2: every row has an empty half (-1: not looked at; from h_loff)
  // method 1: carriers | carriers among the cases << 16 of every row (k_row_counts), for the inspector of a join that has
  // this set as its reduced operand; built on first use, dropped with the lists.  counts_on: the stream that built them,
  // counts_ev: recorded behind the kernel -- an inspector on another stream waits for it
  mutable uint32_t* d_counts = nullptr;
  mutable hipStream_t counts_on = nullptr;
  mutable hipEvent_t counts_ev = nullptr;
  // count planes for the inclusion-exclusion kernel: [tile][row*M+h][groups][64][4] dwords, valid for one mask epoch
  mutable uint32_t* d_planes = nullptr;
  mutable int plane_groups = 0;
  mutable size_t planes_bytes = 0;   // capacity of d_planes
  mutable uint64_t planes_epoch = 0;
  mutable bool planes_valid = false;
  mutable int64_t planes_lo = 0, planes_hi = 0;   // rows whose planes are valid (a multi-device join fills a range)
  mutable bool planes_wanted = false;   // a later join had to rebuild this set's planes from its bit lists: next time the
                                        // join that writes its rows leaves the planes too, whatever their size
};

// UidRelSet (src/gcre.h:49-90) resident on the device: prefix sums of count, locations, signs
struct gcre_uids {
  gcre_ctx* ctx;
  int path_length;
  int64_t n_uids;
  int64_t n_signs;
  int64_t total;      // count_total_paths()
  int64_t max_loc;    // largest paths1 row referenced, -1 if none
  int64_t max_idx;    // largest uid row with count > 0, -1 if none
  int64_t* d_path_idx;
  int64_t* d_location;
  int32_t* d_signs;
  std::vector<int64_t> h_path_idx;   // host copy, for building the sparse kernel's segment tables
  mutable std::vector<int64_t> h_nonempty;   // prefix count of the uids with count > 0 (built on first use)
  std::vector<int64_t> h_location;   // host copy: segments are ordered by the paths1 rows they join (L2 reuse of their planes)
  struct SegCache {
    int64_t first, count, score_b, score_e, plane_b, plane_e;
    int64_t nsegs, nscored;
    SparseSeg* d_segs;
    // quad table of the pruned method-1 kernel (gcre_ieq.hip), built on first use for one warm-up length: runs of up to
    // four consecutive segments that join the same paths1 rows, none straddling `q_warm` or `nscored`
    std::vector<SparseSeg> h_segs;
    int64_t q_warm = -1, nquads = 0, quad_begin = 0;
    uint32_t* d_quads = nullptr;
  };
  mutable std::vector<SegCache> seg_cache;
  // A segment table (and its quads) built ahead of the join that will ask for it, by a helper thread that touches nothing
  // but the host copies of the join index (gcre_process_paths: the last level's tables while the first levels run)
  struct Prefetch {
    int64_t first = 0, count = 0, score_b = 0, score_e = 0, plane_b = 0, plane_e = 0;
    std::vector<SparseSeg> segs;
    int64_t nscored = 0;
    std::vector<uint32_t> quads;
    int64_t q_warm = -1, quad_begin = 0;
    bool ready = false, quads_ready = false, quads_for_table = false;
    std::thread th;
  };
  mutable std::unique_ptr<Prefetch> prefetch;
  // inspection cache (gcre_set_inspect_cache): the inspector output of the last join that ran on this index, per chunk,
  // valid while the operands' rows, the kept set, the shard and the observed-score inputs are the same
  mutable std::deque<ChunkInsp> insp;
  mutable InspKey insp_key;
  mutable bool insp_valid = false;       // the join completed: every chunk entry describes it
  mutable bool insp_hinted = false;      // ... with the reduced operand standing (the hint was not broken)
  mutable uint64_t insp_res_ver = 0;     // version of the kept set's rows as that join left them
  // A join on this index whose permutation kernels were LAUNCHED ahead (gcre_join_ahead chain): they write into the index's
  // own maxima, the winners are the inspection cache's; the join call that comes for it only waits, copies and merges
  struct Launched {
    bool active = false;
    InspKey key;
    uint64_t res_ver = 0, mask_epoch = 0;
    int win_k0 = 0, win_K = 0;
    std::vector<Candidate> cands;
    DevBuf<uint32_t> d_null;              // Kpad running maxima + one word: the launch's look-up counter
    hipEvent_t done = nullptr;            // behind the last kernel of the launch (main stream)
    hipEvent_t sel_done = nullptr;        // behind the winners' copies of the selections the launch closed (selection stream)
    bool sel_pending = false;             // some chunk entry holds such copies (ChunkInsp::win_pending)
    gcre_profile prof{};                  // what the ahead inspection and the launch accumulated for this join
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_null, ev_stats;
  };
  mutable Launched launch;
  // optional hint (gcre_uids_set_reduced): paths0[idx] | paths1[loc] == paths0[idx] | red[red_index[loc]] for every
  // joined path; checked on the device for every join, ignored when it does not hold
  const gcre_pathset* red = nullptr;
  uint64_t red_id = 0;             // the set's id: a freed operand is noticed, not dereferenced
  int32_t* d_red_index = nullptr;
  int64_t n_red_index = 0;
  // distinct (location, count) ranges of the uids (all uids with the same pivot gene share one): built on first use
  mutable int64_t n_ranges = -1;
  mutable int32_t* d_range_of = nullptr;    // uid -> range
  mutable int64_t n_pairs = 0;              // sum of the range lengths: the paths1 rows the range check reads
  mutable int64_t n_pieces = 0, n_cut = 0;  // the ranges as the range check walks them (RangePiece), and those cut in pieces
  mutable RangePiece* d_pieces = nullptr;
  mutable int32_t* d_cut = nullptr;
};

// The per-gene best-path table of one join: which slots a joined path touches -- through its paths0 row
// and through its paths1 row -- and, per slot, the best joined path seen so far under (key, then smaller ordinal).
struct gcre_gene_tally {
  gcre_ctx* ctx = nullptr;
  int n_slots = 0;
  int64_t n_rows0 = 0, n_rows1 = 0;
  int w0 = 0, w1 = 0;                 // 0: the operand contributes no gene
  int32_t *d_genes0 = nullptr, *d_genes1 = nullptr;
  uint64_t* d_ck = nullptr;           // chunk-local tables: empty between folds (k_gene_merge leaves them so)
  uint32_t* d_cidx = nullptr;
  uint64_t* d_bkey = nullptr;         // the table
  int64_t* d_bord = nullptr;
  int32_t *d_bsrc = nullptr, *d_btrg = nullptr, *d_bcases = nullptr, *d_bctrls = nullptr;
  hipStream_t last = nullptr;         // the stream of the last fold: a read waits for it
  bool folded = false;                // the table holds something (k_gene_fold then also tests against it)
  bool folding = false;               // a fold did not get all its launches queued: the chunk-local tables are cleared first
};

// Null exceedance counts of one list of thresholds.  The thresholds are kept sorted ascending on the
// device, as f32 bit patterns for the null values and as score keys for the observed scores; a counted value lands in the
// bin of the largest threshold it reaches, and a read sums the bins from each threshold upwards.  Sums: every chunk counted
// adds, whichever stream it ran on.
struct gcre_exceed {
  gcre_ctx* ctx = nullptr;
  int m = 0;
  std::vector<int32_t> order;         // sorted position -> the caller's index
  std::vector<double> thr;            // the thresholds as given (gcre_exceed_stepdown compares scores with them)
  uint32_t* d_pat = nullptr;          // [m] ascending
  uint64_t* d_tkey = nullptr;         // [m] ascending
  unsigned long long* d_hist = nullptr;    // [m] (path, permutation) pairs per bin
  unsigned long long* d_ohist = nullptr;   // [m] joined paths per bin
  int64_t perms = 0, paths = 0;       // permutations / joined paths that went into the bins
  // per-permutation counts (gcre_exceed_keep_perm_counts): cell [bin][r] = values of permutation r in the bin
  uint32_t* d_pc = nullptr;           // [m][pc_stride] u32, or nullptr: not kept
  int pc_stride = 0;                  // the context's Kpad
  std::vector<uint64_t> pc_load;      // per 2048-permutation tile: joined paths counted into its permutations' cells
};

// The hit list of one cut-off: the records of the joined paths whose observed score reaches it, in the
// order the waves reserved them, as struct-of-arrays carved out of one allocation of 32 x cap bytes, and the 64-bit
// cursor that counts every hit (also those past `cap`).  Appends: every chunk collected adds, whichever join it is of.
struct gcre_hits {
  gcre_ctx* ctx = nullptr;
  double cutoff = 0;
  uint64_t tkey = 1;                  // the cut-off as a score key (gcre_exceed's rule: either zero -> the key of -0.0, -inf -> 1)
  int64_t cap = 0;
  unsigned long long* d_cursor = nullptr;
  void* d_rec = nullptr;              // [cap] x (i64 ordinal, u64 key, i32 src, i32 trg, i32 cases, i32 ctrls), array after array
  int64_t paths = 0;                  // joined paths looked at
  int64_t* ord() const { return (int64_t*)d_rec; }
  uint64_t* key() const { return (uint64_t*)d_rec + cap; }
  int32_t* field(int k) const { return (int32_t*)((uint64_t*)d_rec + 2 * cap) + (int64_t)k * cap; }   // 0 src, 1 trg, 2 cases, 3 ctrls
};

// What the join driver (gcre_host.hip) shows the one-call pipeline (gcre_host_pipeline.hip)
namespace gcre_host __attribute__((visibility("hidden"))) {

int join_once(gcre_ctx* c, const JoinPlan& jp, gcre_result* out);   // run_join for a whole join
// validation that does not need the path sets (join_base.cpp:198-200 checks the rest in run_join)
gcre_uids* make_uids(gcre_ctx* c, int path_length, const int32_t* uid_count, const int64_t* uid_location, int64_t n_uids,
                     const int32_t* signs, int64_t n_signs);
void free_uids(gcre_uids* u);
gcre_pathset* new_pathset(gcre_ctx* c, int64_t nrows, bool zero);
size_t plane_bytes(const gcre_ctx* c, int64_t nrows, int groups);
bool sparse_enabled(const gcre_ctx* c);
bool inspect_cache_allowed();
// The segment table and the quads of join index `u` (P joined paths, none kept apart) for windows of `window` permutations,
// built by a helper thread that the join which asks for them -- or free_uids -- joins
void start_table_prefetch(gcre_ctx* c, gcre_uids* u, int64_t P, int window);

}  // namespace gcre_host

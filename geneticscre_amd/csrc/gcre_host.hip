// gcre_host.hip -- host side of libgcre_hip.so: the C ABI of include/gcre_hip.h on top of the gfx950
// kernels in gcre_kernels.hip.  Owns device memory, the stream and the join driver (JoinExec::join,
// reference src/join_base.cpp:189-264).  The state behind the handles is in gcre_host.h; the top-k merge (merge_scores /
// format_result, methods.h:25-39, join_base.cpp:138-154) is in gcre_pipeline.h, the ProcessPaths sequence
// (src/wrapper.cpp:216-276) on one device and on several in gcre_host_pipeline.hip; the entry points that do not touch the
// join driver are in gcre_host_sets.hip and the stage files beside it (set scores) and in gcre_host_stats.hip (generated
// permutation masks, decorated p-values, overlaps, the gene tally and the exceedance counts as objects).
//
// There is no CPU fallback: without a gfx950 device gcre_create fails with GCRE_ERR_DEVICE.
#include "gcre_host.h"

namespace {

thread_local std::string g_create_error;

// GCRE_POISON (diagnostics): count-plane buffers handed to a set start as 0x5A bytes instead of whatever was there, so
// that a read of rows nobody wrote shows in the results of a fresh process too (planes are data, never indices)
inline bool poison_fresh_planes() {
  static const bool on = std::getenv("GCRE_POISON") != nullptr && std::atoi(std::getenv("GCRE_POISON")) != 0;
  return on;
}
inline void poison_planes(void* p, size_t bytes) {
  if (!poison_fresh_planes() || !p) return;
  (void)hipDeviceSynchronize();
  (void)hipMemset(p, 0x5A, bytes);
  (void)hipDeviceSynchronize();
}

inline size_t tri(size_t t) { return t * (t + 1) / 2; }

// Dense int matrix -> packed bit rows ON THE HOST, before anything crosses PCIe (round 4).  What R hands the shim is hundreds
// of MB of 4-byte ints that carry one bit each (340 MB of genotypes twice and 200 MB of permutation labels at configs[2]):
// pageable host memory goes up at ~10 GB/s, so uploading the ints and packing them on the device cost the one-shot call more
// than its kernels.  Packed here they are 1/32 of that.  out[r][w] (stride `stride` words) gets bit b of word w set iff
// pred(value of (r, 64 w + b), 64 w + b).  Threads own whole word columns (column-major input: 64 consecutive columns are
// streamed once each, the word column is accumulated in a buffer that stays in cache) or row blocks (row-major input).
template <typename Pred>
void pack_bits_host(const int32_t* data, int64_t nrow, int ncol, bool col_major, uint64_t* out, size_t stride, Pred pred) {
  const int W = (ncol + 63) / 64;
  if (nrow <= 0 || W <= 0) return;
  unsigned T = std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
  if (const char* e = std::getenv("GCRE_PACK_THREADS")) T = (unsigned)std::max(1, std::atoi(e));
  if ((double)nrow * ncol < 4e6) T = 1;
  auto work = [&](unsigned t) {
    if (col_major) {
      std::vector<uint64_t> acc((size_t)nrow);
      for (int w = (int)t; w < W; w += (int)T) {
        std::fill(acc.begin(), acc.end(), 0);
        const int q1 = std::min(ncol, (w + 1) * 64);
        for (int q = w * 64; q < q1; q++) {
          const int32_t* col = data + (size_t)q * (size_t)nrow;
          const uint64_t bit = uint64_t(1) << (q & 63);
          for (int64_t r = 0; r < nrow; r++) acc[(size_t)r] |= pred(col[r], q) ? bit : 0;
        }
        for (int64_t r = 0; r < nrow; r++) out[(size_t)r * stride + (size_t)w] = acc[(size_t)r];
      }
    } else {
      const int64_t r0 = nrow * t / T, r1 = nrow * (t + 1) / T;
      for (int64_t r = r0; r < r1; r++) {
        const int32_t* row = data + (size_t)r * (size_t)ncol;
        for (int w = 0; w < W; w++) {
          uint64_t v = 0;
          const int q1 = std::min(ncol, (w + 1) * 64);
          for (int q = w * 64; q < q1; q++) v |= pred(row[q], q) ? uint64_t(1) << (q & 63) : 0;
          out[(size_t)r * stride + (size_t)w] = v;
        }
      }
    }
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < T; t++) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
}

// GCRE_HOST_TIMING=1: wall time of the host-side steps around the kernels (stderr)
struct HostTimer {
  const char* what;
  std::chrono::steady_clock::time_point t0;
  explicit HostTimer(const char* w) : what(w), t0(std::chrono::steady_clock::now()) {}
  ~HostTimer() {
    static const bool on = std::getenv("GCRE_HOST_TIMING") != nullptr;
    if (on) std::fprintf(stderr, "[host] %-28s %8.2f ms\n", what,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
};

}  // namespace

int gcre_host::fail(gcre_ctx* c, int code, const std::string& msg) {
  if (c) {
    c->err = msg;
    c->last_code = code;
  } else {
    g_create_error = msg;
  }
  return code;
}

namespace {

hipEvent_t get_event(gcre_ctx* c) {
  if (!c->ev_pool.empty()) {
    hipEvent_t e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

double drain_events(gcre_ctx* c, std::vector<std::pair<hipEvent_t, hipEvent_t>>& v) {
  double ms = 0;
  for (auto& pr : v) {
    float t = 0;
    if (hipEventElapsedTime(&t, pr.first, pr.second) == hipSuccess) ms += t;
    c->ev_pool.push_back(pr.first);
    c->ev_pool.push_back(pr.second);
  }
  v.clear();
  return ms;
}

}  // namespace

gcre_pathset* gcre_host::new_pathset(gcre_ctx* c, int64_t nrows, bool zero) {
  HostTimer ht("new_pathset");
  if (nrows < 0) {
    fail(c, GCRE_ERR_ARG, "negative path-set size");
    return nullptr;
  }
  // rows are addressed by 31-bit row numbers and 32-bit offsets in 32-byte units inside the null kernel
  const int64_t units = nrows * (int64_t)(c->g.S / 4);
  if (nrows >= (int64_t(1) << 31) || units >= (int64_t(1) << 32)) {
    fail(c, GCRE_ERR_RANGE, "path set too large for 32-bit row addressing");
    return nullptr;
  }
  auto* ps = new gcre_pathset{};
  ps->ctx = c;
  ps->nrows = nrows;
  ps->id = ++c->next_set_id;
  const size_t bytes = (size_t)std::max<int64_t>(nrows, 1) * c->g.S * sizeof(uint64_t);
  hipError_t me = hipMalloc((void**)&ps->d_rows, bytes);
  if (me != hipSuccess && !c->plane_pool.empty()) {   // pooled plane buffers are only a convenience
    (void)hipGetLastError();
    for (auto& pb : c->plane_pool) (void)hipFree(pb.p);
    c->plane_pool.clear();
    me = hipMalloc((void**)&ps->d_rows, bytes);
  }
  if (me != hipSuccess) {
    fail(c, GCRE_ERR_DEVICE, "hipMalloc failed for a path set of " + std::to_string(bytes) + " bytes");
    delete ps;
    return nullptr;
  }
  if (zero || nrows == 0) {
    if (hipMemsetAsync(ps->d_rows, 0, bytes, c->stream) != hipSuccess) {
      fail(c, GCRE_ERR_DEVICE, "hipMemsetAsync failed");
      (void)hipFree(ps->d_rows);
      delete ps;
      return nullptr;
    }
  }
  c->live_sets[ps->id] = ps;
  return ps;
}

// The sparse kernel needs counts that fit 16 bits (64*Wp < 65535 patients); GCRE_NULL_KERNEL=dense turns it off.
// (a table whose vtmax is not symmetric is scored by the dense kernel: the (-) half reads the mirror image there, the
// count-plane and delta-streaming kernels and their ladders index both halves of one table)
bool gcre_host::sparse_enabled(const gcre_ctx* c) {
  return c->null_kernel != 1 && c->g.K > 0 && 64 * c->g.Wp < 65535 && !c->d_dmaxn;
}

namespace {

// d_mt from d_masks as they are now
int transpose_masks(gcre_ctx* c) {
  const Geometry& g = c->g;
  const int nkt = (g.K + kSparseTile - 1) / kSparseTile;
  const uint32_t mt_rows = (uint32_t)(64 * g.Wp + 1);
  const size_t bytes = (size_t)nkt * mt_rows * 64 * 4;
  if (!c->d_mt) HIP_TRY(c, hipMalloc((void**)&c->d_mt, bytes));
  HIP_TRY(c, hipMemsetAsync(c->d_mt, 0, bytes, c->stream));
  HIP_TRY(c, launch_build_mt(c->d_masks, 2 * g.Wp, g.Kpad, nkt, mt_rows, c->d_mt, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->mt_stale = false;
  return GCRE_OK;
}

}  // namespace

// The permutation masks have changed.  Whatever was derived from the old ones is void whether or not the count-plane
// kernels are on at this moment: a later value table can turn them on again (sparse_enabled), and must then find neither
// the old transposed copy nor count planes or a launch-ahead record of the old epoch.
int gcre_host::build_transposed_masks(gcre_ctx* c) {
  c->mask_epoch++;   // every count plane built so far belongs to the old masks
  c->mt_stale = true;
  if (!sparse_enabled(c)) return GCRE_OK;   // (gcre_set_value_table makes the copy if a table brings the kernels back)
  if (int rc = transpose_masks(c)) return rc;
  c->win_k0 = 0;
  c->win_K = c->g.K;
  c->win_K_nominal = 0;
  return GCRE_OK;
}

namespace {

void drop_planes(const gcre_pathset* ps) {
  if (ps->d_planes) {
    gcre_ctx* c = ps->ctx;
    if (c) {
      c->plane_pool.push_back({ps->d_planes, ps->planes_bytes});
      if (c->plane_pool.size() > 8) {   // keep the eight largest
        size_t small = 0;
        for (size_t k = 1; k < c->plane_pool.size(); k++)
          if (c->plane_pool[k].bytes < c->plane_pool[small].bytes) small = k;
        (void)hipFree(c->plane_pool[small].p);
        c->plane_pool.erase(c->plane_pool.begin() + (long)small);
      }
    } else {
      (void)hipFree(ps->d_planes);
    }
  }
  ps->d_planes = nullptr;
  ps->planes_bytes = 0;
  ps->plane_groups = 0;
  ps->planes_valid = false;
}

void drop_row_counts(const gcre_pathset* ps);

void drop_lists(const gcre_pathset* ps) {
  drop_row_counts(ps);
  if (ps->d_loff) (void)hipFree(ps->d_loff);
  if (ps->d_lidx) (void)hipFree(ps->d_lidx);
  ps->d_loff = nullptr;
  ps->d_lidx = nullptr;
  ps->h_loff.clear();
  ps->max_bits = 0;
  ps->max_known = false;
  ps->one_sided = -1;
  drop_planes(ps);
}

// CSR bit lists of a path set (method 1: one list per row): offsets on the host by prefix sum, entries on the device
int ensure_lists(gcre_ctx* c, const gcre_pathset* ps) {
  if (ps->d_loff) return GCRE_OK;
  HostTimer ht("ensure_lists");
  const Geometry& g = c->g;
  // method 2: every row is two half-rows (+)/(-) of W32p dwords, stored back to back -> 2*nrows lists
  const int64_t n = ps->nrows * g.method;
  const int hs32 = 2 * g.Wp;   // dwords per half-row == stride between half-rows
  std::vector<uint32_t> cnt((size_t)std::max<int64_t>(n, 1), 0);
  uint32_t* d_cnt = nullptr;
  HIP_TRY(c, hipMalloc((void**)&d_cnt, cnt.size() * 4));
  hipError_t e = launch_row_bits((const uint32_t*)ps->d_rows, n, hs32, hs32, d_cnt, c->stream);
  if (e == hipSuccess && n > 0) e = hipMemcpyAsync(cnt.data(), d_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d_cnt);
  if (e != hipSuccess) return fail(c, GCRE_ERR_DEVICE, std::string("row lists: ") + hipGetErrorString(e));
  std::vector<uint64_t> off((size_t)n + 1, 0);
  uint32_t longest = 0;
  for (int64_t r = 0; r < n; r++) {
    off[(size_t)r + 1] = off[(size_t)r] + cnt[(size_t)r];
    longest = std::max(longest, cnt[(size_t)r]);
  }
  const uint64_t total = off[(size_t)n];
  HIP_TRY(c, hipMalloc((void**)&ps->d_loff, off.size() * 8));
  HIP_TRY(c, hipMalloc((void**)&ps->d_lidx, (size_t)(total + 16) * 4));
  e = hipMemcpyAsync(ps->d_loff, off.data(), off.size() * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = launch_row_fill((const uint32_t*)ps->d_rows, n, hs32, hs32, ps->d_loff, (uint32_t)(64 * g.Wp) << 8,
                        ps->d_lidx, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // off is a local
  if (e != hipSuccess) {
    drop_lists(ps);
    return fail(c, GCRE_ERR_DEVICE, std::string("row lists: ") + hipGetErrorString(e));
  }
  ps->h_loff = std::move(off);
  ps->max_bits = longest;
  ps->max_known = true;
  return GCRE_OK;
}

// method 2: does every row of the set have an empty half?  (genes: a row's carriers sit in one half.)  From the host copy of
// the list offsets, once per set of lists.
bool one_sided(const gcre_pathset* ps) {
  if (!ps->d_loff || ps->h_loff.size() != (size_t)ps->nrows * 2 + 1) return false;
  if (ps->one_sided < 0) {
    int yes = 1;
    for (int64_t r = 0; r < ps->nrows && yes; r++)
      if (ps->h_loff[(size_t)2 * r + 1] > ps->h_loff[(size_t)2 * r] && ps->h_loff[(size_t)2 * r + 2] > ps->h_loff[(size_t)2 * r + 1]) yes = 0;
    ps->one_sided = yes;
  }
  return ps->one_sided == 1;
}

void drop_row_counts(const gcre_pathset* ps) {
  if (ps->d_counts) (void)hipFree(ps->d_counts);
  if (ps->counts_ev) (void)hipEventDestroy(ps->counts_ev);
  ps->d_counts = nullptr;
  ps->counts_ev = nullptr;
  ps->counts_on = nullptr;
}

// method 1: the row totals of a reduced operand (gcre_pathset::d_counts) for an inspector of `paths` joined paths that is
// about to be queued on `st`, or nullptr where the inspector is to count the joined rows' words itself: the knob is off, or
// the set has more rows than the join has paths (counting them would cost more than it saves).  Built on `st` on first use.
int row_counts_for(gcre_ctx* c, const gcre_pathset* ps, int64_t paths, hipStream_t st, const uint32_t** out) {
  *out = nullptr;
  const Geometry& g = c->g;
  if (!c->stats_ie_counts || g.method != 1 || g.Wp > 160 || ps->nrows <= 0 || ps->nrows > paths) return GCRE_OK;
  if (!ps->d_counts) {
    HIP_TRY(c, hipMalloc((void**)&ps->d_counts, (size_t)ps->nrows * 4));
    hipError_t e = launch_row_counts(ps->d_rows, ps->nrows, g.Wp, c->d_case_mask, ps->d_counts, st);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ps->counts_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ps->counts_ev, st);
    if (e != hipSuccess) {
      drop_row_counts(ps);
      return fail(c, GCRE_ERR_DEVICE, std::string("row counts: ") + hipGetErrorString(e));
    }
    ps->counts_on = st;
  } else if (ps->counts_on != st) {
    HIP_TRY(c, hipStreamWaitEvent(st, ps->counts_ev, 0));
  }
  *out = ps->d_counts;
  return GCRE_OK;
}

// largest number of carriers a row of the set can have (from its lists, or from the join that produced it)
uint32_t row_max(const gcre_ctx* c, const gcre_pathset* ps) {
  return ps->max_known ? ps->max_bits : (uint32_t)(64 * c->g.Wp);
}

int plane_groups_for(uint32_t max_count) {
  int bits = 1;
  while (bits < 16 && (max_count >> bits) != 0) bits++;
  return std::max(2, (bits + 3) / 4);
}

// planes of rows [lo, hi) are there for the current masks
bool planes_cover(const gcre_ctx* c, const gcre_pathset* ps, int64_t lo, int64_t hi) {
  return ps->d_planes && ps->planes_valid && ps->planes_epoch == c->mask_epoch && (hi <= lo || (ps->planes_lo <= lo && hi <= ps->planes_hi));
}
bool planes_current(const gcre_ctx* c, const gcre_pathset* ps) { return planes_cover(c, ps, 0, ps->nrows); }

}  // namespace

size_t gcre_host::plane_bytes(const gcre_ctx* c, int64_t nrows, int groups) {
  const size_t nkt = (size_t)((c->win_K + kSparseTile - 1) / kSparseTile);
  return (size_t)std::max<int64_t>(nrows, 1) * c->g.method * nkt * (size_t)groups * 1024;
}

namespace {

// room for `bytes` more on the device, leaving a quarter of what is free for the scratch of the join itself
// `bytes` fit into three quarters of the free device memory (counting `reclaimable` bytes as free)
bool planes_fit(size_t bytes, size_t reclaimable = 0) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  free_b += reclaimable;
  return bytes < free_b - free_b / 4;
}

// the operands of a set's recipe, if the recipe is complete and both operands still hold the rows it was made from
bool recipe_operands(const gcre_ctx* c, const gcre_pathset* ps, const gcre_pathset** a, const gcre_pathset** z) {
  if (!ps->rec || !ps->rec->valid) return false;
  auto ia = c->live_sets.find(ps->rec->a_id), iz = c->live_sets.find(ps->rec->z_id);
  if (ia == c->live_sets.end() || iz == c->live_sets.end()) return false;
  if (ia->second->version != ps->rec->a_ver || iz->second->version != ps->rec->z_ver) return false;
  *a = ia->second;
  *z = iz->second;
  return true;
}

// allocate (not fill) the plane array of a set; false when it does not fit
bool alloc_planes(gcre_ctx* c, const gcre_pathset* ps, int groups) {
  HostTimer ht("alloc_planes");
  const size_t bytes = plane_bytes(c, ps->nrows, groups);
  if (ps->d_planes && ps->planes_bytes >= bytes) {   // its own buffer is large enough (another window, other groups)
    ps->plane_groups = groups;
    ps->planes_valid = false;
    poison_planes(ps->d_planes, ps->planes_bytes);
    return true;
  }
  drop_planes(ps);
  // smallest pooled buffer that is large enough
  int best = -1;
  for (size_t k = 0; k < c->plane_pool.size(); k++)
    if (c->plane_pool[k].bytes >= bytes && (best < 0 || c->plane_pool[k].bytes < c->plane_pool[(size_t)best].bytes)) best = (int)k;
  if (best >= 0) {
    ps->d_planes = c->plane_pool[(size_t)best].p;
    ps->planes_bytes = c->plane_pool[(size_t)best].bytes;
    c->plane_pool.erase(c->plane_pool.begin() + best);
  } else {
    if (!planes_fit(bytes)) {
      // make room -- pooled buffers that are too small are of no use to this set -- but only when that helps: a set
      // that cannot fit anyway (it will run on its recipe or on bit lists) must not cost the others their buffers
      size_t pooled = 0;
      for (const auto& pb : c->plane_pool) pooled += pb.bytes;
      if (!planes_fit(bytes, pooled)) return false;
      for (auto& pb : c->plane_pool) (void)hipFree(pb.p);
      c->plane_pool.clear();
      if (!planes_fit(bytes)) return false;
    }
    if (hipMalloc((void**)&ps->d_planes, bytes) != hipSuccess) {
      ps->d_planes = nullptr;
      (void)hipGetLastError();
      return false;
    }
    ps->planes_bytes = bytes;
  }
  poison_planes(ps->d_planes, ps->planes_bytes);
  ps->plane_groups = groups;
  return true;
}

// count planes of a path set from its bit lists (sets that were not produced by a kept join on this epoch).
// Returns GCRE_OK with planes_current() false when the planes do not fit in device memory.
int ensure_planes(gcre_ctx* c, const gcre_pathset* ps) {
  if (planes_current(c, ps)) return GCRE_OK;
  if (int rc = ensure_lists(c, ps)) return rc;
  const int groups = plane_groups_for(ps->max_bits);
  if (!alloc_planes(c, ps, groups)) return GCRE_OK;
  const Geometry& g = c->g;
  const int nkt = (c->win_K + kSparseTile - 1) / kSparseTile;
  const uint32_t* w_mt = c->d_mt + (size_t)(c->win_k0 / kSparseTile) * (size_t)(64 * g.Wp + 1) * 64;
  HIP_TRY(c, launch_build_planes(w_mt, (uint32_t)(64 * g.Wp + 1), nkt, ps->d_loff, ps->d_lidx, ps->nrows * g.method,
                                 groups, ps->d_planes, c->stream));
  ps->planes_epoch = c->mask_epoch;
  ps->planes_valid = true;
  ps->planes_lo = 0;
  ps->planes_hi = ps->nrows;
  return GCRE_OK;
}

// Segment table of the joined paths [first, first+count): runs of paths that share their paths0 row, at most
// kSparseSegMax long, none straddling the scored range [score_b, score_e).  The scored segments come first
// (*nscored of them); of the others only the paths inside [plane_b, plane_e) are listed (the rest need no count
// planes).  Cached per uids object (the join index is resident input; repeated joins reuse it).
// The host half of sparse_segments: the table itself (no device call: a helper thread may build it ahead of the join that
// needs it, gcre_uids::prefetch_tables).
void build_segments_host(const gcre_uids& u, int64_t first, int64_t count, int64_t score_b, int64_t score_e, int64_t plane_b,
                         int64_t plane_e, std::vector<SparseSeg>& segs, int64_t* nscored_out) {
  const auto& pi = u.h_path_idx;
  const int64_t end = first + count;
  // uids whose joined paths reach into [first, end)
  const int64_t i_lo = std::max<int64_t>(0, (int64_t)(std::upper_bound(pi.begin(), pi.end(), first) - pi.begin()) - 1);
  const int64_t i_hi = std::min<int64_t>(u.n_uids, (int64_t)(std::lower_bound(pi.begin(), pi.end(), end) - pi.begin()));
  // Millions of uids: the table is built by a few host threads, each over a contiguous piece of the uid range with
  // about the same number of joined paths (part 0: scored segments, part 1: the others; key = the paths1 row the SEGMENT
  // joins first: all uids with one pivot gene join the same rows, so equal keys = the same added rows, which is what the
  // quad kernel shares), and put together by a stable counting sort on the keys -- a noticeable part of a one-shot
  // gcre_process_paths call when done by one thread with a comparison sort.
  int T = 1;
  if (i_hi - i_lo > 200000) T = (int)std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency()));
  struct Local {
    std::vector<SparseSeg> part[2];
    std::vector<uint32_t> key[2];
    bool dense = true;
    uint32_t max_key = 0;
  };
  std::vector<Local> loc((size_t)T);
  std::vector<int64_t> cut((size_t)T + 1, i_hi);
  cut[0] = i_lo;
  for (int t = 1; t < T; t++) {
    const int64_t want = first + count * t / T;
    cut[(size_t)t] = std::min(i_hi, std::max(cut[(size_t)t - 1], (int64_t)(std::lower_bound(pi.begin() + i_lo, pi.begin() + i_hi, want) - pi.begin())));
  }
  auto build = [&](int t) {
    Local& L = loc[(size_t)t];
    const size_t guess = (size_t)(cut[(size_t)t + 1] - cut[(size_t)t]) + (size_t)(count / T / kSparseSegMax) + 16;
    L.part[score_e > score_b ? 0 : 1].reserve(guess);
    L.key[score_e > score_b ? 0 : 1].reserve(guess);
    for (int64_t i = cut[(size_t)t]; i < cut[(size_t)t + 1]; i++) {
      const int64_t lo = std::max(pi[(size_t)i], first), hi = std::min(pi[(size_t)i + 1], end);
      if (hi <= lo) continue;
      const int64_t l = u.h_location[(size_t)i];
      if (l < 0 || l > 0xfffffff0ll) L.dense = false;
      L.max_key = std::max(L.max_key, (uint32_t)l);
      // the uid's paths before, inside and after the scored range
      const int64_t pc[4] = {lo, std::min(std::max(score_b, lo), hi), std::min(std::max(score_e, lo), hi), hi};
      for (int piece = 0; piece < 3; piece++) {
        const int dst = (piece == 1) ? 0 : 1;
        int64_t a0 = pc[piece], a1 = pc[piece + 1];
        if (piece != 1) {   // planes only: clip to the rows that want them
          a0 = std::max(a0, plane_b);
          a1 = std::min(a1, plane_e);
        }
        for (int64_t a = a0; a < a1; a += kSparseSegMax) {
          L.part[dst].push_back(SparseSeg{(uint32_t)i, (uint32_t)(a - first), (uint32_t)std::min<int64_t>(kSparseSegMax, a1 - a)});
          const int64_t k = l + (a - pi[(size_t)i]);
          if (k > 0xfffffff0ll) L.dense = false;
          L.key[dst].push_back((uint32_t)k);
          L.max_key = std::max(L.max_key, (uint32_t)k);
        }
      }
    }
  };
  auto run_all = [&](const std::function<void(int)>& fn) {
    if (T == 1) { fn(0); return; }
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back(fn, t);
    fn(0);
    for (auto& x : th) x.join();
  };
  run_all(build);
  size_t n_part[2] = {0, 0};
  bool dense = true;
  uint32_t max_key = 0;
  for (const Local& L : loc) {
    n_part[0] += L.part[0].size();
    n_part[1] += L.part[1].size();
    dense = dense && L.dense;
    max_key = std::max(max_key, L.max_key);
  }
  const size_t n_scored = n_part[0];
  // Segments that join the same paths1 rows (all uids with the same pivot gene share `location`) run next to each
  // other: the waves of an XCD walk a contiguous window of this table, so the planes of those rows stay in its L2.
  // Any order gives the same maxima.
  segs.assign(n_part[0] + n_part[1], SparseSeg{});
  size_t base = 0;
  for (int q = 0; q < 2; q++) {
    const size_t nq = n_part[q];
    if (nq == 0) continue;
    const size_t nkeys = (size_t)max_key + 1;
    if (dense && (uint64_t)nkeys * (uint64_t)T <= ((uint64_t)64 << 20) && (uint64_t)max_key < (uint64_t)64 * nq + 1024) {
      // stable counting sort: per-thread histograms, then for every key the threads' slices one after the other
      std::vector<std::vector<uint32_t>> start((size_t)T);
      run_all([&](int t) {
        start[(size_t)t].assign(nkeys, 0);
        for (uint32_t k : loc[(size_t)t].key[q]) start[(size_t)t][k]++;
      });
      uint32_t run = 0;
      for (size_t k = 0; k < nkeys; k++)
        for (int t = 0; t < T; t++) {
          const uint32_t h = start[(size_t)t][k];
          start[(size_t)t][k] = run;
          run += h;
        }
      run_all([&](int t) {
        const Local& L = loc[(size_t)t];
        std::vector<uint32_t>& st = start[(size_t)t];
        for (size_t e = 0; e < L.part[q].size(); e++) segs[base + st[L.key[q][e]]++] = L.part[q][e];
      });
    } else {
      std::vector<SparseSeg> all;
      all.reserve(nq);
      for (const Local& L : loc) all.insert(all.end(), L.part[q].begin(), L.part[q].end());
      auto key_of = [&](const SparseSeg& x) { return u.h_location[x.row0] + ((int64_t)x.first + first - pi[x.row0]); };
      std::stable_sort(all.begin(), all.end(), [&](const SparseSeg& x, const SparseSeg& y) { return key_of(x) < key_of(y); });
      std::copy(all.begin(), all.end(), segs.begin() + (std::ptrdiff_t)base);
    }
    base += nq;
  }
  *nscored_out = (int64_t)n_scored;
}

// quads of a segment table (gcre_ieq.hip): runs of up to ieq_quad_segs() consecutive segments with the same first joined row and
// length, none straddling n_warm or nscored.  Host only.
void build_quads_host(const gcre_uids& u, const std::vector<SparseSeg>& segs, int64_t first, int64_t nscored, int64_t n_warm,
                      std::vector<uint32_t>& quads, int64_t* quad_begin_out) {
  const auto& pi = u.h_path_idx;
  const int64_t n = (int64_t)segs.size();
  quads.clear();
  int64_t quad_begin = -1;
  const int64_t qmax = ieq_quad_segs();
  quads.reserve((size_t)n / (size_t)std::max<int64_t>(1, (qmax + 1) / 2) + 16);
  auto key_of = [&](const SparseSeg& x) { return u.h_location[x.row0] + ((int64_t)x.first + first - pi[x.row0]); };
  int64_t i = 0;
  while (i < n) {
    if (i >= n_warm && quad_begin < 0) quad_begin = (int64_t)quads.size();
    const int64_t stop = i < n_warm ? n_warm : (i < nscored ? nscored : n);
    const int64_t k0 = key_of(segs[(size_t)i]);
    const uint32_t n0 = segs[(size_t)i].n;
    int64_t j = i + 1;
    while (j < stop && j < i + qmax && segs[(size_t)j].n == n0 && key_of(segs[(size_t)j]) == k0) j++;
    quads.push_back((uint32_t)i | ((uint32_t)(j - i - 1) << 30));
    i = j;
  }
  if (quad_begin < 0) quad_begin = (int64_t)quads.size();
  *quad_begin_out = quad_begin;
}

// segments of the warm-up slice of a pruned launch (run_join): the first n_warm scored segments are scored without pruning.
// A slice only has to leave every permutation of a tile with some non-zero maximum to prune against; once the pruned
// kernel runs, its waves' own finds (exchanged after 1, 2, 4, .. segments) outnumber the slice's many times over.  So
// the slice is ie_warm_segs segments (per eight tiles), and grows with the join only as nseg / ie_warm_div
// (GCRE_IE_WARM_DIV).  The divisor is 4096: at 1024 the benchmark's last level (2.3 million scored segments) had a slice
// of 2,270 segments, and the sweep (profiles/warmup_sweep.txt) took 0.27 ms less per pass with 1,024 although 1.5 % more
// path-tiles were then looked up; at 512 and 256 the look-ups cost more than the shorter slice saves.
// A small join gets less: at most nseg / ie_warm_cap_div (GCRE_IE_WARM_CAP_DIV), never below 256.  The divisor is 8:
// a shorter slice is not a faster one (the launch keeps about four items per wave, so it only has fewer waves), and at
// 32 and above the thinner thresholds cost the pruned launches more than the slices save (profiles/warm_size_sweep.txt).
int64_t warm_segments(const gcre_ctx* c, int64_t nseg_scored, int nkt) {
  if (c->ie_warm_segs == 0) return 0;   // GCRE_IE_WARM=0 (tests): everything through the pruned kernel, thresholds from 0
  const int64_t warm_min = std::max<int64_t>(256, (int64_t)c->ie_warm_segs * 8 / std::max(nkt, 8));
  return std::min<int64_t>(nseg_scored, std::min<int64_t>(std::max<int64_t>(warm_min, nseg_scored / c->ie_warm_div),
                                                          std::max<int64_t>(256, nseg_scored / c->ie_warm_cap_div)));
}

int sparse_segments(gcre_ctx* c, const gcre_uids& u, int64_t first, int64_t count, int64_t score_b, int64_t score_e,
                    int64_t plane_b, int64_t plane_e, const SparseSeg** d_out, int64_t* nsegs, int64_t* nscored,
                    gcre_uids::SegCache** entry = nullptr) {
  plane_b = std::max(plane_b, first);
  plane_e = std::min(plane_e, first + count);
  for (auto& sc : u.seg_cache)
    if (sc.first == first && sc.count == count && sc.score_b == score_b && sc.score_e == score_e && sc.plane_b == plane_b &&
        sc.plane_e == plane_e) {
      *d_out = sc.d_segs;
      *nsegs = sc.nsegs;
      *nscored = sc.nscored;
      if (entry) *entry = &sc;
      return GCRE_OK;
    }
  std::vector<SparseSeg> segs;
  int64_t n_scored_i = 0;
  gcre_uids::Prefetch* pf = u.prefetch.get();
  if (pf && pf->th.joinable()) {   // a table being built ahead: wait for it, whichever table this call wants
    HostTimer hw("prefetched tables: wait");
    pf->th.join();
  }
  if (pf && pf->ready && pf->first == first && pf->count == count && pf->score_b == score_b && pf->score_e == score_e &&
      pf->plane_b == plane_b && pf->plane_e == plane_e) {
    segs.swap(pf->segs);
    n_scored_i = pf->nscored;
    pf->ready = false;
    pf->quads_for_table = true;   // its quads belong to the table made now
  } else {
    HostTimer ht("sparse_segments");
    build_segments_host(u, first, count, score_b, score_e, plane_b, plane_e, segs, &n_scored_i);
  }
  const size_t n_scored = (size_t)n_scored_i;
  SparseSeg* d = nullptr;
  HIP_TRY(c, hipMalloc((void**)&d, std::max<size_t>(segs.size(), 1) * sizeof(SparseSeg)));
  if (!segs.empty())
    HIP_TRY(c, hipMemcpyAsync(d, segs.data(), segs.size() * sizeof(SparseSeg), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // segs is a local
  if (u.seg_cache.size() >= 64) {                // bound the cache: drop the oldest table
    (void)hipFree(u.seg_cache.front().d_segs);
    if (u.seg_cache.front().d_quads) (void)hipFree(u.seg_cache.front().d_quads);
    u.seg_cache.erase(u.seg_cache.begin());
  }
  u.seg_cache.push_back({first, count, score_b, score_e, plane_b, plane_e, (int64_t)segs.size(), (int64_t)n_scored, d});
  if (c->g.method == 1 && c->ie_quad) u.seg_cache.back().h_segs = std::move(segs);
  if (entry) *entry = &u.seg_cache.back();
  *d_out = d;
  *nsegs = u.seg_cache.back().nsegs;
  *nscored = (int64_t)n_scored;
  return GCRE_OK;
}

// Quad table of a cached segment table (see gcre_ieq.hip): greedy runs of up to ieq_quad_segs() consecutive segments with the same
// first joined paths1 row and the same length -- they join the same rows --, cut at `n_warm` (the pruned launch starts
// there) and at the end of the scored segments.  quad_begin = the first quad of the pruned launch.
int ensure_quads(gcre_ctx* c, const gcre_uids& u, gcre_uids::SegCache& sc, int64_t n_warm) {
  if (sc.q_warm == n_warm && sc.d_quads) return GCRE_OK;
  const int64_t n = (int64_t)sc.h_segs.size();
  if (n != sc.nsegs || n >= ((int64_t)1 << 30)) return GCRE_ERR_ARG;   // no host copy (or too many segments): the caller falls back
  std::vector<uint32_t> quads;
  int64_t quad_begin = 0;
  gcre_uids::Prefetch* pf = u.prefetch.get();
  if (pf && pf->quads_ready && pf->quads_for_table && pf->q_warm == n_warm && pf->first == sc.first && pf->count == sc.count &&
      pf->score_b == sc.score_b && pf->score_e == sc.score_e && pf->plane_b == sc.plane_b && pf->plane_e == sc.plane_e) {
    quads.swap(pf->quads);   // built ahead with the table
    quad_begin = pf->quad_begin;
    pf->quads_ready = false;
  } else {
    HostTimer ht("ensure_quads");
    build_quads_host(u, sc.h_segs, sc.first, sc.nscored, n_warm, quads, &quad_begin);
  }
  if (sc.d_quads) (void)hipFree(sc.d_quads);
  sc.d_quads = nullptr;
  HIP_TRY(c, hipMalloc((void**)&sc.d_quads, std::max<size_t>(quads.size(), 1) * 4));
  if (!quads.empty()) HIP_TRY(c, hipMemcpyAsync(sc.d_quads, quads.data(), quads.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // quads is a local
  sc.q_warm = n_warm;
  sc.nquads = (int64_t)quads.size();
  sc.quad_begin = quad_begin;
  return GCRE_OK;
}

// ---- top-k selection of one scored chunk: indices of the best min(k, valid) keys, ties cut in index order ----
// `key` = the keys of the scored paths (a chunk's key buffer + its first scored path): the indices are relative to it.
// Two halves, so that a caller with a read-back of its own (the inspector's flags) can fold the state's into it:
// select_begin queues the eight digit passes (one read-back of the state they leave, gcre_kernels.hip) and the copy
// of that state into *hs; select_finish -- after a stream synchronisation -- queues the collection of the winners, over all
// keys whatever the digit passes read (the index-ordered tie cut needs every key of the tie class in place).
int select_begin(gcre_ctx* c, const uint64_t* key, int64_t count, int k, SelectState* hs, hipStream_t sst) {
  *hs = SelectState{};
  if (count == 0 || k <= 0) return GCRE_OK;
  HIP_TRY(c, c->d_small.reserve(512));
  HIP_TRY(c, c->d_sel.reserve((size_t)k + 64));
  SelectState* d_state = (SelectState*)(c->d_small.p + 264);
  // the candidates of the third to eighth digit pass (gcre_kernels.hip); 0: every pass reads all keys.  One buffer per
  // context like the rest of the selection's scratch: it is written and read inside the digit passes of one selection,
  // which the selection stream runs one after the other
  const uint32_t cand_cap = (uint32_t)c->sel_cand;
  if (cand_cap) HIP_TRY(c, c->d_cand.reserve(cand_cap));
  HIP_TRY(c, launch_radix_select(key, count, std::min<int64_t>(k, count), c->d_small.p, d_state, cand_cap ? c->d_cand.p : nullptr,
                                 cand_cap, c->d_small.p + 257, sst));
  HIP_TRY(c, hipMemcpyAsync(hs, d_state, sizeof *hs, hipMemcpyDeviceToHost, sst));
  return GCRE_OK;
}

int select_finish(gcre_ctx* c, const uint64_t* key, int64_t count, int k, const SelectState& hs, uint32_t* n_selected,
                  hipStream_t sst) {
  *n_selected = 0;
  if (count == 0 || k <= 0) return GCRE_OK;
  uint32_t* d_counter = c->d_small.p + 256;
  const uint64_t prefix = hs.prefix;
  const int64_t need = hs.need, greater = hs.greater;
  const uint32_t eq_count = hs.eq_count;
  const uint64_t T = prefix;   // the need-th largest key overall
  HIP_TRY(c, hipMemsetAsync(d_counter, 0, sizeof(uint32_t), sst));
  uint32_t nsel = 0;
  // keys `thr` / `alt` tie: the `m` smallest ordinals among them go behind the `at` paths already collected
  auto cut_ties = [&](uint64_t thr, uint64_t alt, uint32_t m, int64_t at) -> int {
    const int64_t chunks = (count + 1023) / 1024;
    HIP_TRY(c, c->d_chunk.reserve((size_t)chunks));
    HIP_TRY(c, launch_eq_count(key, count, thr, alt, c->d_chunk.p, sst));
    std::vector<uint32_t> cnt((size_t)chunks);
    HIP_TRY(c, hipMemcpyAsync(cnt.data(), c->d_chunk.p, cnt.size() * 4, hipMemcpyDeviceToHost, sst));
    HIP_TRY(c, hipStreamSynchronize(sst));
    uint32_t run = 0;
    for (auto& v : cnt) {
      const uint32_t t = v;
      v = run;
      run += t;
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_chunk.p, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice, sst));
    HIP_TRY(c, launch_eq_collect(key, count, thr, alt, c->d_chunk.p, m, c->d_sel.p + at, sst));
    HIP_TRY(c, hipStreamSynchronize(sst));   // cnt must outlive the copy
    return GCRE_OK;
  };
  if (T == 0) {
    // fewer scorable paths than k: everything with a real score is selected
    HIP_TRY(c, launch_collect_gt(key, count, 0, c->d_sel.p, d_counter, (uint32_t)k, sst));
    nsel = (uint32_t)greater;
  } else if (T == kKeyPlusZero || T == kKeyMinusZero) {
    // the cut falls on a zero.  -0.0 and +0.0 are equal scores under two keys: every path above +0 is in, and the zeros of
    // either sign share what is left by ordinal (how many that is follows from the number of paths above +0, which the
    // digit passes only know when the threshold is +0 itself)
    HIP_TRY(c, launch_collect_gt(key, count, kKeyPlusZero, c->d_sel.p, d_counter, (uint32_t)k, sst));
    uint32_t above = 0;
    HIP_TRY(c, hipMemcpyAsync(&above, d_counter, sizeof above, hipMemcpyDeviceToHost, sst));
    HIP_TRY(c, hipStreamSynchronize(sst));
    nsel = (uint32_t)(greater + need);
    if (int rc = cut_ties(kKeyPlusZero, kKeyMinusZero, nsel - above, (int64_t)above)) return rc;
  } else if ((int64_t)eq_count == need) {
    // every path that ties with the threshold is wanted: no cut needed
    HIP_TRY(c, launch_collect_gt(key, count, T - 1, c->d_sel.p, d_counter, (uint32_t)k, sst));
    nsel = (uint32_t)(greater + need);
  } else {
    // ties at the threshold exceed the remaining slots: keep the `need` smallest ordinals
    HIP_TRY(c, launch_collect_gt(key, count, T, c->d_sel.p, d_counter, (uint32_t)k, sst));
    if (int rc = cut_ties(T, T, (uint32_t)need, greater)) return rc;
    nsel = (uint32_t)(greater + need);
  }
  *n_selected = nsel;
  return GCRE_OK;
}

int select_chunk(gcre_ctx* c, const uint64_t* key, int64_t count, int k, uint32_t* n_selected, hipStream_t sst) {
  SelectState hs{};
  if (int rc = select_begin(c, key, count, k, &hs, sst)) return rc;
  HIP_TRY(c, hipStreamSynchronize(sst));
  return select_finish(c, key, count, k, hs, n_selected, sst);
}

void drop_ahead(gcre_ctx* c) {
  delete c->ahead;
  c->ahead = nullptr;
}

// a launch nobody came for (another window, other operands, the pass ended): wait for its kernels, forget it
void drop_launch(const gcre_uids* u) {
  if (u->launch.active && u->launch.done) (void)hipEventSynchronize(u->launch.done);
  if (u->launch.sel_pending) {   // the winners' copies of the selections it closed land in the chunk entries
    if (u->ctx && u->ctx->sel_stream) (void)hipStreamSynchronize(u->ctx->sel_stream);
    for (ChunkInsp& ci : u->insp) ci.win_pending = false;
    u->launch.sel_pending = false;
  }
  u->launch.active = false;
  u->launch.cands.clear();
  if (u->ctx) {
    for (auto& pr : u->launch.ev_null) { u->ctx->ev_pool.push_back(pr.first); u->ctx->ev_pool.push_back(pr.second); }
    for (auto& pr : u->launch.ev_stats) { u->ctx->ev_pool.push_back(pr.first); u->ctx->ev_pool.push_back(pr.second); }
  }
  u->launch.ev_null.clear();
  u->launch.ev_stats.clear();
  u->launch.prof = gcre_profile{};
}

}  // namespace

void gcre_host::free_uids(gcre_uids* u) {
  if (!u) return;
  if (u->ctx && u->ctx->ahead)   // a registered later join names this index
    for (const JoinPlan& a : *u->ctx->ahead)
      if (a.u == u) { drop_ahead(u->ctx); break; }
  drop_launch(u);
  u->launch.d_null.release();
  if (u->launch.done) (void)hipEventDestroy(u->launch.done);
  if (u->launch.sel_done) (void)hipEventDestroy(u->launch.sel_done);
  if (u->ctx && u->ctx->stream) (void)hipStreamSynchronize(u->ctx->stream);
  if (u->ctx && u->ctx->sel_stream) (void)hipStreamSynchronize(u->ctx->sel_stream);   // (an open selection's state lands in its chunk entry)
  if (u->ctx && u->ctx->insp_stream) (void)hipStreamSynchronize(u->ctx->insp_stream);
  if (u->ctx && u->ctx->rec_stream) (void)hipStreamSynchronize(u->ctx->rec_stream);   // (the gather reads the segment tables)
  if (u->ctx) {
    auto& v = u->ctx->live_uids;
    v.erase(std::remove(v.begin(), v.end(), u), v.end());
  }
  for (void* p : {(void*)u->d_path_idx, (void*)u->d_location, (void*)u->d_signs, (void*)u->d_red_index,
                  (void*)u->d_range_of, (void*)u->d_pieces, (void*)u->d_cut})
    if (p) (void)hipFree(p);
  for (auto& sc : u->seg_cache) {
    if (sc.d_segs) (void)hipFree(sc.d_segs);
    if (sc.d_quads) (void)hipFree(sc.d_quads);
  }
  for (auto& ci : u->insp) ci.release();
  if (u->prefetch && u->prefetch->th.joinable()) u->prefetch->th.join();
  delete u;
}

// validation that does not need the path sets (join_base.cpp:198-200 checks the rest in run_join)
gcre_uids* gcre_host::make_uids(gcre_ctx* c, int path_length, const int32_t* uid_count, const int64_t* uid_location,
                                int64_t n_uids, const int32_t* signs, int64_t n_signs) {
  HostTimer ht("make_uids");
  auto* u = new gcre_uids{};
  u->ctx = c;
  u->path_length = path_length;
  u->n_uids = n_uids;
  u->n_signs = n_signs;
  u->max_loc = -1;
  u->max_idx = -1;
  std::vector<int64_t>& path_idx = u->h_path_idx;
  path_idx.assign((size_t)n_uids + 1, 0);
  for (int64_t i = 0; i < n_uids; i++) {
    const int cnt = uid_count[i];
    if (cnt > 0) {
      const int64_t loc = uid_location[i];
      if (loc < 0) {
        fail(c, GCRE_ERR_RANGE, "assertion: uid location out of range");
        delete u;
        return nullptr;
      }
      u->max_loc = std::max(u->max_loc, loc + cnt - 1);
      u->max_idx = i;
    }
    path_idx[(size_t)i + 1] = path_idx[(size_t)i] + std::max(cnt, 0);   // uid_ref.path_idx, wrapper.cpp:128-130
  }
  u->total = path_idx[(size_t)n_uids];
  u->h_location.assign(uid_location, uid_location + n_uids);
  hipError_t e = hipMalloc((void**)&u->d_path_idx, path_idx.size() * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&u->d_location, (size_t)std::max<int64_t>(n_uids, 1) * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&u->d_signs, (size_t)std::max<int64_t>(n_signs, 1) * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(u->d_path_idx, path_idx.data(), path_idx.size() * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && n_uids > 0)
    e = hipMemcpyAsync(u->d_location, uid_location, (size_t)n_uids * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && n_signs > 0)
    e = hipMemcpyAsync(u->d_signs, signs, (size_t)n_signs * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // path_idx is a local
  if (e != hipSuccess) {
    fail(c, GCRE_ERR_DEVICE, std::string("uids upload: ") + hipGetErrorString(e));
    free_uids(u);
    return nullptr;
  }
  c->live_uids.push_back(u);
  return u;
}

namespace {

// distinct (location, count) ranges of a join index, uid -> range (see k_range_union)
int ensure_ranges(gcre_ctx* c, const gcre_uids& u) {
  if (u.n_ranges >= 0) return GCRE_OK;
  HostTimer ht("ensure_ranges");
  const auto& pi = u.h_path_idx;
  std::vector<int32_t> range_of((size_t)std::max<int64_t>(u.n_uids, 1), 0);
  std::vector<int64_t> loc;
  std::vector<int32_t> cnt;
  // uids with the same pivot gene share (location, count): one slot per location remembers the first range seen
  // there (direct-address table; a hash map when the locations are too spread out for one); a second count at the same
  // location simply gets ranges of its own (sharing is an optimisation, correctness does not depend on it)
  const bool direct = u.max_loc + 1 <= 8 * u.n_uids + ((int64_t)1 << 22);
  std::vector<int32_t> by_loc(direct ? (size_t)std::max<int64_t>(u.max_loc + 1, 1) : 1, -1);
  std::unordered_map<int64_t, int32_t> by_loc_map;
  for (int64_t i = 0; i < u.n_uids; i++) {
    const int64_t n = pi[(size_t)i + 1] - pi[(size_t)i];
    if (n <= 0) continue;   // never joined: its range is never looked at
    const int64_t l = u.h_location[(size_t)i];
    int32_t r = -1;
    if (direct) {
      r = by_loc[(size_t)l];
    } else {
      auto it = by_loc_map.find(l);
      if (it != by_loc_map.end()) r = it->second;
    }
    if (r < 0 || cnt[(size_t)r] != (int32_t)n) {
      const int32_t fresh = (int32_t)loc.size();
      loc.push_back(l);
      cnt.push_back((int32_t)n);
      if (r < 0) {
        if (direct) by_loc[(size_t)l] = fresh;
        else by_loc_map.emplace(l, fresh);
      }
      r = fresh;
    }
    range_of[(size_t)i] = r;
  }
  const size_t R = loc.size();
  std::vector<RangePiece> pieces;
  std::vector<int32_t> cut;
  const int64_t T = build_range_pieces(loc, cnt, pieces, cut);
  if (g_launch_trace) {
    std::vector<int32_t> by_len(cnt);
    std::sort(by_len.begin(), by_len.end());
    auto q = [&](double f) { return R ? by_len[std::min(R - 1, (size_t)(f * (double)R))] : 0; };
    fprintf(stderr, "ranges n_uids=%lld paths=%lld n_ranges=%zu n_pairs=%lld pieces=%zu cut=%zu rows/range median=%d p99=%d max=%d\n",
            (long long)u.n_uids, (long long)u.total, R, (long long)T, pieces.size(), cut.size(), q(0.5), q(0.99), q(1.0));
  }
  HIP_TRY(c, hipMalloc((void**)&u.d_range_of, range_of.size() * 4));
  HIP_TRY(c, hipMalloc((void**)&u.d_pieces, std::max<size_t>(pieces.size(), 1) * sizeof(RangePiece)));
  HIP_TRY(c, hipMalloc((void**)&u.d_cut, std::max<size_t>(cut.size(), 1) * 4));
  HIP_TRY(c, hipMemcpyAsync(u.d_range_of, range_of.data(), range_of.size() * 4, hipMemcpyHostToDevice, c->stream));
  if (!pieces.empty())
    HIP_TRY(c, hipMemcpyAsync(u.d_pieces, pieces.data(), pieces.size() * sizeof(RangePiece), hipMemcpyHostToDevice, c->stream));
  if (!cut.empty()) HIP_TRY(c, hipMemcpyAsync(u.d_cut, cut.data(), cut.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // the vectors are locals
  u.n_pairs = T;
  u.n_pieces = (int64_t)pieces.size();
  u.n_cut = (int64_t)cut.size();
  u.n_ranges = (int64_t)R;
  return GCRE_OK;
}

// inspect_only (gcre_join_ahead): the mask-independent half of the join -- expansion, inspector, kept rows, recipe, flags, top-k
// winners -- on the inspection stream, into the join index's inspection cache; nothing of the permutation kernel's (no maxima,
// no count planes, no results).  The join proper then replays it and starts at its null kernel.
// kLaunch (the chain of gcre_join_ahead): the join's permutation kernels are launched -- on the main stream, into the join
// index's own maxima, from the inspection that ran ahead -- and nothing is waited for; the call that comes for the join finds
// it launched and only finishes it (wait, copy the maxima, merge the cached winners).
// kCount (gcre_exceed or gcre_hits armed on a join that was launched ahead): once the join's result is delivered, its chunks
// are replayed from the inspection cache as far as each chunk's IeArgs, and the exceedance kernels are launched where the
// null kernels were (and k_hits_collect behind them); no inspector, no null kernel, no selection, no result.
enum JoinMode { kFull = 0, kInspect = 1, kLaunch = 2, kCount = 3 };

using EvList = std::vector<std::pair<hipEvent_t, hipEvent_t>>;

int run_join(gcre_ctx* c, const JoinPlan& jp, gcre_result* out, JoinMode mode = kFull);

// The chain of gcre_join_ahead: once a join's own work is queued, every registered later join is inspected (on the
// inspection stream) and launched (on the main stream) in turn -- the big inspector of the last level then runs beside the
// small permutation kernels of the levels before it instead of after them
int run_chain(gcre_ctx* c, const std::vector<JoinPlan>& chain) {
  for (const JoinPlan& a : chain) {
    if (int rc = run_join(c, a, nullptr, kInspect)) return rc;
    if (int rc = run_join(c, a, nullptr, kLaunch)) return rc;
    // a join that was not launched (its inspection did not validate: a broken hint) has not written what the joins
    // behind it read: they run whole, in their own calls
    if (!a.u->launch.active) break;
  }
  return GCRE_OK;
}

// The end of every join that returns a result (run_join's own, and one launched ahead): the first K maxima of `d_null` go
// out (methods.h:101-102; format_result, join_base.cpp:144-146) on `cs`; the registered chain, if any, is queued behind
// those copies and only they are waited for; then the candidates are merged and the context's profile gets the times of the
// events the join booked
int deliver_join(gcre_ctx* c, const JoinPlan& jp, gcre_result* out, int K, const uint32_t* d_null, hipStream_t cs,
                 std::vector<Candidate>& cands, EvList& ev_null, EvList& ev_stats,
                 std::chrono::steady_clock::time_point t_begin, std::unique_ptr<std::vector<JoinPlan>> chain) {
  out->n_perm = K;
  out->null_max = (float*)std::calloc((size_t)std::max(K, 1), sizeof(float));
  if (K > 0) {
    HIP_TRY(c, hipMemcpyAsync(out->null_max, d_null, (size_t)K * 4, hipMemcpyDeviceToHost, cs));
    if (jp.d_null_out) HIP_TRY(c, hipMemcpyAsync(jp.d_null_out, d_null, (size_t)K * 4, hipMemcpyDeviceToDevice, cs));
  }
  if (chain) {
    HIP_TRY(c, hipEventRecord(c->ev_tail, cs));
    if (int rc = run_chain(c, *chain)) return rc;
    HIP_TRY(c, hipEventSynchronize(c->ev_tail));
  } else {
    HIP_TRY(c, hipStreamSynchronize(cs));
  }
  merge_candidates(cands, c->top_k, out);
  c->prof.null_kernel_ms = drain_events(c, ev_null);
  c->prof.stats_kernel_ms = drain_events(c, ev_stats);
  c->prof.scores = c->prof.paths * (int64_t)K;
  c->prof.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return GCRE_OK;
}

// ---- per-gene best-path tally (gcre_genes.hip): scored paths [s0, s1) of a chunk whose inspector output is in `b` ----
// Queued on `st` behind the inspector that wrote the keys; whatever rewrites `b` next is queued behind it in turn (the next
// chunk's inspector runs on the same stream; cached buffers are not rewritten during the pass).  Folding a chunk twice
// changes nothing: the table only moves under (key greater) or (key equal and ordinal smaller).
int check_tally(gcre_ctx* c, const gcre_gene_tally* t, const gcre_uids& u) {
  if (t->ctx != c) return fail(c, GCRE_ERR_ARG, "gene tally does not belong to this context");
  if (t->w0 > 0 && t->n_rows0 != u.n_uids)
    return fail(c, GCRE_ERR_ARG, "gene tally: genes0 has " + std::to_string(t->n_rows0) + " rows, the join index has " +
                                     std::to_string(u.n_uids) + " uid rows");
  if (t->w1 > 0 && t->n_rows1 <= u.max_loc)
    return fail(c, GCRE_ERR_ARG, "gene tally: genes1 has " + std::to_string(t->n_rows1) + " rows, the join reads paths1 row " +
                                     std::to_string(u.max_loc));
  return GCRE_OK;
}

int fold_genes(gcre_ctx* c, gcre_gene_tally* t, const ChunkBufs& b, int64_t cb, int64_t s0, int64_t s1, hipStream_t st) {
  if (s1 <= s0) return GCRE_OK;
  if (t->last && t->last != st) {   // (a join folds on one stream; the next join may use another)
    hipEvent_t e = get_event(c);
    HIP_TRY(c, hipEventRecord(e, t->last));
    HIP_TRY(c, hipStreamWaitEvent(st, e, 0));
    c->ev_pool.push_back(e);
  }
  if (t->folding) {
    HIP_TRY(c, hipMemsetAsync(t->d_ck, 0, (size_t)t->n_slots * 8, st));
    HIP_TRY(c, hipMemsetAsync(t->d_cidx, 0xff, (size_t)t->n_slots * 4, st));
  }
  t->folding = true;
  t->last = st;
  GeneFoldArgs a{};
  a.key = b.key.p + s0;
  a.row0 = b.row0.p + s0;
  a.row1 = b.row1.p + s0;
  a.cases = b.cases.p + s0;
  a.ctrls = b.ctrls.p + s0;
  a.count = s1 - s0;
  a.first = cb + s0;
  a.genes0 = t->d_genes0;
  a.genes1 = t->d_genes1;
  a.w0 = t->w0;
  a.w1 = t->w1;
  a.n_slots = t->n_slots;
  a.prior = t->folded ? 1 : 0;
  a.ck = t->d_ck;
  a.cidx = t->d_cidx;
  a.bkey = t->d_bkey;
  a.bord = t->d_bord;
  a.bsrc = t->d_bsrc;
  a.btrg = t->d_btrg;
  a.bcases = t->d_bcases;
  a.bctrls = t->d_bctrls;
  HIP_TRY(c, launch_gene_fold(a, c->cus, st));
  t->folding = false;
  t->folded = true;
  return GCRE_OK;
}

// ---- null exceedance counts (gcre_exceed.hip): scored paths [s0, s1) of a chunk whose inspector output is in `b` ----
// Queued on `st` where the tally is, for the same reason (the next inspector rewrites `b`).  `ie`: the IeArgs the chunk's own
// inclusion-exclusion launches were given (k_exceed_ie takes the same); without them the count is k_null's mapping on the
// chunk's row0 / row1 / tot, which every chunk has.  NOT idempotent: run_chunk counts a chunk once, when no stage sends it
// round again.
int xcd_waves(const gcre_ctx* c, int waves_per_cu);
int count_exceed(gcre_ctx* c, const JoinPlan& jp, const ChunkBufs& b, int64_t s0, int64_t s1, hipStream_t st,
                 const IeArgs* ie = nullptr, int ie_planes = 0, int64_t ie_segs = 0) {
  gcre_exceed* x = jp.exceed;
  if (s1 <= s0) return GCRE_OK;
  const Geometry& g = c->g;
  // GCRE_EXCEED_KERNEL=dense: every chunk through k_exceed_dense (two independent forms can then be compared); =ie, or
  // unset: k_exceed_ie wherever the chunk's own null kernel took the inclusion-exclusion form
  const char* form = std::getenv("GCRE_EXCEED_KERNEL");
  if (form && std::strcmp(form, "dense") == 0) ie = nullptr;
  const int lds_bins = x->m <= (ie ? kExceedLdsBinsIe : kExceedLdsBinsDense) ? x->m : 0;
  if (jp.exceed_observed) {
    ExceedObsArgs oa{};
    oa.key = b.key.p + s0;
    oa.tkey = x->d_tkey;
    oa.hist = x->d_ohist;
    oa.count = s1 - s0;
    oa.m = x->m;
    oa.lds_bins = lds_bins;
    HIP_TRY(c, launch_exceed_observed(oa, c->cus, st));
    x->paths += s1 - s0;
  }
  const int K = c->win_K;
  if (K <= 0) return GCRE_OK;
  ExceedPerm perm;
  if (x->d_pc) {
    // a cell is 32 bits wide and takes at most one hit per joined path: refuse before the launch what could wrap it
    const size_t t0 = (size_t)c->win_k0 / kPermTileMax, t1 = ((size_t)c->win_k0 + (size_t)K + kPermTileMax - 1) / kPermTileMax;
    if (c->win_k0 + K > x->pc_stride || t1 > x->pc_load.size())
      return fail(c, GCRE_ERR_ARG, "exceedance counts: the permutation window lies outside the per-permutation counts");
    for (size_t t = t0; t < t1; t++)
      if (x->pc_load[t] + (uint64_t)(s1 - s0) > 0xffffffffull)
        return fail(c, GCRE_ERR_RANGE, "exceedance counts: more than 2^32-1 joined paths counted into one permutation's 32-bit cells: "
                                       "read and reset the per-permutation counts first");
    for (size_t t = t0; t < t1; t++) x->pc_load[t] += (uint64_t)(s1 - s0);
    perm.pc = x->d_pc;
    perm.stride = x->pc_stride;
    perm.k0 = c->win_k0;
  }
  if (std::getenv("GCRE_EXCEED_TRACE"))   // (tests: which form counted the chunk)
    std::fprintf(stderr, "[exceed] %s form: %lld joined paths x %d permutations, %d thresholds\n", ie ? "ie" : "dense",
                 (long long)(s1 - s0), K, x->m);
  if (ie) {
    IeArgs xa = *ie;
    xa.seg_begin = 0;
    xa.seg_end = ie_segs;
    xa.planes_out = nullptr;
    xa.null_bits = nullptr;
    xa.stats = nullptr;
    xa.timing = nullptr;
    const int wpc = std::min(c->sparse_waves_per_cu, exceed_ie_max_waves_per_cu(g.method, ie_planes, lds_bins, perm.pc != nullptr));
    xa.waves_per_xcd = std::min(ie->waves_per_xcd, xcd_waves(c, wpc));
    HIP_TRY(c, launch_exceed_ie(xa, g.method, ie_planes, x->d_pat, x->d_hist, x->m, lds_bins, st, perm));
    return GCRE_OK;
  }
  const NullConfig cfg = null_config(g.method, K);
  ExceedArgs a{};
  a.p0 = (const uint32_t*)jp.p0->d_rows;
  a.p1 = (const uint32_t*)jp.p1->d_rows;
  a.masks = c->d_masks + c->win_k0;
  a.row0 = b.row0.p + s0;
  a.row1 = b.row1.p + s0;
  a.tot = b.tot.p + (size_t)s0 * g.method;
  a.t32 = c->d_t32;
  a.d64 = c->d_dmax;
  a.d64n = c->d_dmaxn ? c->d_dmaxn : c->d_dmax;
  a.pat = x->d_pat;
  a.hist = x->d_hist;
  a.npaths = s1 - s0;
  a.npt = (a.npaths + cfg.path_tile - 1) / cfg.path_tile;
  a.S32 = 2 * g.S;
  a.W32p = 2 * g.Wp;
  a.Kpad = g.Kpad;
  a.K = K;
  a.nkt = (K + cfg.perm_tile - 1) / cfg.perm_tile;
  const int64_t want = (int64_t)c->cus * c->null_blocks_per_cu;
  a.pgroups = (int)std::min<int64_t>(std::max<int64_t>(1, want / a.nkt), a.npt);
  a.m = x->m;
  a.lds_bins = lds_bins;
  a.pc = perm.pc;
  a.pc_stride = perm.stride;
  a.k0 = perm.k0;
  HIP_TRY(c, launch_exceed_dense(a, g.method, cfg, st));
  return GCRE_OK;
}

// ---- hit lists (gcre_hits.hip): scored paths [s0, s1) of a chunk whose inspector output is in `b` ----
// Queued on `st` where the tally and the observed counts are, for the same reason.  NOT idempotent either: run_chunk
// collects a chunk exactly where and when it counts one.
int collect_hits(gcre_ctx* c, gcre_hits* h, const ChunkBufs& b, int64_t cb, int64_t s0, int64_t s1, hipStream_t st) {
  if (s1 <= s0) return GCRE_OK;
  HitsArgs a{};
  a.key = b.key.p + s0;
  a.row0 = b.row0.p + s0;
  a.row1 = b.row1.p + s0;
  a.cases = b.cases.p + s0;
  a.ctrls = b.ctrls.p + s0;
  a.count = s1 - s0;
  a.first = cb + s0;
  a.tkey = h->tkey;
  a.cursor = h->d_cursor;
  a.cap = h->cap;
  a.ord = h->ord();
  a.hkey = h->key();
  a.src = h->field(0);
  a.trg = h->field(1);
  a.hcases = h->field(2);
  a.hctrls = h->field(3);
  HIP_TRY(c, launch_hits_collect(a, c->cus, st));
  c->hits_launches++;
  h->paths += s1 - s0;
  return GCRE_OK;
}

// the unpacked winners of a chunk whose first scored path is joined path `first`, as candidates of their join
void push_candidates(std::vector<Candidate>& cands, const Winners& win, int64_t first) {
  for (uint32_t i = 0; i < win.n; i++)
    cands.push_back(Candidate{key_to_score(win.key[i]), first + (int64_t)win.sel[i], (int32_t)win.r0[i], (int32_t)win.r1[i],
                              (int32_t)win.cases[i], (int32_t)win.ctrls[i]});
}

// once the copies queue_winners queued have arrived (the caller waited for their stream)
void unpack_winners(Winners& w) {
  if (w.pack.empty()) return;
  const size_t n = w.n;
  const uint32_t* h32 = (const uint32_t*)(w.pack.data() + n);
  w.key.assign(w.pack.data(), w.pack.data() + n);
  w.cases.assign(h32, h32 + n);
  w.ctrls.assign(h32 + n, h32 + 2 * n);
  w.r0.assign(h32 + 2 * n, h32 + 3 * n);
  w.r1.assign(h32 + 3 * n, h32 + 4 * n);
  w.pack.clear();
}

// The tail of a join whose kernels were launched ahead (run_join, kLaunch): wait for them, copy the maxima out of the join
// index's own array, merge the winners its inspection cached.
int finish_launched(gcre_ctx* c, const JoinPlan& jp, gcre_result* out) {
  const auto t_begin = std::chrono::steady_clock::now();
  gcre_uids::Launched& L = jp.u->launch;
  const int K = c->win_K;
  const int Kpad = ((K + kPermTileMax - 1) / kPermTileMax) * kPermTileMax;
  HIP_TRY(c, hipEventSynchronize(L.done));
  L.active = false;
  // (on the inspection stream, idle by now: the main stream holds the later levels' kernels, which this join's caller
  // need not wait for)
  uint32_t lookups = 0;
  if (K > 0) HIP_TRY(c, hipMemcpyAsync(&lookups, L.d_null.p + Kpad, 4, hipMemcpyDeviceToHost, c->insp_stream));
  std::vector<Candidate> cands = std::move(L.cands);
  L.cands.clear();
  if (L.sel_pending) {
    // the selections the launch closed behind its null kernels: their winners' copies have been queued since, here they are
    // unpacked, become candidates and go to the inspection cache -- which then holds what an ahead inspection used to leave
    HIP_TRY(c, hipEventSynchronize(L.sel_done));
    for (ChunkInsp& ci : jp.u->insp) {
      if (!ci.win_pending) continue;
      ci.win_pending = false;
      unpack_winners(ci.win);
      push_candidates(cands, ci.win, ci.cb + ci.s0);
      ci.win_valid = true;
    }
    L.sel_pending = false;
  }
  c->prof = L.prof;
  L.prof = gcre_profile{};
  if (jp.tally) {
    // every chunk of the join is in its inspection cache (the launch replayed it from there, or inspected it into it); an
    // entry an abandoned attempt left behind describes the same paths and folds harmlessly
    for (const ChunkInsp& ci : jp.u->insp)
      if (ci.cb >= 0 && ci.inspected)
        if (int rc = fold_genes(c, jp.tally, ci.bufs, ci.cb, ci.s0, ci.s1, c->insp_stream)) return rc;
  }
  if (int rc = deliver_join(c, jp, out, K, L.d_null.p, c->insp_stream, cands, L.ev_null, L.ev_stats, t_begin, nullptr))
    return rc;
  c->prof.ie_lookup_tiles += lookups;
  // counts are sums, and a hit list appends: every chunk once, through the chunk loop itself (its cuts are the launch's)
  if (jp.exceed || jp.hits)
    if (int rc = run_join(c, jp, nullptr, kCount)) return rc;
  return GCRE_OK;
}

// A stretch of joined paths [b, e) of which [sb, se) is scored (the rest is only materialised: kept rows)
struct Seg { int64_t b, e, sb, se; };

// One call of run_join.  Written by begin_join unless a comment says otherwise; "(join)" marks what the chunks accumulate.
// Nothing here outlives the call.
struct JoinRun {
  gcre_ctx* const c;
  const JoinPlan& jp;
  gcre_result* const out;
  const JoinMode mode;
  const gcre_uids* u = nullptr;
  // the permutation window (all permutations unless gcre_set_perm_window narrowed it): K, the slice of the transposed
  // masks, of the masks (row stride Kstride: the full Kpad) and of the maxima
  Geometry g{};
  int Kstride = 0;
  int nkt_sp = 0;                      // 2048-permutation tiles of the window
  NullConfig cfg{};
  uint32_t* w_null = nullptr;          // the maxima the join writes (kLaunch: the join index's own)
  const uint32_t* w_masks = nullptr;
  const uint32_t* w_mt = nullptr;
  hipStream_t st = nullptr;            // the main stream; kInspect: the inspection stream
  uint32_t* flagblk = nullptr;         // the inspectors' flag block (FlagWord); kInspect: d_max_tot_b
  DevBuf<uint64_t>* exbuf = nullptr;   // excess rows of a hinted join; kInspect: d_excess_b (the join in flight owns d_excess)
  // the profile sink: the context's, or (kInspect, kLaunch) that of the join the ahead work is for (u->launch) -- not the
  // join it runs beside
  gcre_profile* prof = nullptr;
  EvList* ev_null = nullptr;
  EvList* ev_stats = nullptr;
  std::chrono::steady_clock::time_point t_begin;
  // kFull: the registered next joins (gcre_join_ahead) belong to THIS call: run by finish_join once this join's own kernels
  // are in flight, dropped with the JoinRun on every other road out
  std::unique_ptr<std::vector<JoinPlan>> ahead_plan;
  int64_t P = 0;                       // joined paths
  bool keep = false;                   // keep_paths = paths_res.size != 0, join_base.cpp:217
  bool replay = false;                 // the inspection cache holds this very join
  InspKey ikey;
  int64_t sb = 0, se = 0;              // the shard, clamped to [0, P)
  // plan_segments
  std::vector<Seg> segs;
  int64_t pl_b = 0, pl_e = 0;          // rows of res that get count planes
  int64_t r_lo = 0, r_hi = 0;          // rows of paths0 this call reads
  int64_t tile = 0, chunk_cap = 0;     // path tile of the dense kernel; joined paths per chunk
  size_t cap = 0;                      // elements of a chunk's buffers
  // prepare_operands; a chunk that finds the hint broken changes hinted, red, have_pz, want_ie and the res_planes pair
  bool sparse_ok = false, want_ie = false, hinted = false;
  bool range_union_due = false;        // hinted: the range check of the hint has not been queued yet (range_union_now)
  const gcre_pathset* red = nullptr;   // the rows the join adds: the reduced operand, or paths1
  bool have_p0 = false, have_pz = false, use_rec = false;
  const gcre_pathset *rec_a = nullptr, *rec_z = nullptr;   // use_rec: the operands of paths0's recipe
  gcre_recipe* rcp = nullptr;          // the recipe this join leaves with the rows it keeps (method 1)
  bool res_planes = false;             // the kept rows' count planes are written ...
  bool res_planes_ok = false;          // ... and no chunk was priced out of writing them
  bool split = false;                  // chunks are cut at the shard's ends (every form but the inclusion-exclusion one; (join))
  // (join)
  uint32_t over_next = 0;              // entries of the recipe's overflow area handed out so far (kFlagOverReserved)
  bool recipe_started = false, recipe_broken = false, hint_broke_late = false;
  uint32_t join_max_tot = 0, join_max_len = 0;
  bool ie_ran = false, ie_stat_pending = false;
  int exchanges_done = 0;
  std::vector<Candidate> cands;
  double select_ms = 0, select_wait_ms = 0;
  bool sel_abandoned = false;          // begin_join: the join forgot a chunk entry whose selection was still open
  JoinRun(gcre_ctx* c_, const JoinPlan& jp_, gcre_result* out_, JoinMode m) : c(c_), jp(jp_), out(out_), mode(m) {}
};

// One chunk [cb, cb + n) of a join: written by open_chunk, then by the stages in turn.  What outlives it goes to its
// inspection-cache entry or to the JoinRun.
struct ChunkRun {
  const Seg* sg = nullptr;
  int64_t cb = 0, n = 0;
  int64_t s0 = 0, s1 = 0;              // scored paths of the chunk: [s0, s1)
  bool scored = false, partial = false;
  int64_t npt = 0, padded = 0;         // path tiles of the dense kernel; rows up to `padded` are valid
  ChunkInsp* ci = nullptr;             // the chunk's inspection-cache entry (cache on)
  ChunkBufs* b = nullptr;              // its buffers: ci's, or the context's scratch
  bool hit = false;                    // replayed: the inspector's output is in place
  bool use_ie = false, use_sparse = false;
  // inspect_chunk (use_ie): where the inspector's lists go -- the kept set's recipe (absolute row = cb + i), or b
  uint32_t *rowz = nullptr, *linfo = nullptr, *lover = nullptr, *slot = nullptr, *over = nullptr;
  size_t over_cap = 0;
  bool sel_begun = false, sel_done = false;
  bool sel_left_open = false;          // kInspect: the digit passes are queued, whoever replays the chunk closes the selection
  hipStream_t sel_on = nullptr;        // the stream the selection runs on
  SelectState* hs = nullptr;           // where the digit passes' state lands: the chunk entry's pinned copy, or the context's
  Winners win;
  bool win_from_cache = false;
  uint32_t flags[kFlagWords] = {};     // score_chunk_ie: the inspector's flag block
  // score_chunk_ie, once the chunk's launches are decided: what they were given (the exceedance count takes the same)
  bool ie_ok = false;
  IeArgs ie{};
  int ie_planes = 0;
  int64_t ie_segs = 0;                 // scored segments: the first ones of ie.segs
};

// How a chunk's stages ended: the chunk loop of run_join runs it again after the last four
enum class ChunkEnd {
  kOpen,          // nothing decided yet: the null kernel is still to come
  kScored,        // its null kernel is queued: its winners are next
  kInspected,     // kInspect: inspected, its winners are next
  kNotNeeded,     // nothing of it is scored (rows of another shard: kept rows, recipe entries)
  kPricedOut,     // the inclusion-exclusion form costs more than the dense kernel: a whole chunk goes to the latter
  kResplit,       // a partial chunk off the inclusion-exclusion form: chunks are cut at the shard's ends from here on
  kRedoOverflow,  // more long lists than the area held: grown
  kRedoHint,      // the reduced operand does not describe the join: again on paths1 itself
};

// room for a chunk.  A replayed chunk's buffers hold what its inspector wrote: they may only grow with their contents (the
// path tile, and with it `cap` and the padding, depends on the window's permutation count)
template <typename T>
hipError_t hold(const ChunkRun& C, DevBuf<T>& buf, size_t want, hipStream_t st) {
  return C.hit ? buf.grow_keep(want, buf.cap, st) : buf.reserve(want);
}

// counter planes a null kernel keeps for counts up to `max_tot` carriers
int counter_planes(uint32_t max_tot) {
  int planes = 5;
  while (planes < 16 && (max_tot >> planes) != 0) planes++;
  return planes;
}

// persistent waves per XCD of a launch at `waves_per_cu` resident waves per CU
int xcd_waves(const gcre_ctx* c, int waves_per_cu) { return std::max(4, (c->cus * waves_per_cu / 8 / 4) * 4); }

// halve a launch's waves per XCD (not below 4) until every one of the 8 x waves has `per_wave` of the `items`
int spread_waves(int waves, int64_t items, int64_t per_wave) {
  while (waves > 4 && items < (int64_t)8 * waves * per_wave) waves = std::max(4, (waves / 2 / 4) * 4);
  return waves;
}

// Auto kernel choice (GCRE_NULL_KERNEL unset, DESIGN.md "Kernel choice"): dense = 2 VALU ops per dword per permutation at
// ~65 lane-ops/clk/CU.  The expressions are compared at a threshold: keep their order.
double dense_cost(const Geometry& g) { return 2.0 * g.Wp * g.method * (double)g.K * 2.0 / 65.0; }

// inclusion-exclusion: one mask-row load per list entry per 2048-permutation tile at ~15 CU-cycles each; paths0 lists without
// planes are bounded by its longest row, once per segment
bool ie_dearer(const Geometry& g, int nkt_sp, bool have_p0, uint32_t p0_max, int64_t nseg_est, int64_t n, uint64_t n_list) {
  const double base = have_p0 ? 0.0 : (double)p0_max * g.method * (double)nseg_est / (double)n;
  const double entries = (double)n_list / (double)n + base + 10.0 * g.method;
  const double ie_cost = entries * nkt_sp * 15.0;
  return ie_cost >= dense_cost(g);
}

// delta streaming: the same per entry; base lists are bounded by the largest carrier total, once per segment
bool sparse_dearer(const Geometry& g, uint64_t n_delta, uint32_t max_tot, int64_t nseg_est, int64_t n) {
  const double entries = (double)n_delta / (double)n + (double)max_tot * g.method * (double)nseg_est / (double)n;
  const double sparse_cost = entries * ((g.K + kSparseTile - 1) / kSparseTile) * 15.0;
  return sparse_cost >= dense_cost(g);
}

// uids (rows of paths0) with at least one joined path inside [first, first+count)
int64_t uids_in(const gcre_uids& u, int64_t first, int64_t count) {
  const auto& pi = u.h_path_idx;
  int64_t lo = std::upper_bound(pi.begin(), pi.end(), first) - pi.begin() - 1;
  int64_t hi = std::lower_bound(pi.begin(), pi.end(), first + count) - pi.begin();   // first uid starting at/after the end
  if (u.h_nonempty.empty()) {   // prefix count of the uids that join anything: once per join index
    u.h_nonempty.assign((size_t)u.n_uids + 1, 0);
    for (int64_t i = 0; i < u.n_uids; i++)
      u.h_nonempty[(size_t)i + 1] = u.h_nonempty[(size_t)i] + (pi[(size_t)i + 1] > pi[(size_t)i] ? 1 : 0);
  }
  lo = std::max<int64_t>(lo, 0);
  hi = std::min(hi, u.n_uids);
  return hi > lo ? u.h_nonempty[(size_t)hi] - u.h_nonempty[(size_t)lo] : (int64_t)0;
}

// compulsory HBM bytes of the permutation scoring of `count` joined paths: every paths0 row
// once per uid, every paths1 row once per joined path, the masks and the maxima once, the join index
double alg_bytes(const JoinRun& R, int64_t first, int64_t count) {
  const Geometry& g = R.g;
  const double up = (double)uids_in(*R.u, first, count);
  return 8.0 * g.W * g.method * (up + (double)count) + 8.0 * g.W * g.K + 4.0 * g.K + 24.0 * up;
}

// ---- thresholds shared across devices: the maxima so far go out, the merged ones come back (gcre_join_opts.exchange) ----
int exchange_now(JoinRun& R) {
  gcre_ctx* c = R.c;
  const JoinPlan& jp = R.jp;
  if (!jp.exchange || R.exchanges_done >= jp.exchanges) return GCRE_OK;
  R.exchanges_done++;
  if (R.g.K <= 0) return GCRE_OK;
  HIP_TRY(c, hipMemcpyAsync(jp.d_null_out, R.w_null, (size_t)R.g.K * 4, hipMemcpyDeviceToDevice, R.st));
  HIP_TRY(c, hipStreamSynchronize(R.st));
  if (jp.exchange(jp.exchange_user, jp.d_null_out, c->win_k0, c->win_k0 + R.g.K) != 0)
    return fail(c, GCRE_ERR_DEVICE, "the caller's threshold exchange failed");
  // merged maxima are >= this shard's: a plain copy back (non-negative floats order like their bit patterns)
  HIP_TRY(c, hipMemcpyAsync(R.w_null, jp.d_null_out, (size_t)R.g.K * 4, hipMemcpyDeviceToDevice, R.st));
  return GCRE_OK;
}

// the look-up counter the last pruned launch left in the flag block, once the block is about to be reused
void collect_ie_stat(JoinRun& R) {
  if (R.mode == kLaunch) R.ie_stat_pending = false;   // (its counter sits behind its maxima and is read when the join is finished)
  if (!R.ie_stat_pending) return;
  uint32_t v = 0;
  if (hipMemcpyAsync(&v, R.flagblk + kFlagLookupTiles, 4, hipMemcpyDeviceToHost, R.st) == hipSuccess &&
      hipStreamSynchronize(R.st) == hipSuccess)
    R.prof->ie_lookup_tiles += v;
  R.ie_stat_pending = false;
}

// the rows the join adds and their count planes
int prepare_z(JoinRun& R) {
  gcre_ctx* c = R.c;
  R.red = R.hinted ? R.u->red : R.jp.p1;
  // a kept set read as the added rows (level 5 adds rows of paths2) without planes of its own: they are rebuilt from
  // its bit lists now, and the join that writes its rows leaves them next time
  if (!planes_current(c, R.red) && R.red->rec) R.red->planes_wanted = true;
  if (int rc = ensure_lists(c, R.red)) return rc;
  if (int rc = ensure_planes(c, R.red)) return rc;
  R.have_pz = planes_current(c, R.red);
  return GCRE_OK;
}

// the winners of a chunk's selection (c->d_sel): their keys, counts and rows gathered from the chunk's buffers, copied out
int queue_winners(gcre_ctx* c, const ChunkBufs& b, int64_t s0, uint32_t nsel, Winners& w, hipStream_t qs) {
  w.n = nsel;
  if (nsel == 0) return GCRE_OK;
  // keys, then cases, ctrls and the two rows, in one buffer: one copy out instead of five (a copy into pageable memory
  // holds the host for 20-30 us, and this host is what the chain's next launch waits for); unpack_winners splits it
  HIP_TRY(c, c->d_wkey.reserve((size_t)nsel * 3));
  uint32_t* d32 = (uint32_t*)(c->d_wkey.p + nsel);
  HIP_TRY(c, launch_gather_winners(c->d_sel.p, nsel, b.key.p + s0, b.cases.p + s0, b.ctrls.p + s0, b.row0.p + s0,
                                   b.row1.p + s0, c->d_wkey.p, d32, d32 + nsel, d32 + (size_t)nsel * 2, d32 + (size_t)nsel * 3, qs));
  w.sel.resize(nsel);
  w.pack.resize((size_t)nsel * 3);
  HIP_TRY(c, hipMemcpyAsync(w.sel.data(), c->d_sel.p, nsel * 4, hipMemcpyDeviceToHost, qs));
  HIP_TRY(c, hipMemcpyAsync(w.pack.data(), c->d_wkey.p, (size_t)nsel * 24, hipMemcpyDeviceToHost, qs));
  return GCRE_OK;
}

// the second half of a selection begun on C.sel_on, whose state has arrived (the caller waited for it): collect the
// winners and queue their copies
int finish_selection(JoinRun& R, ChunkRun& C) {
  uint32_t nsel = 0;
  const int64_t count = C.s1 - C.s0;
  if (int rc = select_finish(R.c, C.b->key.p + C.s0, count, R.c->top_k, *C.hs, &nsel, C.sel_on)) return rc;
  if (int rc = queue_winners(R.c, *C.b, C.s0, nsel, C.win, C.sel_on)) return rc;
  C.sel_done = true;
  if (C.ci) C.ci->sel_open = false;
  return GCRE_OK;
}

enum class Begin { kRun, kDone, kFinishLaunched };

// The window, the checks of JoinExec::join, the inspection cache's verdict and what follows from it, the shard, the streams.
// *next: kDone when there is nothing for this call to do (kInspect: already inspected; kLaunch: not launched; no cache),
// kFinishLaunched when the join was launched ahead and only its results are left to collect.
int begin_join(JoinRun& R, Begin* next) {
  gcre_ctx* c = R.c;
  const JoinPlan& jp = R.jp;
  const JoinMode mode = R.mode;
  *next = Begin::kDone;
  Geometry& g = R.g;
  g = c->g;
  g.K = c->win_K;
  g.Kpad = ((g.K + kPermTileMax - 1) / kPermTileMax) * kPermTileMax;
  R.Kstride = c->g.Kpad;
  R.nkt_sp = (g.K + kSparseTile - 1) / kSparseTile;
  R.cfg = null_config(g.method, g.K);
  R.w_null = c->d_null ? c->d_null + c->win_k0 : nullptr;
  R.w_masks = c->d_masks ? c->d_masks + c->win_k0 : nullptr;
  R.w_mt = c->d_mt ? c->d_mt + (size_t)(c->win_k0 / kSparseTile) * (size_t)(64 * g.Wp + 1) * 64 : nullptr;
  R.t_begin = std::chrono::steady_clock::now();
  if (R.out) std::memset(R.out, 0, sizeof *R.out);
  if (mode == kFull) {
    R.ahead_plan.reset(c->ahead);
    c->ahead = nullptr;
    c->ahead_closed = false;
  }
  R.flagblk = mode == kInspect ? c->d_max_tot_b : c->d_max_tot;
  if (!c->have_table) return fail(c, GCRE_ERR_ASSERT, "value table not set");
  if (g.K > 0 && !c->have_perms) return fail(c, GCRE_ERR_ASSERT, "permuted cases not set");
  if (c->top_k < 1) return fail(c, GCRE_ERR_ARG, "top_k must be >= 1");
  if (!jp.u || jp.u->ctx != c || !jp.p0 || !jp.p1 || jp.p0->ctx != c || jp.p1->ctx != c || (jp.res && jp.res->ctx != c))
    return fail(c, GCRE_ERR_ARG, "uids / path set do not belong to this context");
  R.u = jp.u;
  const gcre_uids& u = *jp.u;

  // ---- the checks of JoinExec::join, join_base.cpp:196-200 ----
  if (u.n_uids != jp.p0->nrows) return fail(c, GCRE_ERR_ASSERT, "assertion: uids.size() != paths0.size");
  if (u.max_loc >= jp.p1->nrows) return fail(c, GCRE_ERR_RANGE, "assertion: uid location out of range");
  const int64_t P = R.P = u.total;
  const bool keep = R.keep = jp.res != nullptr && jp.res->nrows != 0;
  if (jp.res && jp.res->nrows != 0 && jp.res->nrows != P)
    return fail(c, GCRE_ERR_ASSERT, "assertion: paths_res.size != total paths");
  if (jp.tally && mode == kFull)
    if (int rc = check_tally(c, jp.tally, u)) return rc;
  if (jp.exceed && jp.exceed->ctx != c) return fail(c, GCRE_ERR_ARG, "exceedance counts do not belong to this context");
  if (jp.hits && jp.hits->ctx != c) return fail(c, GCRE_ERR_ARG, "hit list does not belong to this context");
  // ---- inspection cache: has this very join (same operand rows, kept set, shard, table) run on this index before? ----
  InspKey& ikey = R.ikey;
  if (c->insp_cache) {
    ikey.p0_id = jp.p0->id; ikey.p0_ver = jp.p0->version;
    ikey.p1_id = jp.p1->id; ikey.p1_ver = jp.p1->version;
    if (u.red) {
      auto it = c->live_sets.find(u.red_id);
      if (it != c->live_sets.end() && it->second == u.red) { ikey.red_id = u.red_id; ikey.red_ver = u.red->version; }
    }
    ikey.res_id = jp.res ? jp.res->id : 0;
    ikey.obs_epoch = c->obs_epoch;
    ikey.sb = jp.sharded ? jp.shard_begin : 0;
    ikey.se = jp.sharded ? jp.shard_end : -1;
    ikey.keep_mode = (keep ? 1 : 0) | (jp.keep_ranged ? 2 : 0) | (jp.planes_ranged ? 4 : 0);
    ikey.keep_begin = (jp.keep_ranged || jp.planes_ranged) ? jp.keep_begin : 0;
    ikey.keep_end = (jp.keep_ranged || jp.planes_ranged) ? jp.keep_end : 0;
    ikey.chunk_paths = c->chunk_paths;
    ikey.top_k = c->top_k;
    ikey.null_kernel = c->null_kernel;
    R.replay = u.insp_valid && u.insp_key == ikey && (!keep || jp.res->version == u.insp_res_ver);
    if (mode == kCount && !R.replay) return fail(c, GCRE_ERR_DEVICE, "internal: the counting pass of a join launched ahead found no inspection to replay");
    // not launched: the join's own call runs it whole
    if (mode == kLaunch && (!R.replay || jp.exchange || g.K <= 0)) return GCRE_OK;
    if (mode == kFull && u.launch.active) {
      // this join was launched ahead: if it is still the same join (operands, kept set, shard, table, window, masks) only its
      // results are left to collect; otherwise its kernels are waited for and forgotten
      const gcre_uids::Launched& L = u.launch;
      if (R.replay && L.key == ikey && L.win_k0 == c->win_k0 && L.win_K == c->win_K && L.mask_epoch == c->mask_epoch &&
          (!keep || jp.res->version == L.res_ver) && !jp.exchange) {
        *next = Begin::kFinishLaunched;
        return GCRE_OK;
      }
      drop_launch(&u);
    }
    if (mode == kInspect) drop_launch(&u);          // (a stale launch of an earlier pass)
    if (mode == kInspect && R.replay) return GCRE_OK;   // already inspected (a later permutation window, kept inspections)
    if (!R.replay) {
      for (auto& ci : u.insp) {   // the buffers stay and serve the new chunks in turn
        R.sel_abandoned = R.sel_abandoned || ci.sel_open;
        ci.forget();
        ci.cb = -1;
      }
      u.insp_key = ikey;
    }
    u.insp_valid = false;   // until this call completes
  } else if (mode == kCount) {
    return fail(c, GCRE_ERR_DEVICE, "internal: the counting pass of a join launched ahead needs the inspection cache");
  } else if (mode != kFull) {
    return GCRE_OK;   // no inspection cache, nothing to inspect or launch ahead
  } else if (u.insp_valid || !u.insp.empty()) {
    for (auto& ci : u.insp) ci.release();
    u.insp.clear();
    u.insp_valid = false;
  }
  if (keep && !R.replay) {   // its rows are about to be rewritten: lists go, the plane buffer stays allocated for the new rows
    jp.res->version++;
    uint32_t* planes = jp.res->d_planes;
    const int groups = jp.res->plane_groups;
    const size_t pbytes = jp.res->planes_bytes;
    jp.res->d_planes = nullptr;
    drop_lists(jp.res);
    jp.res->d_planes = planes;
    jp.res->plane_groups = groups;
    jp.res->planes_bytes = pbytes;
  }
  if (g.method == 2 && P > 0) {
    // need_flip reads signs[idx] and/or signs[loc] (gcre.h:71-81); the reference would read out of bounds
    int64_t need_signs = 0;
    if (u.path_length > 3) need_signs = u.max_idx + 1;
    else if (u.path_length < 3) need_signs = u.max_loc + 1;
    else need_signs = std::max(u.max_idx, u.max_loc) + 1;
    if (u.n_signs < need_signs) return fail(c, GCRE_ERR_RANGE, "signs vector shorter than the rows it is indexed by");
  }

  R.sb = jp.sharded ? jp.shard_begin : 0;
  R.se = jp.sharded ? jp.shard_end : P;
  R.sb = std::max<int64_t>(0, std::min(R.sb, P));
  R.se = std::max(R.sb, std::min(R.se, P));

  hipStream_t st = R.st = mode == kInspect ? c->insp_stream : c->stream;
  R.exbuf = mode == kInspect ? &c->d_excess_b : &c->d_excess;
  if (R.sel_abandoned) {   // digit passes nobody will come for may still read the keys this join's inspector rewrites
    HIP_TRY(c, hipEventRecord(c->ev_sel_done, c->sel_stream));
    HIP_TRY(c, hipStreamWaitEvent(st, c->ev_sel_done, 0));
  }
  const bool own_sink = mode == kFull;
  R.prof = own_sink ? &c->prof : &u.launch.prof;
  R.ev_null = own_sink ? &c->ev_null : &u.launch.ev_null;
  R.ev_stats = own_sink ? &c->ev_stats : &u.launch.ev_stats;
  if (mode == kInspect) {
    // behind the last inspector that ran on the main stream (its kept rows and recipe are this one's operands)
    HIP_TRY(c, hipStreamWaitEvent(st, c->ev_insp_main, 0));
  } else {
    // behind an inspection that ran ahead on its own stream (a no-op when there was none)
    HIP_TRY(c, hipStreamWaitEvent(st, c->ev_insp_done, 0));
    if (mode == kLaunch) {   // the launch's own maxima (+ its look-up counter): the context's belong to the join that is being finished
      HIP_TRY(c, u.launch.d_null.reserve((size_t)g.Kpad + 64));
      R.w_null = u.launch.d_null.p;
      if (!u.launch.done && hipEventCreateWithFlags(&u.launch.done, hipEventDisableTiming) != hipSuccess)
        return fail(c, GCRE_ERR_DEVICE, "hipEventCreate failed");
      if (!u.launch.sel_done && hipEventCreateWithFlags(&u.launch.sel_done, hipEventDisableTiming) != hipSuccess)
        return fail(c, GCRE_ERR_DEVICE, "hipEventCreate failed");
      HIP_TRY(c, hipMemsetAsync(R.w_null, 0, ((size_t)g.Kpad + 1) * 4, st));
    } else if (g.Kpad > 0 && mode != kCount) {   // (a counting pass writes no maxima)
      HIP_TRY(c, hipMemsetAsync(R.w_null, 0, (size_t)g.Kpad * 4, st));
    }
  }
  if (mode == kFull) c->prof = gcre_profile{};
  *next = Begin::kRun;
  return GCRE_OK;
}

// Segments: rows outside the shard are only materialised (when kept); the shard [sb, se) inside a segment is scored.
// Kept rows next to the shard share its launches (one inspector pass, one flag read-back, one kernel that scores the shard's
// path runs and only writes count planes / recipe entries for the others).  Then the chunk size and the rows of paths0 read.
void plan_segments(JoinRun& R) {
  const JoinPlan& jp = R.jp;
  const int64_t P = R.P, sb = R.sb, se = R.se;
  // kept rows outside the scored shard: all of them, or only [keep_begin, keep_end) (gcre_join_opts.keep_ranged)
  int64_t kb = 0, ke = P;
  if (jp.keep_ranged) {
    kb = std::max<int64_t>(0, std::min(jp.keep_begin, P));
    ke = std::max(kb, std::min(jp.keep_end, P));
  }
  // rows of `res` that get count planes: every produced row, or (gcre_join_opts.keep_ranged == 2) the hull of
  // [keep_begin, keep_end) and the shard
  R.pl_b = std::min(kb, se > sb ? sb : kb);
  R.pl_e = std::max(ke, se > sb ? se : ke);
  if (jp.planes_ranged) {
    const int64_t qb = std::max<int64_t>(0, std::min(jp.keep_begin, P)), qe = std::max(qb, std::min(jp.keep_end, P));
    R.pl_b = qe > qb ? qb : (se > sb ? sb : 0);
    R.pl_e = qe > qb ? qe : (se > sb ? se : 0);
    if (se > sb) {
      R.pl_b = std::min(R.pl_b, sb);
      R.pl_e = std::max(R.pl_e, se);
    }
  }
  std::vector<Seg>& segs = R.segs;
  if (!R.keep || kb >= ke) {
    if (se > sb) segs.push_back({sb, se, sb, se});
  } else if (se <= sb) {
    segs.push_back({kb, ke, kb, kb});
  } else if (kb <= se && sb <= ke) {   // overlapping or adjacent: one segment
    segs.push_back({std::min(kb, sb), std::max(ke, se), sb, se});
  } else if (ke < sb) {
    segs.push_back({kb, ke, kb, kb});
    segs.push_back({sb, se, sb, se});
  } else {
    segs.push_back({sb, se, sb, se});
    segs.push_back({kb, ke, kb, kb});
  }

  R.tile = R.cfg.path_tile;
  R.chunk_cap = std::max<int64_t>(R.tile, (R.c->chunk_paths / R.tile) * R.tile);
  R.cap = (size_t)std::min<int64_t>(R.chunk_cap, ((P + R.tile - 1) / R.tile) * R.tile) + (size_t)R.tile;
  // rows of paths0 this call reads: the uids of the joined paths it processes
  if (!segs.empty()) {
    int64_t first = P, last = 0;
    for (const Seg& sg : segs) {
      first = std::min(first, sg.b);
      last = std::max(last, sg.e);
    }
    const auto& pi = R.u->h_path_idx;
    R.r_lo = std::max<int64_t>(0, (int64_t)(std::upper_bound(pi.begin(), pi.end(), first) - pi.begin()) - 1);
    R.r_hi = std::min<int64_t>(R.u->n_uids, (int64_t)(std::lower_bound(pi.begin(), pi.end(), last) - pi.begin()));
  }
}

// ---- inclusion-exclusion form (gcre_ie.hip): operands and their count planes, once per join ----
int prepare_operands(JoinRun& R) {
  gcre_ctx* c = R.c;
  const JoinPlan& jp = R.jp;
  const gcre_uids& u = *R.u;
  const Geometry& g = R.g;
  const bool inspect_only = R.mode == kInspect;
  hipStream_t st = R.st;
  R.sparse_ok = sparse_enabled(c) && R.w_mt != nullptr;
  R.want_ie = R.sparse_ok && (c->null_kernel == 0 || c->null_kernel == 3);
  if (R.want_ie && u.red && u.d_red_index && u.n_red_index > u.max_loc) {
    auto it = c->live_sets.find(u.red_id);   // the caller may have freed the operand since
    R.hinted = it != c->live_sets.end() && it->second == u.red;
    if (R.replay && !u.insp_hinted) R.hinted = false;   // the cached run found the hint broken: it ended on paths1 itself
  }
  const auto tp0 = std::chrono::steady_clock::now();
  if (R.want_ie) {
    if (inspect_only) {
      // count planes are the permutation kernel's business: the join proper looks after them (and decides, from what it
      // then finds, where its rows' planes go); the inspector only needs to know which rows the join adds
      R.red = R.hinted ? u.red : jp.p1;
      R.have_pz = R.have_p0 = true;
    } else {
      if (int rc = prepare_z(R)) return rc;
      R.have_p0 = planes_cover(c, jp.p0, R.r_lo, R.r_hi);        // a kept join left them behind
      if (!R.have_p0 && recipe_operands(c, jp.p0, &R.rec_a, &R.rec_z)) {
        // ... or it left the recipe: the kernel rebuilds a row's planes from the planes of the recipe's operands
        // (of which a multi-device run may hold a range only: the rows the recipe of [r_lo, r_hi) names -- the
        // producing join's paths0 rows, ascending)
        int64_t a_lo = 0, a_hi = R.rec_a->nrows;
        if (!planes_current(c, R.rec_a) && R.r_hi > R.r_lo && (size_t)R.r_hi <= jp.p0->rec->row0.cap) {
          uint32_t ends[2] = {0, 0};
          HIP_TRY(c, hipMemcpyAsync(&ends[0], jp.p0->rec->row0.p + R.r_lo, 4, hipMemcpyDeviceToHost, st));
          HIP_TRY(c, hipMemcpyAsync(&ends[1], jp.p0->rec->row0.p + (R.r_hi - 1), 4, hipMemcpyDeviceToHost, st));
          HIP_TRY(c, hipStreamSynchronize(st));
          a_lo = ends[0];
          a_hi = (int64_t)ends[1] + 1;
        }
        if (!planes_cover(c, R.rec_a, a_lo, a_hi)) {
          R.rec_a->planes_wanted = true;
          if (int rc = ensure_planes(c, R.rec_a)) return rc;
        }
        if (int rc = ensure_planes(c, R.rec_z)) return rc;
        R.use_rec = planes_cover(c, R.rec_a, a_lo, a_hi) && planes_current(c, R.rec_z);
        R.have_p0 = R.use_rec;
      }
      if (!R.have_p0) {
        if (int rc = ensure_planes(c, jp.p0)) return rc;   // from its bit lists (all rows)
        R.have_p0 = planes_current(c, jp.p0);
      }
      if (!R.have_p0 || !R.have_pz) R.want_ie = false;   // the planes do not fit in device memory: delta streaming (gcre_sparse.hip)
    }
    if (R.want_ie && R.hinted) {
      // the hint is checked without reading paths1 per joined path: once per distinct uid range here (the reduced
      // row lies inside paths1[loc]; what paths1[loc] has beyond it is collected per range), and per joined path in
      // k_stats_ie (that excess lies inside paths0[idx])
      if (int rc = ensure_ranges(c, u)) return rc;
      HIP_TRY(c, R.exbuf->reserve((size_t)std::max<int64_t>(u.n_ranges, 1) * g.S));
      // the check itself (k_range_union) feeds the inspector alone: it is queued in front of the first inspector this join
      // launches (range_union_now) -- a join that replays every chunk from the inspection cache launches none, and its
      // chunks carry the verdict in their cached flags
      R.range_union_due = true;
    }
    if (R.want_ie && R.keep) {
      // carriers of a joined row <= carriers(paths0 row) + carriers(added row); <= padded patient count
      const uint32_t bound = std::min<uint32_t>((uint32_t)(64 * g.Wp), row_max(c, jp.p0) + row_max(c, R.red));
      const int out_groups = plane_groups_for(bound);
      bool want_out = true;
      // the kept rows leave with the recipe of this join (its inspector output: 60 B per row, 104 B for the signed
      // method's two lists).  Their planes are only written when they are small, or when the next join could not use the
      // recipe (it needs stored planes of paths0)
      if (!jp.res->rec) jp.res->rec = new gcre_recipe();
      gcre_recipe* rcp = R.rcp = jp.res->rec;
      if (!R.replay) rcp->valid = false;
      const size_t rows = (size_t)R.P, lists = rows * (size_t)g.method;
      hipError_t e = rcp->row0.reserve(rows + 64);
      if (e == hipSuccess) e = rcp->rowz.reserve(rows + 64);
      if (e == hipSuccess) e = rcp->linfo.reserve(lists + 64);
      if (e == hipSuccess) e = rcp->lover.reserve(lists + 64);
      if (e == hipSuccess) e = rcp->tot.reserve(lists + 64);
      if (e == hipSuccess) e = rcp->slot.reserve(lists * 8 + 64);
      if (e == hipSuccess) e = rcp->over.reserve(std::max<size_t>(rcp->over.cap, lists * 2 + ((size_t)1 << 26)));
      if (e != hipSuccess) {
        (void)hipGetLastError();
        rcp->release();
        R.rcp = nullptr;
      } else {
        // (sized for the nominal window: the same answer in every window of a run)
        const size_t nkt_nom = (size_t)((std::max(c->win_K, c->win_K_nominal) + kSparseTile - 1) / kSparseTile);
        const size_t nominal = (size_t)std::max<int64_t>(jp.res->nrows, 1) * g.method * nkt_nom * (size_t)out_groups * 1024;
        want_out = nominal <= c->planes_out_max || R.use_rec || jp.res->planes_wanted;
      }
      if (inspect_only || R.mode == kCount) {
        // (the join proper allocates -- or drops -- the kept rows' planes; a counting pass leaves them as they are)
      } else if (want_out) {
        R.res_planes = alloc_planes(c, jp.res, out_groups);
        R.res_planes_ok = R.res_planes;
      } else {
        drop_planes(jp.res);   // nothing stale stays behind
      }
    }
  }
  R.prof->prepare_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count();
  // only the inclusion-exclusion kernels score part of a chunk; every other form gets chunks cut at the shard's ends
  R.split = !(R.want_ie && g.K > 0);
  return GCRE_OK;
}

// The range check of a hinted join, once, in front of the first inspector the join launches: what paths1[loc] has beyond the
// reduced row, per distinct uid range (the inspector's `excess`).  Its verdict lands in words kFlagRangeUnion.. of the flag
// block, which the chunks leave alone: it is read with that chunk's flags (no round trip of its own); a reduced row that is
// not even part of the row it stands for sends that chunk, and the join, back to paths1 itself like any other broken hint
int range_union_now(JoinRun& R) {
  gcre_ctx* c = R.c;
  const gcre_uids& u = *R.u;
  const Geometry& g = R.g;
  R.range_union_due = false;
  HIP_TRY(c, hipMemsetAsync(R.flagblk + kFlagRangeUnion, 0, (kFlagWords - kFlagRangeUnion) * 4, R.st));
  HIP_TRY(c, launch_range_union(R.jp.p1->d_rows, R.red->d_rows, u.d_red_index, u.d_pieces, u.n_pieces, u.d_cut, u.n_cut, g.S,
                                g.Wp, g.method, R.exbuf->p, R.flagblk + kFlagRangeUnion, R.st));
  return GCRE_OK;
}

// an open selection nobody will close (the entry is about to describe other paths): its digit passes may still be reading
// the keys that the join's stream is about to rewrite
int abandon_selection(JoinRun& R, ChunkInsp& ci) {
  if (!ci.sel_open) return GCRE_OK;
  ci.sel_open = false;
  HIP_TRY(R.c, hipEventRecord(R.c->ev_sel_done, R.c->sel_stream));
  HIP_TRY(R.c, hipStreamWaitEvent(R.st, R.c->ev_sel_done, 0));
  return GCRE_OK;
}

// The chunk [cb, ce) of segment sg: what it scores, its inspection-cache entry, its buffers and their padding
int open_chunk(JoinRun& R, ChunkRun& C, const Seg& sg, int64_t cb, int64_t ce) {
  gcre_ctx* c = R.c;
  const gcre_uids& u = *R.u;
  const int64_t n = ce - cb;
  C.sg = &sg;
  C.cb = cb;
  C.n = n;
  C.s0 = std::min(std::max<int64_t>(sg.sb - cb, 0), n);
  C.s1 = std::max(C.s0, std::min(std::max<int64_t>(sg.se - cb, 0), n));
  C.scored = C.s1 > C.s0;
  C.partial = C.scored && (C.s0 > 0 || C.s1 < n);
  C.sel_on = R.st;
  C.npt = (n + R.tile - 1) / R.tile;
  C.padded = C.npt * R.tile;
  if (c->insp_cache) {
    ChunkInsp*& ci = C.ci;
    for (auto& e : u.insp)
      if (e.cb == cb && e.n == n) ci = &e;
    if (!ci) {
      for (auto& e : u.insp)   // an entry of an earlier join on this index: its buffers serve this chunk
        if (e.cb < 0) { ci = &e; break; }
      if (!ci) { u.insp.emplace_back(); ci = &u.insp.back(); }
      ci->forget();
      ci->cb = cb;
      ci->n = n;
    }
    if (ci->s0 != C.s0 || ci->s1 != C.s1) {
      ci->win_valid = false;
      if (int rc = abandon_selection(R, *ci)) return rc;
    }
    ci->s0 = C.s0;
    ci->s1 = C.s1;
  }
  ChunkInsp* ci = C.ci;
  ChunkBufs& b = *(C.b = ci ? &ci->bufs : &c->scratch);
  C.use_ie = R.want_ie && (C.scored || R.res_planes || R.rcp != nullptr);
  C.use_sparse = C.scored && R.sparse_ok && !R.want_ie;
  // replayed: the inspector's output is in place (rows, statistics, keys, kept rows, lists when this chunk wants them)
  C.hit = ci && R.replay && ci->inspected &&
          (!C.use_ie || (ci->with_lists && ci->flags_valid && ci->in_recipe == (R.rcp != nullptr)));
  if (ci && !C.hit) {
    if (int rc = abandon_selection(R, *ci)) return rc;
    ci->forget();
  }
  if (C.hit) R.prof->inspect_replays++;
  const size_t cap = R.cap;
  hipStream_t st = R.st;
  HIP_TRY(c, hold(C, b.row0, cap, st));
  HIP_TRY(c, hold(C, b.row1, cap, st));
  HIP_TRY(c, hold(C, b.tot, cap * R.g.method, st));
  HIP_TRY(c, hold(C, b.cases, cap, st));
  HIP_TRY(c, hold(C, b.ctrls, cap, st));
  HIP_TRY(c, hold(C, b.key, cap, st));
  // the null kernel reads whole tiles: rows / totals beyond n must be valid (row 0, zero carriers)
  const int64_t padded = C.padded;
  const bool pad_now = padded > n && (!C.hit || padded > ci->padded);
  if (ci) ci->padded = std::max(C.hit ? ci->padded : (int64_t)0, padded);
  if (pad_now) {
    HIP_TRY(c, hipMemsetAsync(b.row0.p + n, 0, (size_t)(padded - n) * 4, st));
    HIP_TRY(c, hipMemsetAsync(b.row1.p + n, 0, (size_t)(padded - n) * 4, st));
    HIP_TRY(c, hipMemsetAsync(b.tot.p + (size_t)n * R.g.method, 0, (size_t)(padded - n) * 4 * R.g.method, st));
  }
  return GCRE_OK;
}

// Expansion and the inspector -- k_stats, or k_stats_ie with the lists -- unless the chunk is replayed; the start of its
// top-k selection.  *end: kOpen, kResplit or kNotNeeded.
int inspect_chunk(JoinRun& R, ChunkRun& C, ChunkEnd* end) {
  gcre_ctx* c = R.c;
  const JoinPlan& jp = R.jp;
  const gcre_uids& u = *R.u;
  const Geometry& g = R.g;
  ChunkBufs& b = *C.b;
  ChunkInsp* ci = C.ci;
  const int64_t cb = C.cb, n = C.n;
  hipStream_t st = R.st;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!C.hit) {
    e0 = get_event(c);
    e1 = get_event(c);
    HIP_TRY(c, hipEventRecord(e0, st));
    HIP_TRY(c, launch_expand(u.d_path_idx, u.d_location, u.n_uids, u.d_signs, u.path_length, g.method,
                             cb, n, b.row0.p, b.row1.p, st));
  }
  if (C.partial && !C.use_ie && g.K > 0) {   // the join left the inclusion-exclusion form on an earlier chunk
    if (e0) {
      c->ev_pool.push_back(e0);
      c->ev_pool.push_back(e1);
    }
    *end = ChunkEnd::kResplit;
    return GCRE_OK;
  }
  StatsArgs sa{};
  sa.p0 = jp.p0->d_rows;
  sa.p1 = jp.p1->d_rows;
  sa.row0 = b.row0.p;
  sa.row1 = b.row1.p;
  sa.case_mask = c->d_case_mask;
  sa.dvt = c->d_dvt;
  sa.key = b.key.p;
  sa.tot = b.tot.p;
  sa.cases = b.cases.p;
  sa.ctrls = b.ctrls.p;
  sa.res = R.keep ? jp.res->d_rows : nullptr;
  sa.first = cb;
  sa.count = n;
  sa.S = g.S;
  sa.Wp = g.Wp;
  gcre_recipe* rcp = R.rcp;
  if (C.use_ie && !C.hit && R.hinted && R.range_union_due)
    if (int rc = range_union_now(R)) return rc;
  if (C.use_sparse || C.use_ie) {
    collect_ie_stat(R);
    // the chunk's words of the flag block (6, 7: the join's).  Once a recipe has started, word kFlagOverReserved -- the
    // entries reserved so far in the recipe's overflow area -- is the JOIN's (FlagWord): written from over_next in front of
    // every inspector that fills the recipe, never zeroed
    HIP_TRY(c, hipMemsetAsync(R.flagblk, 0, (rcp && R.recipe_started) ? kFlagOverReserved * 4 : kFlagRangeUnion * 4, st));
    if (rcp) HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)(R.flagblk + kFlagOverReserved), (int)R.over_next, 1, st));
    R.recipe_started = R.recipe_started || rcp != nullptr;
    sa.max_tot = R.flagblk;
    HIP_TRY(c, hold(C, b.dcnt, (size_t)n * g.method, st));
    sa.dcnt = b.dcnt.p;
  }
  if (C.use_ie) {
    // one pass: statistics, kept rows, the check of the reduced operand, and the lists the null kernel streams
    const size_t nl = (size_t)n * g.method;
    HIP_TRY(c, hold(C, b.rowz, R.cap, st));
    HIP_TRY(c, hold(C, b.linfo, nl, st));
    HIP_TRY(c, hold(C, b.lover, nl, st));
    HIP_TRY(c, hold(C, b.dlist, nl * 8 + 16, st));
    // + the waves' chunk slack: every wave of the inspector may leave most of a kOverChunk reservation unused (no
    // inspector has more waves than k_stats_ie's grid of one block per kStatsIeBlockPaths paths)
    const size_t ie_blocks = ((size_t)n + kStatsIeBlockPaths - 1) / kStatsIeBlockPaths;
    const size_t over_slack = (std::min<size_t>((size_t)kInspectMaxBlocks, ie_blocks) * kInspectBlockWaves + 2) * kOverChunk;
    HIP_TRY(c, hold(C, b.dover, std::max<size_t>(b.dover.cap, nl * 2 + over_slack), st));
    if (rcp) {   // straight into the recipe of the kept set (absolute row = cb + i)
      C.rowz = rcp->rowz.p + cb;
      C.linfo = rcp->linfo.p + (size_t)cb * g.method;
      C.lover = rcp->lover.p + (size_t)cb * g.method;
      C.slot = rcp->slot.p + (size_t)cb * g.method * 8;
      C.over = rcp->over.p;
      C.over_cap = rcp->over.cap;
    } else {
      C.rowz = b.rowz.p;
      C.linfo = b.linfo.p;
      C.lover = b.lover.p;
      C.slot = b.dlist.p;
      C.over = b.dover.p;
      C.over_cap = b.dover.cap;
    }
    sa.pz = R.red->d_rows;
    sa.zindex = R.hinted ? u.d_red_index : nullptr;
    sa.excess = R.hinted ? R.exbuf->p : nullptr;
    sa.range_of = R.hinted ? u.d_range_of : nullptr;
    sa.bad = R.flagblk + kFlagHintBroken;
    sa.ie_bias = 8;
    sa.ie_rule = g.method == 1 ? 1 : 0;   // the bound filter and the quad kernel want overlap lists
    sa.rowz = C.rowz;
    sa.linfo = C.linfo;
    sa.lover = C.lover;
    sa.slot = C.slot;
    sa.over = C.over;
    sa.over_cap = (uint32_t)std::min<size_t>(C.over_cap - 16, 0xfffffff0u);
    if (rcp && !C.hit) HIP_TRY(c, hipMemcpyAsync(rcp->row0.p + cb, b.row0.p, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    sa.ov_count = R.flagblk + kFlagOverReserved;
    sa.zoff = (uint32_t)(64 * g.Wp) << 8;
    if (g.method == 2 && one_sided(R.red)) sa.lz_off = R.red->d_loff;   // one round per path instead of one per half
    if (!C.hit)   // method 1: counts from the reduced operand's row totals, where the join has at least as many paths as it has rows
      if (int rc = row_counts_for(c, R.red, R.P, st, &sa.z_counts)) return rc;
    if (!C.hit) HIP_TRY(c, launch_stats_ie(sa, g.method, st));
    // a kept row's carrier total bounds every count of it: the next level loads only the plane groups that can be non-zero
    if (rcp && !C.hit)
      HIP_TRY(c, hipMemcpyAsync(rcp->tot.p + (size_t)cb * g.method, b.tot.p, nl * 4, hipMemcpyDeviceToDevice, st));
  } else if (!C.hit) {
    HIP_TRY(c, launch_stats(sa, g.method, st));
  }
  if (!C.hit) {
    HIP_TRY(c, hipEventRecord(e1, st));
    if (R.mode != kInspect) HIP_TRY(c, hipEventRecord(c->ev_insp_main, st));
    R.ev_stats->emplace_back(e0, e1);
    if (ci) {
      ci->inspected = true;
      ci->with_lists = C.use_ie;
      ci->in_recipe = C.use_ie && rcp != nullptr;
    }
  }
  if (C.hit && ci->win_valid && C.scored) {   // the chunk's top-k does not depend on the masks either
    C.win = ci->win;
    C.sel_done = true;
    C.win_from_cache = true;
  }
  // the top-k selection only needs the keys the inspector just wrote: its digit passes run now, their state
  // comes back with the inspector's flags, its winners are collected before the null kernel starts
  C.hs = &c->h_sel;
  if (C.hit && ci->sel_open && C.scored && !C.sel_done && R.mode != kCount) {
    // the inspection that ran ahead queued the digit passes and left the rest to this call (score_chunk_ie, kInspect)
    C.sel_on = c->sel_stream;
    C.hs = ci->h_state;
    C.sel_begun = true;
  }
  if (C.use_ie && g.K > 0 && C.scored && !C.sel_done && !C.sel_begun && R.mode != kCount) {
    if (c->sel_async) {   // beside the warm-up slice and the null kernel, behind the inspector
      HIP_TRY(c, hipEventRecord(c->ev_sel, st));
      HIP_TRY(c, hipStreamWaitEvent(c->sel_stream, c->ev_sel, 0));
      C.sel_on = c->sel_stream;
    }
    if (ci && c->sel_defer && c->sel_async) {   // a state of the chunk's own: it may stay open behind other chunks' selections
      if (!ci->h_state) HIP_TRY(c, hipHostMalloc((void**)&ci->h_state, sizeof(SelectState), hipHostMallocDefault));
      C.hs = ci->h_state;
    }
    if (int rc = select_begin(c, b.key.p + C.s0, C.s1 - C.s0, c->top_k, C.hs, C.sel_on)) return rc;
    C.sel_begun = true;
  }
  *end = (!C.scored && !(C.use_ie && g.K > 0)) ? ChunkEnd::kNotNeeded : ChunkEnd::kOpen;
  return GCRE_OK;
}

// the IeArgs of a chunk's pruned launches: operands, their planes or the recipe they are rebuilt from, the lists, the tables
int fill_ie_args(JoinRun& R, const ChunkRun& C, IeArgs& ia, int64_t* nseg_scored, gcre_uids::SegCache** seg_entry) {
  gcre_ctx* c = R.c;
  const JoinPlan& jp = R.jp;
  const Geometry& g = R.g;
  const int64_t cb = C.cb, n = C.n;
  if (int rc = sparse_segments(c, *R.u, cb, n, cb + C.s0, cb + C.s1, R.res_planes ? R.pl_b : cb + C.s0,
                               R.res_planes ? R.pl_e : cb + C.s1, &ia.segs, &ia.nsegs, nseg_scored, seg_entry))
    return rc;
  ia.mt = R.w_mt;
  ia.tot = C.b->tot.p;
  ia.rowz = C.rowz;
  ia.planes0 = (R.have_p0 && !R.use_rec) ? jp.p0->d_planes : nullptr;
  ia.g0 = (R.have_p0 && !R.use_rec) ? jp.p0->plane_groups : 0;
  ia.planesz = R.have_pz ? R.red->d_planes : nullptr;
  ia.gz = R.have_pz ? R.red->plane_groups : 0;
  ia.rows0 = (uint32_t)(jp.p0->nrows * g.method);
  ia.rowsz = (uint32_t)(R.red->nrows * g.method);
  ia.rows_out = R.res_planes ? (uint32_t)(jp.res->nrows * g.method) : 0u;
  ia.loff0 = jp.p0->d_loff;
  ia.lidx0 = jp.p0->d_lidx;
  ia.linfo = C.linfo;
  ia.lover = C.lover;
  ia.dlist = C.slot;
  ia.dover = C.over;
  if (R.use_rec) {
    const gcre_recipe* r0 = jp.p0->rec;
    ia.rec_row0 = r0->row0.p;
    ia.rec_rowz = r0->rowz.p;
    ia.rec_linfo = r0->linfo.p;
    ia.rec_lover = r0->lover.p;
    ia.rec_slot = r0->slot.p;
    ia.rec_over = r0->over.p;
    ia.rec_planes_a = R.rec_a->d_planes;
    ia.rec_planes_z = R.rec_z->d_planes;
    ia.rec_rows_a = (uint32_t)(R.rec_a->nrows * g.method);   // row-halves
    ia.rec_rows_z = (uint32_t)(R.rec_z->nrows * g.method);
    ia.rec_ga = R.rec_a->plane_groups;
    ia.rec_gz = R.rec_z->plane_groups;
    if (g.method == 1) {
      // the recipe entries of every segment's row, next to the segment table (no load depends on row0 any more):
      // gathered by launch_ie_slices in front of the pruned launches that read them
      HIP_TRY(c, c->d_rec_segs.reserve((size_t)std::max<int64_t>(ia.nsegs, 1) * kRecSegWords));
      ia.rec_segs = c->d_rec_segs.p;
    }
  }
  ia.t32 = c->d_t32;
  ia.d64 = c->d_dmax;
  ia.ladder = c->d_ladder;
  ia.ladder_stride = g.TD;
  ia.lad_mode = !C.scored ? 1 : (c->ie_prune ? 0 : 2);
  ia.g00_rows = c->g00_rows;
  ia.null_bits = R.w_null;
  ia.planes_out = R.res_planes ? jp.res->d_planes : nullptr;
  ia.go = R.res_planes ? jp.res->plane_groups : 0;
  ia.out_first = cb;
  ia.score_begin = (uint32_t)C.s0;
  ia.score_end = (uint32_t)C.s1;
  ia.score_segs = (uint32_t)*nseg_scored;
  ia.nkt = R.nkt_sp;
  ia.K = g.K;
  ia.mt_rows = (uint32_t)(64 * g.Wp + 1);
  ia.zoff = (uint32_t)(64 * g.Wp) << 8;
  return GCRE_OK;
}

// The launches of a chunk's inclusion-exclusion road: the warm-up slice, then the pruned kernel -- the quad form where
// segments come in groups -- in one launch or in slices with a threshold exchange before each.  *quad: the quad form ran.
// `behind_slice` runs once the slice and the gather are queued and nothing of the pruned launches is.
int launch_ie_slices(JoinRun& R, const ChunkRun& C, IeArgs& ia, int planes, int64_t nseg_scored,
                     gcre_uids::SegCache* seg_entry, int64_t ie_tile_factor, bool* quad_ran,
                     const std::function<int()>& behind_slice) {
  gcre_ctx* c = R.c;
  const JoinPlan& jp = R.jp;
  const Geometry& g = R.g;
  hipStream_t st = R.st;
  const int64_t n = C.n;
  ia.seg_begin = 0;
  ia.seg_end = ia.nsegs;
  const bool warm_up = c->d_ladder && ia.lad_mode == 0;
  int64_t n_warm = 0;
  if (warm_up) {
    // warm-up: the first segments are scored without pruning (every count looked up, general kernel); what
    // they find seeds the thresholds the pruned kernel starts from.  Joins of a few thousand paths run here whole.
    // (the scored segments lead the table.)  The general kernel is several times slower per path: a short
    // shard gives it an eighth of its segments, not all of them.
    // every tile warms up on its own permutations: with many tiles the slice gets shorter (its cost is per tile)
    n_warm = warm_segments(c, nseg_scored, R.nkt_sp);
    // maxima shared with the other devices right after the warm-up: every device warms its share of the slice
    if (jp.exchange && R.exchanges_done < jp.exchanges && R.P > 0)
      n_warm = std::min(n_warm, std::max<int64_t>(64, (int64_t)((double)n_warm * (double)(R.se - R.sb) / (double)R.P) + 1));
    if (c->ie_warm_segs == 0) n_warm = 0;   // GCRE_IE_WARM=0 (tests): everything through the pruned kernel, thresholds from 0
  }
  // The recipe gather (k_fill_rec_segs) feeds the pruned launches only -- the slice reads the recipe itself -- so a join
  // that fits whole into its slice needs none, and any other gets it beside its slice, on the context's gather stream.
  // That stream starts behind everything queued on this one so far (ev_rec_in): the recipe copies, the segment-table
  // upload, and every earlier pruned launch that reads the one d_rec_segs buffer -- the chunk before this one, the slices
  // of an exchanged join, the level before, a join launched ahead; they are all on the context's main stream, as is
  // every join that gets here (an ahead inspection stops at its flags).  The pruned launches wait for ev_rec_done below.
  // Until they do, `gathering` waits for the gather stream on every way out: the gather reads the segment table and the
  // recipe of paths0, which the caller may free as soon as a failed join returns.
  struct Gathering {
    hipStream_t on = nullptr;
    ~Gathering() { if (on) (void)hipStreamSynchronize(on); }
  } gathering;
  const bool gather = ia.rec_segs != nullptr && n_warm < ia.nsegs;
  if (gather) {
    const gcre_recipe* r0 = jp.p0->rec;
    const bool beside = n_warm > 0 && c->rec_async && st == c->stream;
    if (beside) {
      HIP_TRY(c, hipEventRecord(c->ev_rec_in, st));
      HIP_TRY(c, hipStreamWaitEvent(c->rec_stream, c->ev_rec_in, 0));
      gathering.on = c->rec_stream;
    }
    // (the gather also zeroes the ticket counters of the first pruned launch: nothing on either stream uses them before)
    HIP_TRY(c, launch_fill_rec_segs(ia.segs, ia.nsegs, r0->row0.p, r0->rowz.p, r0->linfo.p, r0->lover.p, r0->slot.p, r0->tot.p,
                                    c->d_rec_segs.p, c->d_queue, beside ? c->rec_stream : st));
    if (beside) HIP_TRY(c, hipEventRecord(c->ev_rec_done, c->rec_stream));
  }
  if (warm_up) {
    IeArgs wa = ia;
    wa.seg_end = n_warm;
    // a wave walks its tiles one after the other: keep enough waves that each gets about four (segment, tile) items
    wa.waves_per_xcd = spread_waves(wa.waves_per_xcd, n_warm * R.nkt_sp, c->ie_warm_items);
    if (wa.timing) wa.timing += 12;   // diagnostics build: the slice's section clocks, next to the pruned launch's
    if (n_warm > 0) HIP_TRY(c, launch_null_ie(wa, g.method, planes, true, st));
    if (n_warm > 0 && wa.timing && R.mode != kLaunch) {
      uint64_t tw[7] = {0};
      HIP_TRY(c, hipMemcpyAsync(tw, wa.timing, sizeof tw, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      const double waves = 8.0 * wa.waves_per_xcd;
      std::fprintf(stderr, "[ie warm timing] level %d paths %lld segments %lld x %d tiles, waves %.0f: per-wave kcycles prologue %.1f paths to counts %.1f "
                   "transpose+look-ups %.1f flush %.1f (%.2f flushes) total %.1f, slowest wave %.1f\n", R.u->path_length, (long long)n,
                   (long long)n_warm, wa.nkt, waves, tw[0] / waves / 1e3, tw[1] / waves / 1e3, tw[2] / waves / 1e3, tw[3] / waves / 1e3,
                   (double)tw[4] / waves, tw[5] / waves / 1e3, tw[6] / 1e3);
    }
    ia.seg_begin = n_warm;
  }
  if (int rc = behind_slice()) return rc;
  if (gathering.on) {   // from here on this stream carries the gather: whoever waits for it waits for both
    HIP_TRY(c, hipStreamWaitEvent(st, c->ev_rec_done, 0));
    gathering.on = nullptr;
  }
  if (ia.seg_begin >= ia.seg_end) return GCRE_OK;
  ia.queue = c->d_queue;
  ia.batch = c->ie_batch;
  // method 1, no plane output: the quad form (gcre_ieq.hip) wherever segments come in groups that join the same
  // paths1 rows -- every level but the one whose uids are the genes themselves (one uid per pivot)
  bool quad = false;
  if (g.method == 1 && c->d_ladder && c->ie_quad && !ia.planes_out && seg_entry &&
      ensure_quads(c, *R.u, *seg_entry, ia.seg_begin) == GCRE_OK) {
    const int64_t nq = seg_entry->nquads - seg_entry->quad_begin;
    // worth it from 1 + (qmax - 1) / 4 segments per quad on average: 1.25 with two segments per quad (a quad of one
    // segment does what k_null_ie_m1 does with a longer prologue); the 1.5 of the four-segment form could never be
    // reached by joins that average 1.3-1.5
    const int64_t qmax = ieq_quad_segs();
    quad = nq > 0 && ((ia.seg_end - ia.seg_begin) * 4 >= nq * (4 + (qmax - 1)) || c->ie_quad == 2);
    if (std::getenv("GCRE_HOST_TIMING"))
      std::fprintf(stderr, "[host] quads: %lld segments in %lld quads (%.2f per quad), %lld joined paths, quad form %s\n",
                   (long long)(ia.seg_end - ia.seg_begin), (long long)nq, (double)(ia.seg_end - ia.seg_begin) / (double)std::max<int64_t>(nq, 1),
                   (long long)n, quad ? "on" : "off");
    if (quad) {
      ia.quads = seg_entry->d_quads;
      ia.quad_begin = seg_entry->quad_begin;
      ia.quad_end = seg_entry->nquads;
      // an added row's planes are a 32-bit byte offset from the tile's first row wherever a tile of them stays below 4 GiB
      const uint64_t z_units = (uint64_t)ia.rowsz * (uint64_t)ia.gz;
      // (the queue's drain addresses a mask row through a range-checked 31-bit vector offset)
      ia.flagq = (c->ie_flagq && (uint64_t)ia.mt_rows * 256u < (1ull << 31)) ? 1u : 0u;
      ia.z_wide = (c->ie_zwide || z_units >= (1ull << 22)) ? 1u : 0u;
      ia.z_tile_units = ia.z_wide ? 0u : (uint32_t)z_units;
      ia.batch = c->ieq_batch > 0 ? c->ieq_batch : std::max(1, c->ie_batch * 2);   // quads per ticket: the headers of a ticket's quads are fetched one ahead
      const int wq = std::min(c->sparse_waves_per_cu, ieq_max_waves_per_cu(planes, ia.gz, ia.rec_slot != nullptr, ia.z_wide != 0u));
      ia.waves_per_xcd = spread_waves(xcd_waves(c, wq), n * ie_tile_factor, 128);
    }
  }
  // tickets are 32-bit: (batches per tile) x tiles must stay below 2^32
  while (((ia.nsegs - ia.seg_begin) / ia.batch + 1) * (int64_t)ia.nkt > (int64_t)0xf0000000ll) ia.batch *= 2;
  // One launch -- or, when the maxima are shared with other devices as the join goes (gcre_join_opts.exchange),
  // E slices with an exchange before each, so that the thresholds of a shard follow the whole level's maxima: the
  // first slices double (1/2^k of the head), the last m = exchange_tail are equal steps 1/(m+1) of the range.
  // Measured at 8 ranks on configs[3]: equal steps at the end and up to 16 exchanges halve the
  // look-ups once more but every slice is a launch that starts cold -- doubling slices alone (m = 0) stay best.
  const bool pruned = c->d_ladder && ia.lad_mode == 0;
  const int n_slices = (pruned && jp.exchange) ? std::max(1, jp.exchanges - R.exchanges_done) : 1;
  const int64_t r_b = quad ? ia.quad_begin : ia.seg_begin, r_e = quad ? ia.quad_end : ia.seg_end;
  int64_t lo = r_b;
  for (int sl = 0; sl < n_slices && lo < r_e; sl++) {
    int64_t hi = r_e;
    if (sl + 1 < n_slices) {
      const int m = std::min(n_slices - 1, c->exchange_tail < 0 ? n_slices / 2 : c->exchange_tail), head = n_slices - m;
      const double end = sl >= head ? (double)(sl - head + 2) / (double)(m + 1) : std::ldexp(1.0 / (double)(m + 1), -(head - 1 - sl));
      hi = std::min(r_e, std::max(lo + 1, r_b + (int64_t)((double)(r_e - r_b) * end)));
    }
    if (pruned && jp.exchange)
      if (int rc = exchange_now(R)) return rc;
    IeArgs sa2 = ia;
    if (quad) { sa2.quad_begin = lo; sa2.quad_end = hi; }
    else { sa2.seg_begin = lo; sa2.seg_end = hi; }
    if (sl > 0 || !gather) HIP_TRY(c, hipMemsetAsync(sa2.queue, 0, 8 * 16 * 4, st));   // (the first launch's: zeroed by the gather)
    if (quad) HIP_TRY(c, launch_null_ie_quad(sa2, planes, st));
    else HIP_TRY(c, launch_null_ie(sa2, g.method, planes, c->d_ladder == nullptr, st));
    lo = hi;
  }
  if (quad) R.prof->ie_quad_launches++;
  *quad_ran = quad;
  return GCRE_OK;
}

// GCRE_IE_TIMING=1 with a diagnostics build (-DGCRE_IE_TIMING): the section counters of the chunk's pruned launches (stderr)
int print_ie_timing(JoinRun& R, const ChunkRun& C, const IeArgs& ia, bool quad) {
  gcre_ctx* c = R.c;
  const int64_t n = C.n;
  uint64_t tmv[12] = {0};
  HIP_TRY(c, hipMemcpyAsync(tmv, c->d_ie_timing.p, sizeof tmv, hipMemcpyDeviceToHost, R.st));
  HIP_TRY(c, hipStreamSynchronize(R.st));
  const double waves = 8.0 * ia.waves_per_xcd;
  if (R.g.method == 2)
    std::fprintf(stderr, "[ie2 classes] paths %lld x %d tiles: path-tiles with the other half empty %llu, one test %llu, all steps %llu, both halves %llu; "
                 "lists of 5-8 rows %llu, long lists %llu; permutations looked up %llu\n", (long long)n, ia.nkt, (unsigned long long)tmv[0],
                 (unsigned long long)tmv[1], (unsigned long long)tmv[2], (unsigned long long)tmv[3], (unsigned long long)tmv[4],
                 (unsigned long long)tmv[6], (unsigned long long)tmv[5]);
  else if (quad)
    std::fprintf(stderr, "[ieq timing] paths %lld waves %.0f quads/wave %.0f: per-wave Mcycles header+loads %.2f base counters %.2f intervals %.2f filter pass %.2f exact pass %.2f exchange %.2f total %.2f; "
                 "inside the filter pass: second look / queueing %.2f drains %.2f; flagged path-tiles %llu with %llu flagged permutations\n",
                 (long long)n, waves, tmv[7] / waves, tmv[0] / waves / 1e6, tmv[1] / waves / 1e6, tmv[2] / waves / 1e6, tmv[3] / waves / 1e6,
                 tmv[4] / waves / 1e6, tmv[5] / waves / 1e6, tmv[6] / waves / 1e6, tmv[8] / waves / 1e6, tmv[9] / waves / 1e6,
                 (unsigned long long)tmv[10], (unsigned long long)tmv[11]);
  else
    std::fprintf(stderr, "[ie filter] uncertain path-tiles %llu of %lld x %d tiles, lanes that fetched rows %llu\n",
                 (unsigned long long)tmv[1], (long long)n, ia.nkt, (unsigned long long)tmv[3]);
  std::fprintf(stderr, "[ie timing] paths %lld out %d waves %.0f: per-wave Mcycles seg %.2f load %.2f comp(incl load) %.2f lookup %.2f exch %.2f total %.2f, slowest wave %.2f\n",
               (long long)n, ia.planes_out != nullptr, waves, tmv[0] / waves / 1e6, tmv[1] / waves / 1e6,
               tmv[2] / waves / 1e6, tmv[3] / waves / 1e6, tmv[4] / waves / 1e6, tmv[5] / waves / 1e6, tmv[6] / 1e6);
  return GCRE_OK;
}

// The inclusion-exclusion road of a chunk (gcre_ie.hip): the inspector's flags and the checks that send the chunk round
// again, then -- unless the chunk was only to be inspected (kInspect), is priced out or needs no scoring -- its pruned
// launches (kLaunch: their look-up counter goes behind the launch's maxima).
int score_chunk_ie(JoinRun& R, ChunkRun& C, ChunkEnd* end) {
  gcre_ctx* c = R.c;
  const JoinPlan& jp = R.jp;
  const Geometry& g = R.g;
  hipStream_t st = R.st;
  ChunkInsp* ci = C.ci;
  const int64_t cb = C.cb, n = C.n;
  const auto ti0 = std::chrono::steady_clock::now();
  if (C.hit) {
    std::memcpy(C.flags, ci->flags, sizeof C.flags);   // as the inspector left them (no round trip)
  } else {
    HIP_TRY(c, hipMemcpyAsync(C.flags, R.flagblk, sizeof C.flags, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
  }
  const uint32_t over_used = C.flags[kFlagOverReserved];
  if ((size_t)over_used + 16 > C.over_cap) {
    // more long lists than the area holds: size it from what the pass asked for, run the chunk again (a recipe
    // keeps what the earlier chunks wrote; the failed attempt's reservation is simply left unused)
    const size_t want = (size_t)over_used + (size_t)over_used / 4 + ((size_t)1 << 24);
    if (R.rcp) HIP_TRY(c, R.rcp->over.grow_keep(want, R.rcp->over.cap, st));
    else HIP_TRY(c, C.b->dover.reserve(want));
    if (ci) ci->inspected = false;
    *end = ChunkEnd::kRedoOverflow;
    return GCRE_OK;
  }
  const uint64_t n_list = (uint64_t)(n * g.method) * 8 + over_used;
  if (R.rcp) R.over_next = std::max(R.over_next, over_used);
  const uint32_t max_tot = C.flags[kFlagMaxTot];
  R.join_max_tot = std::max(R.join_max_tot, max_tot);
  R.join_max_len = std::max(R.join_max_len, C.flags[kFlagMaxLen]);
  if (C.flags[kFlagHintBroken] != 0 || (R.hinted && C.flags[kFlagRangeUnion] != 0)) {
    // the hint does not describe this join: run it on paths1 itself (identity map) from this chunk on
    if (!R.hinted) return fail(c, GCRE_ERR_DEVICE, "internal: joined path differs from paths0 | paths1");
    R.hinted = false;
    if (int rc = prepare_z(R)) return rc;
    if (!R.have_pz) R.want_ie = false;
    // the kept rows' planes were sized for the reduced rows: rows of paths1 may carry more
    if (R.res_planes && plane_groups_for(std::min<uint32_t>((uint32_t)(64 * g.Wp), row_max(c, jp.p0) + row_max(c, R.red))) >
                            jp.res->plane_groups) {
      R.res_planes = false;
      R.res_planes_ok = false;
    }
    if (cb > C.sg->b || C.sg != &R.segs.front()) {   // earlier chunks added rows of another set
      R.recipe_broken = true;
      R.hint_broke_late = true;
    }
    if (ci) ci->inspected = false;
    *end = ChunkEnd::kRedoHint;
    return GCRE_OK;
  }
  if (ci && !C.hit) {
    std::memcpy(ci->flags, C.flags, sizeof C.flags);
    ci->flags_valid = true;
  }
  if (R.mode == kInspect) {   // nothing of the permutation kernel's
    if (C.sel_begun && !C.sel_done) {
      if (c->sel_defer && ci && C.hs == ci->h_state && C.sel_on == c->sel_stream) {
        // the selection stays open: nothing the launch needs depends on it, so the launch queues its slice and its gather
        // first and closes it behind them (below, behind_slice); a join that is not launched closes it in its own call, the
        // same way
        ci->sel_open = true;
        C.sel_left_open = true;
      } else {   // the chunk's winners are collected next
        HIP_TRY(c, hipStreamSynchronize(C.sel_on));
        if (int rc = finish_selection(R, C)) return rc;
      }
    }
    *end = ChunkEnd::kInspected;
    return GCRE_OK;
  }
  const int64_t nseg_est = std::max<int64_t>(uids_in(*R.u, cb, n), 1);
  if (c->null_kernel == 0 && C.scored && ie_dearer(g, R.nkt_sp, R.have_p0, row_max(c, jp.p0), nseg_est, n, n_list)) {
    R.res_planes_ok = false;
    *end = C.partial ? ChunkEnd::kResplit : ChunkEnd::kPricedOut;
    return GCRE_OK;
  }
  if (!C.scored && !(R.res_planes && cb < R.pl_e && cb + n > R.pl_b)) {   // rows of another shard that only needed their recipe entries
    *end = ChunkEnd::kNotNeeded;
    return GCRE_OK;
  }
  const int planes = counter_planes(max_tot);
  IeArgs ia{};
  int64_t nseg_scored = 0;
  gcre_uids::SegCache* seg_entry = nullptr;
  if (int rc = fill_ie_args(R, C, ia, &nseg_scored, &seg_entry)) return rc;
  R.prof->null_row_loads += ((R.have_p0 ? 0.0 : (double)row_max(c, jp.p0) * g.method * (double)nseg_est) + (double)n_list) * R.nkt_sp;
  const int wpc = std::min(c->sparse_waves_per_cu, ie_max_waves_per_cu(g.method, planes, ia.gz, ia.planes_out != nullptr, ia.rec_slot != nullptr));
  // small joins: a wave's fixed costs (cold TLB and caches, LDS set-up, threshold exchange) are per tile it
  // visits, so give every wave at least ~32 joined paths of a tile -- counting the tiles a queue can hold whole
  // (a wave walks a contiguous piece of the tile-major sequence)
  const int64_t ie_tile_factor = std::min(std::max(R.nkt_sp * c->ie_small_join_tiles / 8, 1), R.nkt_sp);
  ia.waves_per_xcd = spread_waves(xcd_waves(c, wpc), n * ie_tile_factor, 32);
  R.prof->inspect_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ti0).count();
  ia.stats = R.mode == kLaunch ? R.w_null + g.Kpad : R.flagblk + kFlagLookupTiles;   // zeroed with the block before the inspector ran
  if (jp.exceed || R.mode == kCount) {   // (a counting pass for a hit list alone stops here too)
    C.ie = ia;
    C.ie_planes = planes;
    C.ie_segs = nseg_scored;
    C.ie_ok = true;
    if (R.mode == kCount) {   // this chunk's null kernels ran with the launch: only the count is left (run_chunk)
      *end = ChunkEnd::kScored;
      return GCRE_OK;
    }
  }
  const bool timing = std::getenv("GCRE_IE_TIMING") != nullptr;   // diagnostics builds only (-DGCRE_IE_TIMING)
  if (timing) {
    HIP_TRY(c, c->d_ie_timing.reserve(24));   // [0,12) the pruned launches, [12,24) the warm-up slice
    HIP_TRY(c, hipMemsetAsync(c->d_ie_timing.p, 0, 192, st));
    ia.timing = c->d_ie_timing.p;
  }
  if (C.sel_begun && C.sel_on == st)   // (its state came back with the flags)
    if (int rc = finish_selection(R, C)) return rc;
  hipEvent_t n0 = get_event(c), n1 = get_event(c);
  bool quad = false;
  // own stream: the digit passes ran beside whatever was queued since they were; the rest of the selection follows them
  auto close_selection = [&]() -> int {
    const auto tw0 = std::chrono::steady_clock::now();
    HIP_TRY(c, hipStreamSynchronize(C.sel_on));
    R.select_wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count();
    if (int rc = finish_selection(R, C)) return rc;
    if (R.mode == kLaunch)   // (no collect_winners behind it books this)
      R.select_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count();
    return GCRE_OK;
  };
  // A selection that an ahead inspection left open is closed between the slice and the pruned launch, and the pruned launch
  // waits for it on the device: its digit passes have had the inspection's tail, this call's set-up and the slice to run
  // beside, while a pruned kernel is persistent and fills the chip -- one-block kernels of another stream queued beside it
  // (k_select_step, measured) wait until it ends, and the winners then cost the join its tail instead of nothing
  auto behind_slice = [&]() -> int {
    if (!(C.sel_begun && !C.sel_done && ci && ci->sel_open && C.sel_on != st)) return GCRE_OK;
    if (int rc = close_selection()) return rc;
    HIP_TRY(c, hipEventRecord(c->ev_sel_done, C.sel_on));
    HIP_TRY(c, hipStreamWaitEvent(st, c->ev_sel_done, 0));
    return GCRE_OK;
  };
  HIP_TRY(c, hipEventRecord(n0, st));
  if (int rc = launch_ie_slices(R, C, ia, planes, nseg_scored, seg_entry, ie_tile_factor, &quad, behind_slice)) return rc;
  HIP_TRY(c, hipEventRecord(n1, st));
  if (C.sel_begun && !C.sel_done)
    if (int rc = close_selection()) return rc;
  if (timing && R.mode != kLaunch)
    if (int rc = print_ie_timing(R, C, ia, quad)) return rc;
  R.ev_null->emplace_back(n0, n1);
  if (C.scored) {
    R.prof->null_kernel_launches++;
    R.prof->null_alg_bytes += alg_bytes(R, cb + C.s0, C.s1 - C.s0);
  }
  R.prof->ie_launches++;
  R.prof->ie_overlap_lists += C.flags[kFlagOverlapLists];
  R.ie_stat_pending = true;
  R.ie_ran = true;
  *end = ChunkEnd::kScored;
  return GCRE_OK;
}

// Delta streaming (gcre_sparse.hip): per joined path the bits paths1 adds on top of paths0 -- offsets by a device scan of
// the counts k_stats left, entries by k_delta_fill -- once per chunk, shared by all permutation tiles.  kPricedOut: the
// dense kernel is cheaper.
int score_chunk_sparse(JoinRun& R, ChunkRun& C, ChunkEnd* end) {
  gcre_ctx* c = R.c;
  const JoinPlan& jp = R.jp;
  const gcre_uids& u = *R.u;
  const Geometry& g = R.g;
  hipStream_t st = R.st;
  ChunkBufs& b = *C.b;
  ChunkInsp* ci = C.ci;
  const int64_t cb = C.cb, n = C.n;
  if (int rc = ensure_lists(c, jp.p0)) return rc;
  if (int rc = ensure_lists(c, jp.p1)) return rc;
  const uint32_t zoff = (uint32_t)(64 * g.Wp) << 8;
  const int64_t nl = n * g.method;   // delta lists: one per joined path and half
  HIP_TRY(c, c->d_doff.reserve((size_t)nl + 1));
  HIP_TRY(c, c->d_scan.reserve((size_t)(nl + 1023) / 1024 + 2));
  HIP_TRY(c, launch_scan_u32_u64(b.dcnt.p, nl, c->d_doff.p, c->d_scan.p, st));
  uint32_t max_tot = 0;
  uint64_t n_delta = 0;
  HIP_TRY(c, hipMemcpyAsync(&max_tot, R.flagblk + kFlagMaxTot, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(&n_delta, c->d_doff.p + nl, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (C.hit) max_tot = ci->flags[kFlagMaxTot];   // the flag block was cleared for this window; the inspector's value was kept
  else if (ci) { ci->flags[kFlagMaxTot] = max_tot; ci->flags_valid = true; }
  if (c->null_kernel == 0 && sparse_dearer(g, n_delta, max_tot, std::max<int64_t>(uids_in(u, cb, n), 1), n)) {
    *end = ChunkEnd::kPricedOut;
    return GCRE_OK;
  }
  if (ci) ci->with_lists = false;   // the delta lists below take the place of the inspector's
  HIP_TRY(c, b.dlist.reserve((size_t)n_delta + 16));
  HIP_TRY(c, launch_delta_fill((const uint32_t*)jp.p0->d_rows, 2 * g.S, 2 * g.Wp, g.method, b.row0.p, b.row1.p, n,
                               jp.p1->d_loff, jp.p1->d_lidx, c->d_doff.p, zoff, b.dlist.p, st));
  const int planes = counter_planes(max_tot);
  SparseArgs sp{};
  int64_t nseg_scored = 0;
  if (int rc = sparse_segments(c, u, cb, n, cb, cb + n, cb, cb + n, &sp.segs, &sp.nsegs, &nseg_scored)) return rc;
  sp.mt = R.w_mt;
  sp.tot = b.tot.p;
  sp.loff0 = jp.p0->d_loff;
  sp.lidx0 = jp.p0->d_lidx;
  sp.doff = c->d_doff.p;
  sp.dlist = b.dlist.p;
  sp.t32 = c->d_t32;
  sp.d64 = c->d_dmax;
  sp.null_bits = R.w_null;
  sp.nkt = (g.K + kSparseTile - 1) / kSparseTile;
  sp.mt_rows = (uint32_t)(64 * g.Wp + 1);
  sp.zoff = zoff;
  {
    // mask-row loads of this launch: every segment walks its paths0 list(s) once, every joined path its
    // delta list(s), for each permutation tile
    const auto& pi = u.h_path_idx;
    const auto& lo = jp.p0->h_loff;
    double base_entries = 0;
    int64_t i = std::upper_bound(pi.begin(), pi.end(), cb) - pi.begin() - 1;
    for (; i < u.n_uids && pi[(size_t)i] < cb + n; i++) {
      const int64_t a0 = std::max(pi[(size_t)i], cb), a1 = std::min(pi[(size_t)i + 1], cb + n);
      if (a1 <= a0) continue;
      const double segs_here = (double)((a1 - a0 + kSparseSegMax - 1) / kSparseSegMax);
      base_entries += segs_here * (double)(lo[(size_t)(i + 1) * g.method] - lo[(size_t)i * g.method]);
    }
    R.prof->null_row_loads += (base_entries + (double)n_delta) * sp.nkt;
  }
  sp.waves_per_xcd = xcd_waves(c, std::min(c->sparse_waves_per_cu, sparse_max_waves_per_cu(g.method, planes)));
  hipEvent_t n0 = get_event(c), n1 = get_event(c);
  HIP_TRY(c, hipEventRecord(n0, st));
  HIP_TRY(c, launch_null_sparse(sp, g.method, planes, st));
  HIP_TRY(c, hipEventRecord(n1, st));
  R.ev_null->emplace_back(n0, n1);
  R.prof->null_kernel_launches++;
  R.prof->null_alg_bytes += alg_bytes(R, cb, n);
  *end = ChunkEnd::kScored;
  return GCRE_OK;
}

// the AND+BCNT kernel on the bit rows themselves (gcre_kernels.hip)
int score_chunk_dense(JoinRun& R, ChunkRun& C) {
  gcre_ctx* c = R.c;
  const Geometry& g = R.g;
  const ChunkBufs& b = *C.b;
  NullArgs na{};
  na.p0 = (const uint32_t*)R.jp.p0->d_rows;
  na.p1 = (const uint32_t*)R.jp.p1->d_rows;
  na.masks = R.w_masks;
  na.row0 = b.row0.p;
  na.row1 = b.row1.p;
  na.tot = b.tot.p;
  na.t32 = c->d_t32;
  na.d64 = c->d_dmax;
  na.d64n = c->d_dmaxn ? c->d_dmaxn : c->d_dmax;
  na.null_bits = R.w_null;
  na.npaths = C.n;
  na.npt = C.npt;
  na.S32 = 2 * g.S;
  na.W32p = 2 * g.Wp;
  na.Kpad = R.Kstride;
  na.nkt = (g.K + R.cfg.perm_tile - 1) / R.cfg.perm_tile;
  const int64_t want = (int64_t)c->cus * c->null_blocks_per_cu;
  int64_t groups = std::max<int64_t>(1, want / na.nkt);
  groups = std::min<int64_t>(groups, C.npt);
  na.pgroups = (int)groups;
  hipEvent_t n0 = get_event(c), n1 = get_event(c);
  HIP_TRY(c, hipEventRecord(n0, R.st));
  HIP_TRY(c, launch_null(na, g.method, R.cfg, R.st));
  HIP_TRY(c, hipEventRecord(n1, R.st));
  R.ev_null->emplace_back(n0, n1);
  R.prof->null_kernel_launches++;
  R.prof->null_alg_bytes += alg_bytes(R, C.cb, C.n);
  return GCRE_OK;
}

// ---- top-k of a scored chunk: the selection (finished, or run whole), its winners into the join's candidates ----
int collect_winners(JoinRun& R, ChunkRun& C) {
  gcre_ctx* c = R.c;
  hipStream_t st = R.st;
  const auto ts0 = std::chrono::steady_clock::now();
  if (!C.sel_done) {
    if (C.sel_begun) {   // begun, then the chunk left the inclusion-exclusion road: its state is still good
      HIP_TRY(c, hipStreamSynchronize(C.sel_on));
      if (int rc = finish_selection(R, C)) return rc;
    } else {
      if (c->sel_stream) HIP_TRY(c, hipStreamSynchronize(c->sel_stream));   // an abandoned selection shares the scratch
      uint32_t nsel = 0;
      if (int rc = select_chunk(c, C.b->key.p + C.s0, C.s1 - C.s0, c->top_k, &nsel, st)) return rc;
      if (int rc = queue_winners(c, *C.b, C.s0, nsel, C.win, C.sel_on)) return rc;
    }
    // whatever still runs on the selection stream reads this chunk's keys and rows: the next chunk's inspector (on the
    // main stream) rewrites them, so it queues behind an event -- not behind "the results are discarded anyway"
    if (C.sel_on != st) {
      HIP_TRY(c, hipEventRecord(c->ev_sel_done, C.sel_on));
      HIP_TRY(c, hipStreamWaitEvent(st, c->ev_sel_done, 0));
    }
  }
  const Winners& win = C.win;
  if (win.n > 0) {
    const auto tw0 = std::chrono::steady_clock::now();
    if (!C.win_from_cache) {   // (cached winners are host data: nothing to wait for)
      if (C.sel_on != st) HIP_TRY(c, hipStreamSynchronize(C.sel_on));
      HIP_TRY(c, hipStreamSynchronize(st));   // the null kernel of this chunk: its time is not the selection's
      unpack_winners(C.win);
    }
    R.select_wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count();
    push_candidates(R.cands, win, C.cb + C.s0);
  }
  if (C.ci && !C.ci->win_valid) {   // (its copies have arrived: the stream was waited for above)
    C.ci->win = win;
    C.ci->win_valid = true;
  }
  R.select_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts0).count();
  return GCRE_OK;
}

// One attempt at the chunk [cb, ce).  *end tells the chunk loop whether to run it again.
int run_chunk(JoinRun& R, const Seg& sg, int64_t cb, int64_t ce, ChunkEnd* end) {
  ChunkRun C;
  *end = ChunkEnd::kOpen;
  if (int rc = open_chunk(R, C, sg, cb, ce)) return rc;
  if (R.mode == kCount && !C.hit)   // (its inspector would rewrite what the joins launched behind this one are reading)
    return fail(R.c, GCRE_ERR_DEVICE, "internal: the counting pass of a join launched ahead met a chunk that is not in the inspection cache");
  if (int rc = inspect_chunk(R, C, end)) return rc;
  if (*end == ChunkEnd::kOpen && R.g.K > 0 && C.use_ie)
    if (int rc = score_chunk_ie(R, C, end)) return rc;
  if (*end == ChunkEnd::kResplit || *end == ChunkEnd::kRedoOverflow || *end == ChunkEnd::kRedoHint) {
    // the abandoned digit passes may still be reading the keys the relaunched inspector is about to rewrite
    if (C.sel_begun && C.sel_on != R.st) {
      HIP_TRY(R.c, hipEventRecord(R.c->ev_sel_done, C.sel_on));
      HIP_TRY(R.c, hipStreamWaitEvent(R.st, R.c->ev_sel_done, 0));
    }
    return GCRE_OK;
  }
  if (!C.scored) return GCRE_OK;
  if (R.g.K > 0 && R.mode != kCount && (*end == ChunkEnd::kOpen || *end == ChunkEnd::kPricedOut)) {
    if (R.mode == kInspect) {
      if (C.use_sparse && C.ci) {
        // the delta-streaming road sizes its counters from the inspector's flag block: an ahead inspection reads it now and
        // leaves it with the chunk (the launch that replays the chunk finds the block cleared)
        HIP_TRY(R.c, hipMemcpyAsync(C.ci->flags, R.flagblk, sizeof C.ci->flags, hipMemcpyDeviceToHost, R.st));
        HIP_TRY(R.c, hipStreamSynchronize(R.st));
        C.ci->flags_valid = true;
      }
    } else {
      if (C.use_sparse)
        if (int rc = score_chunk_sparse(R, C, end)) return rc;
      if (*end != ChunkEnd::kScored)
        if (int rc = score_chunk_dense(R, C)) return rc;
    }
  }
  // the chunk's keys are final (no stage sends it round again) and still in place: the tally reads them behind the chunk's
  // own kernels, before the next chunk's inspector -- on this stream too -- may rewrite them
  if (R.jp.tally && R.mode == kFull)
    if (int rc = fold_genes(R.c, R.jp.tally, *C.b, C.cb, C.s0, C.s1, R.st)) return rc;
  if (R.jp.exceed && (R.mode == kFull || R.mode == kCount))
    if (int rc = count_exceed(R.c, R.jp, *C.b, C.s0, C.s1, R.st, (C.ie_ok && *end == ChunkEnd::kScored) ? &C.ie : nullptr,
                              C.ie_planes, C.ie_segs))
      return rc;
  if (R.jp.hits && (R.mode == kFull || R.mode == kCount))
    if (int rc = collect_hits(R.c, R.jp.hits, *C.b, C.cb, C.s0, C.s1, R.st)) return rc;
  if (R.mode == kCount) return GCRE_OK;
  if (C.sel_left_open) return GCRE_OK;   // (kInspect: its winners come with the call that closes the selection)
  if (R.mode == kLaunch && R.c->sel_defer && C.ci && C.sel_done && !C.win_from_cache && C.sel_on == R.c->sel_stream) {
    // closed behind the null kernels: the winners' copies are queued and land in the chunk's entry, nothing is waited for;
    // finish_launched unpacks them.  The next selection on that stream -- another chunk's, the next join's -- is behind them
    C.ci->win = std::move(C.win);
    C.ci->win_pending = true;
    R.u->launch.sel_pending = true;
    R.prof->paths += C.s1 - C.s0;
    return GCRE_OK;
  }
  if (int rc = collect_winners(R, C)) return rc;
  if (R.mode != kInspect) R.prof->paths += C.s1 - C.s0;   // (a launch books them on the profile of the join it is for)
  return GCRE_OK;
}

// After the chunks: what the join leaves with its operands and its join index, then by mode -- kInspect marks its stream,
// kLaunch leaves the launch with the join index, kFull delivers the result (and runs the registered chain)
int finish_join(JoinRun& R) {
  gcre_ctx* c = R.c;
  const JoinPlan& jp = R.jp;
  const gcre_uids& u = *R.u;
  const Geometry& g = R.g;
  hipStream_t st = R.st;
  if (R.P > 0) {
    if (R.mode == kFull) collect_ie_stat(R);
    if (R.rcp && R.want_ie && !R.recipe_broken) {
      // the recipe names its operands by id and row version: the set paths0 was, and the rows the join really added
      R.rcp->a_id = jp.p0->id;
      R.rcp->a_ver = jp.p0->version;
      R.rcp->z_id = R.red->id;
      R.rcp->z_ver = R.red->version;
      R.rcp->valid = true;
      R.rcp->max_len = R.join_max_len;
      jp.res->max_bits = (R.join_max_tot + 3u) & ~3u;
      jp.res->max_known = true;
    }
    if (c->insp_cache) {
      u.insp_hinted = R.hinted;
      u.insp_res_ver = R.keep ? jp.res->version : 0;
      u.insp_valid = !R.hint_broke_late;
    }
    if (R.ie_ran && R.hinted) R.prof->ie_hinted_joins++;
    if (R.ie_ran && R.have_p0) R.prof->ie_plane_joins++;
  }
  if (R.mode == kCount) return GCRE_OK;
  if (R.mode == kInspect) {
    // everything this inspection queued is behind this event: the join proper waits for it on the main stream
    HIP_TRY(c, hipEventRecord(c->ev_insp_done, st));
    return GCRE_OK;
  }
  if (R.res_planes && R.res_planes_ok && g.K > 0) {
    // the kept rows leave with their count planes: the next level's N0 (gcre_ie.hip)
    jp.res->planes_epoch = c->mask_epoch;
    jp.res->planes_valid = true;
    jp.res->planes_lo = R.pl_b;
    jp.res->planes_hi = R.pl_e;
    jp.res->max_bits = (R.join_max_tot + 3u) & ~3u;
    jp.res->max_known = true;
  }
  // a join that took another road (small, unpruned, another kernel form) still makes the calls the other devices expect
  while (jp.exchange && R.exchanges_done < jp.exchanges)
    if (int rc = exchange_now(R)) return rc;
  if (R.mode == kLaunch) {
    // launched: the kernels are queued, nothing is waited for.  What the join's own call will need stays with the index
    gcre_uids::Launched& L = u.launch;
    HIP_TRY(c, hipEventRecord(L.done, st));
    if (L.sel_pending) HIP_TRY(c, hipEventRecord(L.sel_done, c->sel_stream));
    R.prof->select_ms += std::max(0.0, R.select_ms - R.select_wait_ms);
    L.cands = std::move(R.cands);
    L.key = R.ikey;
    L.res_ver = R.keep ? jp.res->version : 0;
    L.mask_epoch = c->mask_epoch;
    L.win_k0 = c->win_k0;
    L.win_K = c->win_K;
    L.active = true;
    return GCRE_OK;
  }
  if (int rc = deliver_join(c, jp, R.out, g.K, R.w_null, st, R.cands, c->ev_null, c->ev_stats, R.t_begin, std::move(R.ahead_plan)))
    return rc;
  c->prof.select_ms = std::max(0.0, R.select_ms - R.select_wait_ms);
  return GCRE_OK;
}

// The join driver (JoinExec::join): chunks of at most chunk_paths joined paths, each inspected, scored against the
// permutations of the window and reduced to its top-k; a chunk the stages send round again runs again from its start.
int run_join(gcre_ctx* c, const JoinPlan& jp, gcre_result* out, JoinMode mode) {
  JoinRun R(c, jp, out, mode);
  Begin next = Begin::kDone;
  if (int rc = begin_join(R, &next)) return rc;
  if (next == Begin::kDone) return GCRE_OK;
  if (next == Begin::kFinishLaunched) return finish_launched(c, jp, out);
  if (R.P > 0) {
    plan_segments(R);
    if (int rc = prepare_operands(R)) return rc;
    for (const Seg& sg : R.segs) {
      int64_t cb = sg.b;
      while (cb < sg.e) {
        int64_t ce = std::min(cb + R.chunk_cap, sg.e);
        if (R.split && cb < sg.sb) ce = std::min(ce, sg.sb);
        else if (R.split && cb < sg.se) ce = std::min(ce, sg.se);
        ChunkEnd end = ChunkEnd::kOpen;
        if (int rc = run_chunk(R, sg, cb, ce, &end)) return rc;
        if (end == ChunkEnd::kResplit) R.split = true;
        const bool again = end == ChunkEnd::kResplit || end == ChunkEnd::kRedoOverflow || end == ChunkEnd::kRedoHint;
        if (!again) cb = ce;
      }
    }
  }
  if (jp.exceed && (mode == kFull || mode == kCount)) jp.exceed->perms += R.g.K;   // (every chunk above was counted once)
  return finish_join(R);
}

}  // namespace

int gcre_host::join_once(gcre_ctx* c, const JoinPlan& jp, gcre_result* out) { return run_join(c, jp, out); }

// GCRE_INSPECT_CACHE=0: every join inspects, whatever the caller asked for (cross-check)
bool gcre_host::inspect_cache_allowed() {
  static const bool off = std::getenv("GCRE_INSPECT_CACHE") && std::atoi(std::getenv("GCRE_INSPECT_CACHE")) == 0;
  return !off;
}

void gcre_host::start_table_prefetch(gcre_ctx* c, gcre_uids* u, int64_t P, int window) {
  u->prefetch.reset(new gcre_uids::Prefetch());
  gcre_uids::Prefetch* pf = u->prefetch.get();
  pf->first = 0; pf->count = P; pf->score_b = 0; pf->score_e = P; pf->plane_b = 0; pf->plane_e = P;
  const int nkt = (window + kSparseTile - 1) / kSparseTile;
  const bool with_quads = c->g.method == 1 && c->ie_quad && c->d_ladder;
  const gcre_ctx* cc = c;
  pf->th = std::thread([u, pf, P, nkt, with_quads, cc]() {
    HostTimer hb("prefetched tables: build (helper thread)");
    build_segments_host(*u, 0, P, 0, P, 0, P, pf->segs, &pf->nscored);
    pf->ready = true;
    if (with_quads && (int64_t)pf->segs.size() < ((int64_t)1 << 30)) {
      pf->q_warm = warm_segments(cc, pf->nscored, nkt);
      build_quads_host(*u, pf->segs, 0, pf->nscored, pf->q_warm, pf->quads, &pf->quad_begin);
      pf->quads_ready = true;
    }
  });
}

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

int gcre_abi_version(void) { return GCRE_ABI_VERSION; }
#ifndef GCRE_BUILD_FLAGS
#define GCRE_BUILD_FLAGS ""
#endif
const char* gcre_build_flags(void) { return GCRE_BUILD_FLAGS; }
int gcre_device_count(void) {
  int n = 0;
  return (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? n : 0;
}

const char* gcre_last_error(const gcre_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

gcre_ctx* gcre_create(int method, int n_cases, int n_ctrls, int iterations, int device) {
  // check_true(num_cases > 0 && num_ctrls > 0 && iters >= 0), join_base.cpp:47
  if ((method != 1 && method != 2) || n_cases <= 0 || n_ctrls <= 0 || iterations < 0) {
    g_create_error = "assertion: need method in {1,2}, num_cases > 0, num_ctrls > 0, iterations >= 0";
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_create_error = "no HIP device: libgcre_hip has no CPU fallback";
    return nullptr;
  }
  if (device < 0 || device >= ndev) {
    g_create_error = "device index out of range";
    return nullptr;
  }
  hipDeviceProp_t prop;
  if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
    g_create_error = "cannot select HIP device";
    return nullptr;
  }
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    g_create_error = std::string("kernels are built for gfx950 only, device is ") + prop.gcnArchName;
    return nullptr;
  }
  auto* c = new gcre_ctx();
  c->device = device;
  (void)hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device);
  Geometry& g = c->g;
  g.method = method;
  g.n = n_cases + n_ctrls;
  g.n_cases = n_cases;
  g.W = (g.n + 63) / 64;
  g.Wp = ((g.W + 3) / 4) * 4;
  g.S = g.Wp * method;
  g.K = iterations;
  g.Kpad = ((iterations + kPermTileMax - 1) / kPermTileMax) * kPermTileMax;
  g.TD = 64 * g.Wp + 1;
  c->win_k0 = 0;
  c->win_K = g.K;
  if (const char* e = std::getenv("GCRE_QUIET")) c->quiet = std::atoi(e) != 0;
  g_launch_trace = std::getenv("GCRE_LAUNCH_TRACE") != nullptr;   // (tests: which launches went past their grid caps)
  if (const char* e = std::getenv("GCRE_CHUNK_PATHS")) c->chunk_paths = std::max<long long>(64, std::atoll(e));
  if (const char* e = std::getenv("GCRE_NULL_BLOCKS_PER_CU")) c->null_blocks_per_cu = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("GCRE_NULL_KERNEL"))
    c->null_kernel = !std::strcmp(e, "dense") ? 1 : !std::strcmp(e, "sparse") ? 2 : !std::strcmp(e, "ie") ? 3 : 0;
  if (const char* e = std::getenv("GCRE_IE_PRUNE")) c->ie_prune = std::atoi(e) != 0;
  if (const char* e = std::getenv("GCRE_EXCHANGE_TAIL")) c->exchange_tail = std::min(std::max(std::atoi(e), -1), 64);
  if (const char* e = std::getenv("GCRE_IE_WARM")) c->ie_warm_segs = std::min(std::max(std::atoi(e), 0), 1 << 20);
  if (const char* e = std::getenv("GCRE_IE_WARM_ITEMS")) c->ie_warm_items = std::min(std::max(std::atoi(e), 1), 64);
  if (const char* e = std::getenv("GCRE_IE_WARM_DIV")) c->ie_warm_div = std::min(std::max(std::atoi(e), 1), 1 << 30);
  if (const char* e = std::getenv("GCRE_IE_WARM_CAP_DIV")) c->ie_warm_cap_div = std::min(std::max(std::atoi(e), 1), 1 << 30);
  if (const char* e = std::getenv("GCRE_IE_SJT")) c->ie_small_join_tiles = std::atoi(e);
  if (const char* e = std::getenv("GCRE_IE_BATCH")) c->ie_batch = std::min(std::max(std::atoi(e), 1), 4096);
  if (const char* e = std::getenv("GCRE_IEQ_BATCH")) c->ieq_batch = std::max(0, std::atoi(e));
  if (const char* e = std::getenv("GCRE_IE_QUAD")) c->ie_quad = std::min(std::max(std::atoi(e), 0), 2);   // 2: wherever it can run
  if (const char* e = std::getenv("GCRE_IE_FLAGQ")) c->ie_flagq = std::atoi(e) != 0;
  if (const char* e = std::getenv("GCRE_IE_ZWIDE")) c->ie_zwide = std::atoi(e) != 0;
  if (const char* e = std::getenv("GCRE_STATS_IE_COUNTS")) c->stats_ie_counts = std::atoi(e) != 0;
  if (const char* e = std::getenv("GCRE_PLANES_OUT_MAX_MB")) c->planes_out_max = (size_t)std::max(0ll, std::atoll(e)) << 20;
  if (const char* e = std::getenv("GCRE_SPARSE_WAVES_PER_CU")) c->sparse_waves_per_cu = std::max(1, std::atoi(e));

  bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipStreamCreateWithFlags(&c->sel_stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipStreamCreateWithFlags(&c->insp_stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipStreamCreateWithFlags(&c->rec_stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->ev_rec_in, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->ev_rec_done, hipEventDisableTiming) == hipSuccess;
  if (const char* e = std::getenv("GCRE_REC_STREAM")) c->rec_async = std::atoi(e) != 0;
  ok = ok && hipEventCreateWithFlags(&c->ev_insp_done, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->ev_insp_main, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->ev_tail, hipEventDisableTiming) == hipSuccess;
  if (const char* e = std::getenv("GCRE_AHEAD")) c->ahead_on = std::atoi(e) != 0;
  ok = ok && hipEventCreateWithFlags(&c->ev_sel, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->ev_sel_done, hipEventDisableTiming) == hipSuccess;
  if (const char* e = std::getenv("GCRE_SELECT_STREAM")) c->sel_async = std::atoi(e) != 0;
  if (const char* e = std::getenv("GCRE_SELECT_DEFER")) c->sel_defer = std::atoi(e) != 0;
  if (const char* e = std::getenv("GCRE_SELECT_CAND")) c->sel_cand = std::min(std::max(std::atoi(e), 0), 1 << 24);
  if (const char* e = std::getenv("GCRE_SELECT_PASSES"))
    if (std::atoi(e) == 8) c->sel_cand = 0;
  ok = ok && hipMalloc((void**)&c->d_case_mask, (size_t)g.Wp * 8) == hipSuccess;
  ok = ok && hipMalloc((void**)&c->d_max_tot, kFlagWords * 4) == hipSuccess;
  ok = ok && hipMalloc((void**)&c->d_max_tot_b, kFlagWords * 4) == hipSuccess;
  ok = ok && hipMalloc((void**)&c->d_queue, 8 * 16 * 4) == hipSuccess;
  if (ok && g.Kpad > 0) {
    ok = hipMalloc((void**)&c->d_masks, (size_t)2 * g.Wp * g.Kpad * 4) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->d_null, (size_t)g.Kpad * 4) == hipSuccess;
    ok = ok && hipMemsetAsync(c->d_masks, 0, (size_t)2 * g.Wp * g.Kpad * 4, c->stream) == hipSuccess;
  }
  if (ok) {
    // cases are patient columns 0..n_cases-1, join_base.cpp:50-54
    std::vector<uint64_t> cm((size_t)g.Wp, 0);
    for (int k = 0; k < n_cases; k++) cm[(size_t)k / 64] |= uint64_t(1) << (k % 64);
    ok = hipMemcpy(c->d_case_mask, cm.data(), cm.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) {
    g_create_error = "device allocation failed in gcre_create";
    gcre_destroy(c);
    return nullptr;
  }
  return c;
}

void gcre_destroy(gcre_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->insp_stream) (void)hipStreamSynchronize(c->insp_stream);
  if (c->rec_stream) (void)hipStreamSynchronize(c->rec_stream);
  drop_ahead(c);
  // path sets and join indices the caller did not free: their rows, lists, count planes, recipes and segment tables go
  // with the context (their handles are invalid from here on, include/gcre_hip.h)
  while (!c->live_uids.empty()) free_uids(c->live_uids.back());
  while (!c->live_tallies.empty()) gcre_gene_tally_free(c->live_tallies.back());
  while (!c->live_exceeds.empty()) gcre_exceed_free(c->live_exceeds.back());
  while (!c->live_hits.empty()) gcre_hits_free(c->live_hits.back());
  {
    std::vector<const gcre_pathset*> sets;
    for (const auto& kv : c->live_sets) sets.push_back(kv.second);
    for (const gcre_pathset* ps : sets) gcre_pathset_free(const_cast<gcre_pathset*>(ps));
  }
  for (void* p : {(void*)c->d_case_mask, (void*)c->d_masks, (void*)c->d_t32, (void*)c->d_dvt, (void*)c->d_dmax, (void*)c->d_dmaxn,
                  (void*)c->d_null, (void*)c->d_mt, (void*)c->d_max_tot, (void*)c->d_max_tot_b, (void*)c->d_queue, (void*)c->d_ladder})
    if (p) (void)hipFree(p);
  c->scratch.release();
  for (auto* b : {&c->d_sel, &c->d_small, &c->d_chunk, &c->d_rec_segs}) b->release();
  c->d_hub_null.release();
  c->d_wkey.release();
  c->d_cand.release();
  c->d_doff.release();
  c->d_scan.release();
  c->d_excess.release();
  c->d_excess_b.release();
  c->d_ie_timing.release();
  for (auto& pb : c->plane_pool) (void)hipFree(pb.p);
  c->plane_pool.clear();
  for (auto e : c->ev_pool) (void)hipEventDestroy(e);
  if (c->sel_stream) (void)hipStreamSynchronize(c->sel_stream);
  if (c->sel_stream) (void)hipStreamDestroy(c->sel_stream);
  if (c->insp_stream) (void)hipStreamDestroy(c->insp_stream);
  if (c->rec_stream) (void)hipStreamSynchronize(c->rec_stream);
  if (c->rec_stream) (void)hipStreamDestroy(c->rec_stream);
  if (c->ev_rec_in) (void)hipEventDestroy(c->ev_rec_in);
  if (c->ev_rec_done) (void)hipEventDestroy(c->ev_rec_done);
  if (c->ev_insp_done) (void)hipEventDestroy(c->ev_insp_done);
  if (c->ev_insp_main) (void)hipEventDestroy(c->ev_insp_main);
  if (c->ev_tail) (void)hipEventDestroy(c->ev_tail);
  if (c->ev_sel) (void)hipEventDestroy(c->ev_sel);
  if (c->ev_sel_done) (void)hipEventDestroy(c->ev_sel_done);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int gcre_set_top_k(gcre_ctx* c, int top_k) {
  if (!c) return GCRE_ERR_ARG;
  if (top_k < 1) return fail(c, GCRE_ERR_ARG, "top_k must be >= 1");
  c->top_k = top_k;
  return GCRE_OK;
}

int gcre_width_ul(const gcre_ctx* c) { return c ? c->g.W : GCRE_ERR_ARG; }
int gcre_vlen(const gcre_ctx* c) { return c ? c->g.W * c->g.method : GCRE_ERR_ARG; }

int gcre_set_value_table(gcre_ctx* c, const double* table, int nrow, int ncol, int col_major) {
  HostTimer ht("set_value_table");
  if (!c || (!table && nrow > 0 && ncol > 0) || nrow < 0 || ncol < 0) return fail(c, GCRE_ERR_ARG, "bad value table");
  (void)hipSetDevice(c->device);
  const Geometry& g = c->g;
  const int n = g.n;
  // the reference pads the table to (n+1)x(n+1) with -1 (join_base.cpp:67-78); the device keeps it diagonal-major
  // (and covers carrier counts up to the padded word width with -1).  The repacking runs on the device: the raw table
  // goes up as it is (k_table_to_diag, gcre_frontend.hip) -- on the host it is 10 s of cache misses at 50,000 patients.
  const size_t TD = (size_t)g.TD, NT = tri(TD);
  const bool was_asym = c->d_dmaxn != nullptr;
  for (void** p : {(void**)&c->d_dvt, (void**)&c->d_t32, (void**)&c->d_dmax, (void**)&c->d_dmaxn})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  double* d_raw = nullptr;
  uint32_t* d_asym = nullptr;
  const size_t raw = (size_t)nrow * (size_t)ncol;
  HIP_TRY(c, hipMalloc((void**)&c->d_dvt, NT * 8));
  if (g.method == 1) HIP_TRY(c, hipMalloc((void**)&c->d_t32, NT * 4));
  else HIP_TRY(c, hipMalloc((void**)&c->d_dmax, NT * 8));
  HIP_TRY(c, hipMalloc((void**)&d_raw, std::max<size_t>(raw, 1) * 8));
  hipError_t e = hipSuccess;
  if (g.method == 2) {
    e = hipMalloc((void**)&d_asym, sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemsetAsync(d_asym, 0, sizeof(uint32_t), c->stream);
  }
  if (e == hipSuccess && raw) e = hipMemcpyAsync(d_raw, table, raw * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = launch_table_to_diag(d_raw, nrow, ncol, col_major, n, (int)TD, c->d_dvt, c->d_t32, c->d_dmax, d_asym, c->stream);
  if (e == hipSuccess && TD <= 65536) {   // counts fit the 16-bit bounds of a ladder entry
    if (!c->d_ladder) e = hipMalloc((void**)&c->d_ladder, (size_t)(kLadder2Levels + 2) * TD * 4);
    if (e == hipSuccess)
      e = g.method == 1 ? launch_build_ladder(c->d_t32, (int)TD, c->d_ladder, c->stream)
                        : launch_build_ladder2(c->d_dmax, (int)TD, c->d_ladder, c->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d_raw);
  if (e == hipSuccess && g.method == 2) {
    // vtmax[r][c] != vtmax[c][r] somewhere (std::max and a NaN on one side of the diagonal): the (-) half of a path, which
    // reads vtmax[tn - b][b] at index b of its diagonal, gets the mirror image of the table
    uint32_t asym = 0;
    e = hipMemcpy(&asym, d_asym, sizeof asym, hipMemcpyDeviceToHost);
    if (e == hipSuccess && asym) {
      e = hipMalloc((void**)&c->d_dmaxn, NT * 8);
      if (e == hipSuccess) e = launch_mirror_diag(c->d_dmax, (int)TD, c->d_dmaxn, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
  }
  if (d_asym) (void)hipFree(d_asym);
  c->g00_rows = 0xffffffffu;
  if (e == hipSuccess && g.method == 2) {
    // what an empty half adds to a path's null score: vtmax[0][0], as the device table holds it, rounded UP to ladder rows
    double g00 = 0;
    e = hipMemcpy(&g00, c->d_dmax, 8, hipMemcpyDeviceToHost);
    if (!(g00 != g00)) {
      const double x = g00 > 0 ? std::ceil(g00 * (double)(2 * kLadderPerUnit)) : 0.0;   // (times 16: exact)
      if (x < 1e9) c->g00_rows = (uint32_t)x;
    }
  }
  if (e != hipSuccess) return fail(c, GCRE_ERR_DEVICE, std::string("set_value_table: ") + hipGetErrorString(e));
  c->have_table = true;
  c->obs_epoch++;
  if (c->d_dmaxn && !was_asym && !c->quiet)
    std::fprintf(stderr, "[table] vtmax is not symmetric (a NaN on one side of the diagonal only): permutations are scored by "
                         "the dense kernel, without pruning\n");
  // the masks changed while such a table kept the count-plane kernels off: their transposed copy is due now (the epoch
  // was bumped when they changed, the window is the caller's and stays)
  if (c->have_perms && c->mt_stale && sparse_enabled(c))
    if (int rc = transpose_masks(c)) return rc;
  return GCRE_OK;
}

int gcre_set_inspect_cache(gcre_ctx* c, int on) {
  if (!c) return GCRE_ERR_ARG;
  c->insp_cache = on != 0 && inspect_cache_allowed();
  if (!c->insp_cache) return gcre_drop_inspections(c, 1);
  return GCRE_OK;
}

int gcre_drop_inspections(gcre_ctx* c, int release_memory) {
  if (!c) return GCRE_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (release_memory && c->stream) (void)hipStreamSynchronize(c->stream);
  drop_ahead(c);
  for (gcre_uids* u : c->live_uids) {
    drop_launch(u);
    u->insp_valid = false;
    if (release_memory) {
      for (auto& ci : u->insp) ci.release();
      u->insp.clear();
    }
  }
  return GCRE_OK;
}

int gcre_set_perm_cases(gcre_ctx* c, const int32_t* perms, int nrow, int ncol, int col_major) {
  if (!c || nrow < 0 || ncol < 0) return fail(c, GCRE_ERR_ARG, "bad permutation matrix");
  (void)hipSetDevice(c->device);
  const Geometry& g = c->g;
  if (g.K == 0) { c->have_perms = true; return GCRE_OK; }
  // too few rows are reused cyclically (join_base.cpp:116-123) -- with zero rows the reference divides by zero
  if (nrow == 0 || !perms) return fail(c, GCRE_ERR_ASSERT, "assertion: iterations > 0 but no permuted cases");
  if (ncol != g.n) return fail(c, GCRE_ERR_ASSERT, "assertion: permuted cases must have num_cases + num_ctrls columns");
  if (nrow > g.K && !c->quiet) std::printf("  ** WARN more permuted cases than iterations, input will be truncated\n");   // :89-90
  if (nrow < g.K && !c->quiet)
    std::printf("  ** WARN not enough permuted cases, some will be reused to match iterations - hope this is for testing!\n");
  const int used = std::min(nrow, g.K);
  static const bool device_pack = std::getenv("GCRE_DEVICE_PACK") && std::atoi(std::getenv("GCRE_DEVICE_PACK")) != 0;
  if (!device_pack) {
    // setPermutedCases (join_base.cpp:85-125) on the host: mask_r = case_mask XOR flipped_r, flipped where the input is
    // not 1 (:103-104); cases are the first n_cases columns (:50-54).  Only the rows that are used are packed (a column-major
    // matrix keeps its row stride); the packed masks take the road of gcre_set_perm_masks (row reuse included).
    HostTimer hp("pack permutations (host)");
    std::vector<uint64_t> packed((size_t)used * g.W, 0);
    const int n_cases = g.n_cases;
    if (col_major) {
      // columns of the full matrix are nrow long: pack all of its rows column block by column block, keep the first `used`
      if (used == nrow) {
        pack_bits_host(perms, nrow, ncol, true, packed.data(), (size_t)g.W, [n_cases](int32_t v, int q) { return (v != 1) != (q < n_cases); });
      } else {
        std::vector<uint64_t> all((size_t)nrow * g.W, 0);
        pack_bits_host(perms, nrow, ncol, true, all.data(), (size_t)g.W, [n_cases](int32_t v, int q) { return (v != 1) != (q < n_cases); });
        std::memcpy(packed.data(), all.data(), packed.size() * 8);
      }
    } else {
      pack_bits_host(perms, used, ncol, false, packed.data(), (size_t)g.W, [n_cases](int32_t v, int q) { return (v != 1) != (q < n_cases); });
    }
    uint64_t* d_in = nullptr;
    HIP_TRY(c, hipMalloc((void**)&d_in, packed.size() * 8));
    hipError_t e = hipMemcpyAsync(d_in, packed.data(), packed.size() * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_masks_from_words(d_in, used, g, c->d_masks, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_in);
    if (e != hipSuccess) return fail(c, GCRE_ERR_DEVICE, std::string("set_perm_cases: ") + hipGetErrorString(e));
    if (int rc = build_transposed_masks(c)) return rc;
    c->have_perms = true;
    return GCRE_OK;
  }
  std::vector<int32_t> rows;
  const int32_t* src = perms;   // row-major: the first `used` rows are contiguous
  if (col_major) {              // R matrix: gather the rows we need
    rows.resize((size_t)used * ncol);
    for (int r = 0; r < used; r++)
      for (int q = 0; q < ncol; q++) rows[(size_t)r * ncol + q] = perms[(size_t)q * nrow + r];
    src = rows.data();
  }
  int32_t* d_in = nullptr;
  const size_t bytes = (size_t)used * ncol * 4;
  HIP_TRY(c, hipMalloc((void**)&d_in, bytes));
  hipError_t e = hipMemcpyAsync(d_in, src, bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = launch_masks_from_ints(d_in, used, ncol, 0, g, c->d_masks, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d_in);
  if (e != hipSuccess) return fail(c, GCRE_ERR_DEVICE, std::string("set_perm_cases: ") + hipGetErrorString(e));
  if (int rc = build_transposed_masks(c)) return rc;
  c->have_perms = true;
  return GCRE_OK;
}

int gcre_set_perm_masks(gcre_ctx* c, const uint64_t* masks, int nrow) {
  if (!c || nrow < 0) return fail(c, GCRE_ERR_ARG, "bad mask matrix");
  (void)hipSetDevice(c->device);
  const Geometry& g = c->g;
  if (g.K == 0) { c->have_perms = true; return GCRE_OK; }
  if (nrow == 0 || !masks) return fail(c, GCRE_ERR_ASSERT, "assertion: iterations > 0 but no permuted cases");
  const int used = std::min(nrow, g.K);
  uint64_t* d_in = nullptr;
  HIP_TRY(c, hipMalloc((void**)&d_in, (size_t)used * g.W * 8));
  hipError_t e = hipMemcpyAsync(d_in, masks, (size_t)used * g.W * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = launch_masks_from_words(d_in, used, g, c->d_masks, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d_in);
  if (e != hipSuccess) return fail(c, GCRE_ERR_DEVICE, std::string("set_perm_masks: ") + hipGetErrorString(e));
  if (int rc = build_transposed_masks(c)) return rc;
  c->have_perms = true;
  return GCRE_OK;
}

int gcre_set_perm_window(gcre_ctx* c, int k0, int k1) {
  if (!c) return GCRE_ERR_ARG;
  const int K = c->g.K;
  if (k0 < 0 || k1 < k0 || k1 > K || (k0 % kSparseTile) != 0 || (k1 != K && (k1 % kSparseTile) != 0))
    return fail(c, GCRE_ERR_ARG, "permutation window must be tile-aligned (2048) and inside [0, iterations]");
  if (k0 != c->win_k0 || k1 - k0 != c->win_K) {
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->win_k0 = k0;
    c->win_K = k1 - k0;
    c->mask_epoch++;   // count planes hold the tiles of one window
  }
  c->win_K_nominal = std::max(c->win_K_nominal, k1 - k0);
  return GCRE_OK;
}

int gcre_plan_perm_window(gcre_ctx* c, const int64_t* set_rows, int n_sets) {
  if (!c || n_sets < 0 || (n_sets > 0 && !set_rows)) return GCRE_ERR_ARG;
  const int K = c->g.K;
  const int nkt = (K + kSparseTile - 1) / kSparseTile;
  if (nkt <= 1 || !sparse_enabled(c)) return K;
  (void)hipSetDevice(c->device);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return K;
  // sets that store their planes: the ones under the recipe limit (larger kept sets leave a recipe instead, and operands
  // that are not kept are small)
  double rows = 1;
  for (int i = 0; i < n_sets; i++) {
    const double full = (double)std::max<int64_t>(set_rows[i], 0) * c->g.method * 4096.0 * nkt;
    if (full <= (double)c->planes_out_max) rows += (double)std::max<int64_t>(set_rows[i], 0);
  }
  const double per_tile = rows * c->g.method * 4096.0;
  int64_t tiles = (int64_t)((double)free_b * 0.5 / per_tile);
  if (const char* e = std::getenv("GCRE_WINDOW_TILES")) tiles = std::max(1, std::atoi(e));   // tests
  if (tiles >= nkt) return K;
  return (int)std::max<int64_t>(tiles, 1) * kSparseTile;
}

int gcre_get_perm_mask(gcre_ctx* c, int r, uint64_t* out) {
  if (!c || !out) return GCRE_ERR_ARG;
  const Geometry& g = c->g;
  if (r < 0 || r >= g.K) return fail(c, GCRE_ERR_RANGE, "permutation index out of range");
  (void)hipSetDevice(c->device);
  std::vector<uint32_t> col((size_t)2 * g.Wp);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy2D(col.data(), 4, c->d_masks + r, (size_t)g.Kpad * 4, 4, (size_t)2 * g.Wp, hipMemcpyDeviceToHost));
  for (int k = 0; k < g.W; k++) out[k] = (uint64_t)col[(size_t)2 * k] | ((uint64_t)col[(size_t)2 * k + 1] << 32);
  return GCRE_OK;
}

// ---- tests: one helper kernel of a join on inputs given from the host ----
int gcre_test_range_union(gcre_ctx* c, const uint64_t* p1, int64_t n1, const uint64_t* pz, int64_t nz, const int32_t* zindex,
                          const int64_t* loc, const int32_t* cnt, int64_t n_ranges, int S, int Wp, int method, uint64_t* u_out,
                          uint32_t* bad_out, int32_t* piece_rows_out) {
  if (!c) return GCRE_ERR_ARG;
  if (piece_rows_out) *piece_rows_out = kRangePieceRows;
  if (n_ranges == 0) return GCRE_OK;
  if (!p1 || !pz || !zindex || !loc || !cnt || !u_out || !bad_out || n_ranges < 0 || Wp <= 0 || Wp % 4 || (method != 1 && method != 2) ||
      S != method * Wp)
    return fail(c, GCRE_ERR_ARG, "gcre_test_range_union: bad arguments");
  for (int64_t r = 0; r < n_ranges; r++) {
    if (cnt[r] <= 0 || loc[r] < 0 || loc[r] + cnt[r] > n1) return fail(c, GCRE_ERR_RANGE, "gcre_test_range_union: range outside paths1");
    for (int64_t l = loc[r]; l < loc[r] + cnt[r]; l++)
      if ((int64_t)(zindex[l] & 0x7fffffff) >= nz) return fail(c, GCRE_ERR_RANGE, "gcre_test_range_union: reduced row out of range");
  }
  (void)hipSetDevice(c->device);
  std::vector<RangePiece> pieces;
  std::vector<int32_t> cut;
  build_range_pieces(std::vector<int64_t>(loc, loc + n_ranges), std::vector<int32_t>(cnt, cnt + n_ranges), pieces, cut);
  DevBuf<uint64_t> d1, dz, du;
  DevBuf<int32_t> dzi, dcut;
  DevBuf<RangePiece> dp;
  DevBuf<uint32_t> dbad;
  hipStream_t st = c->stream;
  const size_t uw = (size_t)n_ranges * S;
  hipError_t e = d1.upload(p1, (size_t)n1 * S, st);
  if (e == hipSuccess) e = dz.upload(pz, (size_t)nz * S, st);
  if (e == hipSuccess) e = dzi.upload(zindex, (size_t)n1, st);
  if (e == hipSuccess) e = dp.upload(pieces.data(), pieces.size(), st);
  if (e == hipSuccess) e = dcut.upload(cut.data(), cut.size(), st);
  if (e == hipSuccess) e = du.reserve(uw);
  if (e == hipSuccess) e = dbad.reserve(1);
  if (e == hipSuccess) e = hipMemsetAsync(du.p, 0xa5, uw * 8, st);   // the kernel must not count on a zeroed table
  if (e == hipSuccess) e = hipMemsetAsync(dbad.p, 0, 4, st);
  if (e == hipSuccess)
    e = launch_range_union(d1.p, dz.p, dzi.p, dp.p, (int64_t)pieces.size(), dcut.p, (int64_t)cut.size(), S, Wp, method, du.p, dbad.p, st);
  if (e == hipSuccess) e = hipMemcpyAsync(u_out, du.p, uw * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(bad_out, dbad.p, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  for (void* p : {(void*)d1.p, (void*)dz.p, (void*)du.p, (void*)dzi.p, (void*)dcut.p, (void*)dp.p, (void*)dbad.p})
    if (p) (void)hipFree(p);
  if (e != hipSuccess) return fail(c, GCRE_ERR_DEVICE, std::string("gcre_test_range_union: ") + hipGetErrorString(e));
  return GCRE_OK;
}

int gcre_test_expand(gcre_ctx* c, const int64_t* path_idx, const int64_t* location, int64_t n_uids, const int32_t* signs,
                     int64_t n_signs, int path_length, int method, int64_t first, int64_t count, uint32_t* row0, uint32_t* row1) {
  if (!c) return GCRE_ERR_ARG;
  if (count == 0) return GCRE_OK;
  if (!path_idx || !location || !row0 || !row1 || n_uids <= 0 || first < 0 || count < 0 || n_signs < 0 || (n_signs && !signs) ||
      (method != 1 && method != 2))
    return fail(c, GCRE_ERR_ARG, "gcre_test_expand: bad arguments");
  if (path_idx[0] != 0 || first + count > path_idx[n_uids]) return fail(c, GCRE_ERR_RANGE, "gcre_test_expand: ordinals outside the index");
  for (int64_t i = 0; i < n_uids; i++) {
    const int64_t n = path_idx[i + 1] - path_idx[i];
    if (n < 0 || (n > 0 && location[i] < 0)) return fail(c, GCRE_ERR_RANGE, "gcre_test_expand: bad index");
    // the signs a uid with paths is looked up by (begin_join makes the same demand of a join's index)
    const int64_t need = n == 0 || method != 2 ? 0 : path_length > 3 ? i + 1 : path_length < 3 ? location[i] + n
                                                                                                : std::max(i + 1, location[i] + n);
    if (n_signs < need) return fail(c, GCRE_ERR_RANGE, "gcre_test_expand: signs vector shorter than the rows it is indexed by");
  }
  (void)hipSetDevice(c->device);
  DevBuf<int64_t> dpi, dloc;
  DevBuf<int32_t> dsg;
  DevBuf<uint32_t> d0, d1;
  hipStream_t st = c->stream;
  hipError_t e = dpi.upload(path_idx, (size_t)n_uids + 1, st);
  if (e == hipSuccess) e = dloc.upload(location, (size_t)n_uids, st);
  if (e == hipSuccess) e = dsg.upload(signs, (size_t)n_signs, st);
  if (e == hipSuccess) e = d0.reserve((size_t)count);
  if (e == hipSuccess) e = d1.reserve((size_t)count);
  if (e == hipSuccess) e = launch_expand(dpi.p, dloc.p, n_uids, dsg.p, path_length, method, first, count, d0.p, d1.p, st);
  if (e == hipSuccess) e = hipMemcpyAsync(row0, d0.p, (size_t)count * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(row1, d1.p, (size_t)count * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  for (void* p : {(void*)dpi.p, (void*)dloc.p, (void*)dsg.p, (void*)d0.p, (void*)d1.p})
    if (p) (void)hipFree(p);
  if (e != hipSuccess) return fail(c, GCRE_ERR_DEVICE, std::string("gcre_test_expand: ") + hipGetErrorString(e));
  return GCRE_OK;
}

// The method-1 inspector (launch_stats_ie) on given row numbers: path i joins row row0[i] of `p0` to row row1[i] of `red`, or,
// with `zindex`, to row zindex[row1[i]] of it (a hinted join: then excess[n_ranges][W], rows as the host packs them, and range_of[rows of p0]
// are its range table).  The counts come from the row totals of `red` where the context's knob and the join's size say so (row_counts_for).
// Out, per path: tot, cases, ctrls, rowz, linfo, key, and the list's entries (padding included) in entries[i * ent_stride ..),
// the slot's eight followed by the overflow part found through lover; res_out (optional): the kept rows; flags: the flag block.
int gcre_test_inspect(gcre_ctx* c, const gcre_pathset* p0, const gcre_pathset* red, const uint32_t* row0, const uint32_t* row1,
                      int64_t count, const int32_t* zindex, int64_t n_zindex, const uint64_t* excess, const int32_t* range_of,
                      int64_t n_ranges, int64_t over_entries, uint32_t* tot, uint32_t* cases, uint32_t* ctrls, uint32_t* rowz,
                      uint32_t* linfo, uint64_t* key, uint32_t* entries, int64_t ent_stride, uint64_t* res_out, uint32_t* flags) {
  if (!c) return GCRE_ERR_ARG;
  const Geometry& g = c->g;
  if (!p0 || !red || p0->ctx != c || red->ctx != c || !row0 || !row1 || count <= 0 || count > (1 << 24) || over_entries < 0 ||
      !tot || !cases || !ctrls || !rowz || !linfo || !key || !entries || ent_stride < 8 || !flags || (zindex && n_zindex <= 0) ||
      ((excess != nullptr) != (range_of != nullptr)) || (excess && (!zindex || n_ranges <= 0)))
    return fail(c, GCRE_ERR_ARG, "gcre_test_inspect: bad arguments");
  if (g.method != 1 || g.Wp > 160) return fail(c, GCRE_ERR_ARG, "gcre_test_inspect: the block-staged method-1 inspector only");
  if (!c->d_dvt) return fail(c, GCRE_ERR_ARG, "gcre_test_inspect: no value table");
  for (int64_t i = 0; i < count; i++) {
    if ((int64_t)row0[i] >= p0->nrows) return fail(c, GCRE_ERR_RANGE, "gcre_test_inspect: paths0 row out of range");
    if ((row1[i] >> 31) || (int64_t)row1[i] >= (zindex ? n_zindex : red->nrows))
      return fail(c, GCRE_ERR_RANGE, "gcre_test_inspect: paths1 row out of range");
    if (zindex && (zindex[row1[i]] < 0 || (int64_t)zindex[row1[i]] >= red->nrows))
      return fail(c, GCRE_ERR_RANGE, "gcre_test_inspect: reduced row out of range");
    if (range_of && (range_of[row0[i]] < 0 || (int64_t)range_of[row0[i]] >= n_ranges))
      return fail(c, GCRE_ERR_RANGE, "gcre_test_inspect: range out of range");
  }
  (void)hipSetDevice(c->device);
  hipStream_t st = c->stream;
  const size_t n = (size_t)count;
  const size_t blocks = (n + kStatsIeBlockPaths - 1) / kStatsIeBlockPaths;
  const size_t over_cap = (size_t)over_entries + (std::min<size_t>((size_t)kInspectMaxBlocks, blocks) * kInspectBlockWaves + 2) * kOverChunk + 16;
  DevBuf<uint32_t> d0, d1, dtot, dcases, dctrls, drowz, dlinfo, dlover, dslot, dover, dflags;
  DevBuf<int32_t> dzi, drng;
  DevBuf<uint64_t> dkey, dex, dres;
  std::vector<uint32_t> lover(n), slot(n * 8), over;
  hipError_t e = d0.upload(row0, n, st);
  if (e == hipSuccess) e = d1.upload(row1, n, st);
  if (e == hipSuccess && zindex) e = dzi.upload(zindex, (size_t)n_zindex, st);
  if (e == hipSuccess && excess) e = dex.reserve((size_t)n_ranges * g.S);   // rows of W words from the host, of S on the device
  if (e == hipSuccess && excess) e = hipMemsetAsync(dex.p, 0, (size_t)n_ranges * g.S * 8, st);
  if (e == hipSuccess && excess)
    e = hipMemcpy2DAsync(dex.p, (size_t)g.S * 8, excess, (size_t)g.W * 8, (size_t)g.W * 8, (size_t)n_ranges, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && excess) e = drng.upload(range_of, (size_t)p0->nrows, st);
  for (DevBuf<uint32_t>* b : {&dtot, &dcases, &dctrls, &drowz, &dlinfo, &dlover})
    if (e == hipSuccess) e = b->reserve(n);
  if (e == hipSuccess) e = dkey.reserve(n);
  if (e == hipSuccess) e = dslot.reserve(n * 8);
  if (e == hipSuccess) e = dover.reserve(over_cap);
  if (e == hipSuccess) e = dflags.reserve(kFlagWords);
  if (e == hipSuccess && res_out) e = dres.reserve(n * g.S);
  if (e == hipSuccess) e = hipMemsetAsync(dflags.p, 0, kFlagWords * 4, st);
  StatsArgs sa{};
  int rc = GCRE_OK;
  if (e == hipSuccess) {
    sa.p0 = p0->d_rows;
    sa.p1 = red->d_rows;
    sa.pz = red->d_rows;
    sa.row0 = d0.p;
    sa.row1 = d1.p;
    sa.case_mask = c->d_case_mask;
    sa.dvt = c->d_dvt;
    sa.key = dkey.p;
    sa.tot = dtot.p;
    sa.cases = dcases.p;
    sa.ctrls = dctrls.p;
    sa.res = res_out ? dres.p : nullptr;
    sa.max_tot = dflags.p;
    sa.zindex = zindex ? dzi.p : nullptr;
    sa.excess = excess ? dex.p : nullptr;
    sa.range_of = excess ? drng.p : nullptr;
    sa.rowz = drowz.p;
    sa.bad = dflags.p + kFlagHintBroken;
    sa.ie_bias = 8;
    sa.ie_rule = 1;
    sa.linfo = dlinfo.p;
    sa.lover = dlover.p;
    sa.slot = dslot.p;
    sa.over = dover.p;
    sa.over_cap = (uint32_t)std::min<size_t>(over_cap - 16, 0xfffffff0u);
    sa.ov_count = dflags.p + kFlagOverReserved;
    sa.zoff = (uint32_t)(64 * g.Wp) << 8;
    sa.first = 0;
    sa.count = count;
    sa.S = g.S;
    sa.Wp = g.Wp;
    rc = row_counts_for(c, red, count, st, &sa.z_counts);
  }
  if (rc == GCRE_OK) {
    if (e == hipSuccess) e = launch_stats_ie(sa, 1, st);
    for (auto pr : {std::make_pair(tot, dtot.p), std::make_pair(cases, dcases.p), std::make_pair(ctrls, dctrls.p),
                    std::make_pair(rowz, drowz.p), std::make_pair(linfo, dlinfo.p), std::make_pair(lover.data(), dlover.p)})
      if (e == hipSuccess) e = hipMemcpyAsync(pr.first, pr.second, n * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(key, dkey.p, n * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(slot.data(), dslot.p, n * 32, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(flags, dflags.p, kFlagWords * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && res_out)
      e = hipMemcpy2DAsync(res_out, (size_t)g.W * 8, dres.p, (size_t)g.S * 8, (size_t)g.W * 8, n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && flags[kFlagOverReserved] > sa.over_cap) rc = fail(c, GCRE_ERR_RANGE, "gcre_test_inspect: the lists need more overflow entries than given");
    if (e == hipSuccess && rc == GCRE_OK && flags[kFlagOverReserved]) {
      over.resize(flags[kFlagOverReserved]);
      e = hipMemcpy(over.data(), dover.p, over.size() * 4, hipMemcpyDeviceToHost);
    }
  }
  for (void* p : {(void*)d0.p, (void*)d1.p, (void*)dtot.p, (void*)dcases.p, (void*)dctrls.p, (void*)drowz.p, (void*)dlinfo.p,
                  (void*)dlover.p, (void*)dslot.p, (void*)dover.p, (void*)dflags.p, (void*)dzi.p, (void*)drng.p, (void*)dkey.p,
                  (void*)dex.p, (void*)dres.p})
    if (p) (void)hipFree(p);
  if (rc != GCRE_OK) return rc;
  if (e != hipSuccess) return fail(c, GCRE_ERR_DEVICE, std::string("gcre_test_inspect: ") + hipGetErrorString(e));
  for (size_t i = 0; i < n; i++) {
    const uint32_t len8 = linfo_len(linfo[i]);
    if ((int64_t)len8 > ent_stride) return fail(c, GCRE_ERR_RANGE, "gcre_test_inspect: a list is longer than the room per path");
    if (len8 > 8 && (size_t)lover[i] + (len8 - 8) > over.size()) return fail(c, GCRE_ERR_DEVICE, "gcre_test_inspect: a list's overflow part lies outside the area");
    uint32_t* dst = entries + i * (size_t)ent_stride;
    std::copy(slot.begin() + (long)(i * 8), slot.begin() + (long)(i * 8 + 8), dst);
    if (len8 > 8) std::copy(over.begin() + lover[i], over.begin() + lover[i] + (len8 - 8), dst + 8);
  }
  return GCRE_OK;
}

// ---- path sets ----
gcre_pathset* gcre_pathset_zeros(gcre_ctx* c, int64_t nrows) {
  if (!c) return nullptr;
  (void)hipSetDevice(c->device);
  return new_pathset(c, nrows, true);
}

gcre_pathset* gcre_pathset_from_dense(gcre_ctx* c, const int32_t* data, int64_t nrow, int ncol, int col_major) {
  if (!c) return nullptr;
  (void)hipSetDevice(c->device);
  if (nrow < 0 || ncol < 0 || (!data && nrow > 0 && ncol > 0)) {
    fail(c, GCRE_ERR_ARG, "bad dense matrix");
    return nullptr;
  }
  // check_index(data[r].size(), width_ul*64), gcre_paths.h:63: every column must fit the mask words
  if (ncol > c->g.W * 64) {
    fail(c, GCRE_ERR_RANGE, "assertion: more data columns than mask bits");
    return nullptr;
  }
  gcre_pathset* ps = new_pathset(c, nrow, true);
  if (!ps || nrow == 0 || ncol == 0) return ps;
  hipError_t e = hipSuccess;
  static const bool device_pack = std::getenv("GCRE_DEVICE_PACK") && std::atoi(std::getenv("GCRE_DEVICE_PACK")) != 0;
  if (!device_pack) {
    // PathSet::load (gcre_paths.h:56-70) on the host: bit c of row r set iff data[r][c] != 0, (+) half only -- then the
    // packed rows go up (1/32 of the ints; GCRE_DEVICE_PACK=1: the ints go up and k_pack_dense packs them, as before round 4)
    HostTimer hp("pack genotypes (host)");
    std::vector<uint64_t> packed((size_t)nrow * c->g.S, 0);
    pack_bits_host(data, nrow, ncol, col_major != 0, packed.data(), (size_t)c->g.S, [](int32_t v, int) { return v != 0; });
    e = hipMemcpyAsync(ps->d_rows, packed.data(), packed.size() * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // `packed` is a local
  } else {
    int32_t* d_in = nullptr;
    const size_t bytes = (size_t)nrow * ncol * 4;
    e = hipMalloc((void**)&d_in, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, data, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_pack_dense(d_in, nrow, ncol, col_major, ps->d_rows, c->g.S, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (d_in) (void)hipFree(d_in);
  }
  if (e != hipSuccess) {
    fail(c, GCRE_ERR_DEVICE, std::string("pathset_from_dense: ") + hipGetErrorString(e));
    gcre_pathset_free(ps);
    return nullptr;
  }
  return ps;
}

gcre_pathset* gcre_pathset_from_words(gcre_ctx* c, const uint64_t* rows, int64_t nrows) {
  if (!c) return nullptr;
  (void)hipSetDevice(c->device);
  gcre_pathset* ps = new_pathset(c, nrows, true);
  if (!ps || nrows == 0) return ps;
  const Geometry& g = c->g;
  // host rows are [half][W]; device rows are [half][Wp]
  std::vector<uint64_t> dev((size_t)nrows * g.S, 0);
  for (int64_t r = 0; r < nrows; r++)
    for (int h = 0; h < g.method; h++)
      std::memcpy(&dev[(size_t)r * g.S + (size_t)h * g.Wp], &rows[(size_t)r * g.W * g.method + (size_t)h * g.W],
                  (size_t)g.W * 8);
  // same (non-blocking) stream as the zero-fill in new_pathset: a null-stream copy would race with it
  hipError_t e = hipMemcpyAsync(ps->d_rows, dev.data(), dev.size() * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    fail(c, GCRE_ERR_DEVICE, "pathset_from_words: copy failed");
    gcre_pathset_free(ps);
    return nullptr;
  }
  return ps;
}

gcre_pathset* gcre_pathset_select(gcre_ctx* c, const gcre_pathset* from, const int32_t* idx, int64_t n) {
  if (!c || !from || from->ctx != c || n < 0 || (!idx && n > 0)) {
    fail(c, GCRE_ERR_ARG, "bad select arguments");
    return nullptr;
  }
  (void)hipSetDevice(c->device);
  for (int64_t i = 0; i < n; i++)   // check_index(indices[k], size), gcre_paths.h:85
    if (idx[i] < 0 || idx[i] >= from->nrows) {
      fail(c, GCRE_ERR_RANGE, "assertion: select index out of range");
      return nullptr;
    }
  gcre_pathset* ps = new_pathset(c, n, false);
  if (!ps || n == 0) return ps;
  int32_t* d_idx = nullptr;
  hipError_t e = hipMalloc((void**)&d_idx, (size_t)n * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(d_idx, idx, (size_t)n * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = launch_select(from->d_rows, d_idx, n, c->g.S, ps->d_rows, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (d_idx) (void)hipFree(d_idx);
  if (e != hipSuccess) {
    fail(c, GCRE_ERR_DEVICE, std::string("pathset_select: ") + hipGetErrorString(e));
    gcre_pathset_free(ps);
    return nullptr;
  }
  return ps;
}

int64_t gcre_pathset_size(const gcre_pathset* ps) { return ps ? ps->nrows : GCRE_ERR_ARG; }

int gcre_pathset_read(gcre_ctx* c, const gcre_pathset* ps, uint64_t* out_rows) {
  if (!c || !ps || ps->ctx != c || (!out_rows && ps->nrows > 0)) return fail(c, GCRE_ERR_ARG, "bad read arguments");
  (void)hipSetDevice(c->device);
  const Geometry& g = c->g;
  if (ps->nrows == 0) return GCRE_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<uint64_t> dev((size_t)ps->nrows * g.S);
  HIP_TRY(c, hipMemcpy(dev.data(), ps->d_rows, dev.size() * 8, hipMemcpyDeviceToHost));
  for (int64_t r = 0; r < ps->nrows; r++)
    for (int h = 0; h < g.method; h++)
      std::memcpy(&out_rows[(size_t)r * g.W * g.method + (size_t)h * g.W], &dev[(size_t)r * g.S + (size_t)h * g.Wp],
                  (size_t)g.W * 8);
  return GCRE_OK;
}

void gcre_pathset_free(gcre_pathset* ps) {
  HostTimer ht("pathset_free");
  if (!ps) return;
  if (ps->ctx) {
    (void)hipSetDevice(ps->ctx->device);
    if (ps->ctx->stream) (void)hipStreamSynchronize(ps->ctx->stream);
    if (ps->ctx->insp_stream) (void)hipStreamSynchronize(ps->ctx->insp_stream);
    if (ps->ctx->rec_stream) (void)hipStreamSynchronize(ps->ctx->rec_stream);   // (the gather reads the set's recipe)
    if (ps->ctx->ahead)
      for (const JoinPlan& a : *ps->ctx->ahead)
        if (a.p0 == ps || a.p1 == ps || a.res == ps) { drop_ahead(ps->ctx); break; }
    for (gcre_uids* lu : ps->ctx->live_uids) drop_launch(lu);   // (a launched join may read or write this set)
  }
  if (ps->d_rows) (void)hipFree(ps->d_rows);
  drop_lists(ps);   // lists, and the plane buffer goes to the context's pool
  if (ps->rec) {
    ps->rec->release();
    delete ps->rec;
  }
  if (ps->ctx) ps->ctx->live_sets.erase(ps->id);
  delete ps;
}

int gcre_join(gcre_ctx* c, int path_length, const int32_t* uid_count, const int64_t* uid_location, int64_t n_uids,
              const int32_t* signs, int64_t n_signs, const gcre_pathset* paths0, const gcre_pathset* paths1,
              gcre_pathset* res, const gcre_join_opts* opts, gcre_result* out) {
  if (!c || !out || n_uids < 0 || (n_uids > 0 && (!uid_count || !uid_location)) || n_signs < 0 ||
      (n_signs > 0 && !signs))
    return fail(c, GCRE_ERR_ARG, "bad join arguments");
  (void)hipSetDevice(c->device);
  gcre_uids* u = make_uids(c, path_length, uid_count, uid_location, n_uids, signs, n_signs);
  if (!u) return c->last_code;
  JoinPlan jp{u, paths0, paths1, res, opts && opts->sharded, opts ? opts->shard_begin : 0,
              opts ? opts->shard_end : 0, opts ? opts->d_null_out : nullptr};
  jp.take(opts);
  jp.tally = c->armed_tally;
  c->armed_tally = nullptr;
  jp.exceed = c->armed_exceed;
  c->armed_exceed = nullptr;
  jp.hits = c->armed_hits;
  c->armed_hits = nullptr;
  int rc = run_join(c, jp, out);
  free_uids(u);
  if (rc != GCRE_OK) gcre_result_free(out);
  return rc;
}

gcre_uids* gcre_uids_create(gcre_ctx* c, int path_length, const int32_t* uid_count, const int64_t* uid_location,
                            int64_t n_uids, const int32_t* signs, int64_t n_signs) {
  if (!c || n_uids < 0 || (n_uids > 0 && (!uid_count || !uid_location)) || n_signs < 0 || (n_signs > 0 && !signs)) {
    fail(c, GCRE_ERR_ARG, "bad uids arguments");
    return nullptr;
  }
  (void)hipSetDevice(c->device);
  return make_uids(c, path_length, uid_count, uid_location, n_uids, signs, n_signs);
}

int64_t gcre_uids_total_paths(const gcre_uids* u) { return u ? u->total : GCRE_ERR_ARG; }

int gcre_uids_set_reduced(gcre_uids* u, const gcre_pathset* reduced, const int32_t* index, int64_t n) {
  if (!u) return GCRE_ERR_ARG;
  gcre_ctx* c = u->ctx;
  (void)hipSetDevice(c->device);
  if (u->d_red_index) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(u->d_red_index);
  }
  u->d_red_index = nullptr;
  u->red = nullptr;
  u->n_red_index = 0;
  // what the inspector left for this index was computed under the old hint (the cache key names the reduced SET, not the
  // index contents): a replay would skip the device-side check of the new one
  u->insp_valid = false;
  u->insp.clear();
  if (!reduced) return GCRE_OK;
  if (reduced->ctx != c || !index || n < 0) return fail(c, GCRE_ERR_ARG, "bad reduced operand");
  for (int64_t i = 0; i < n; i++)
    if ((int64_t)((uint32_t)index[i] & 0x7fffffffu) >= reduced->nrows) return fail(c, GCRE_ERR_RANGE, "reduced index out of range");
  if (n == 0) return GCRE_OK;
  HIP_TRY(c, hipMalloc((void**)&u->d_red_index, (size_t)n * 4));
  HIP_TRY(c, hipMemcpyAsync(u->d_red_index, index, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  u->red = reduced;
  u->red_id = reduced->id;
  u->n_red_index = n;
  return GCRE_OK;
}

void gcre_uids_free(gcre_uids* u) {
  if (u && u->ctx) (void)hipSetDevice(u->ctx->device);
  free_uids(u);
}

int gcre_join_uids(gcre_ctx* c, const gcre_uids* uids, const gcre_pathset* paths0, const gcre_pathset* paths1,
                   gcre_pathset* res, const gcre_join_opts* opts, gcre_result* out) {
  if (!c || !uids || !out) return fail(c, GCRE_ERR_ARG, "bad join arguments");
  (void)hipSetDevice(c->device);
  JoinPlan jp{uids, paths0, paths1, res, opts && opts->sharded, opts ? opts->shard_begin : 0,
              opts ? opts->shard_end : 0, opts ? opts->d_null_out : nullptr};
  jp.take(opts);
  jp.tally = c->armed_tally;
  c->armed_tally = nullptr;
  jp.exceed = c->armed_exceed;
  c->armed_exceed = nullptr;
  jp.hits = c->armed_hits;
  c->armed_hits = nullptr;
  int rc = run_join(c, jp, out);
  if (rc != GCRE_OK) gcre_result_free(out);
  return rc;
}

int gcre_join_ahead(gcre_ctx* c, const gcre_uids* uids, const gcre_pathset* paths0, const gcre_pathset* paths1,
                    gcre_pathset* res, const gcre_join_opts* opts) {
  if (!c) return GCRE_ERR_ARG;
  if (!uids) { drop_ahead(c); c->ahead_closed = false; return GCRE_OK; }   // (cancels the registrations)
  if (!c->ahead_on || !c->insp_cache || c->ahead_closed) return GCRE_OK;   // nothing to inspect ahead into: the joins simply run whole
  if (uids->ctx != c || !paths0 || !paths1 || paths0->ctx != c || paths1->ctx != c || (res && res->ctx != c))
    return fail(c, GCRE_ERR_ARG, "uids / path set do not belong to this context");
  if (opts && opts->exchange && opts->exchanges > 0) {
    // a join that exchanges thresholds with other devices runs whole, in its own call -- and so does everything behind it in
    // the sequence (it reads what this one writes)
    c->ahead_closed = true;
    return GCRE_OK;
  }
  if (!c->ahead) c->ahead = new std::vector<JoinPlan>();
  JoinPlan a{uids, paths0, paths1, res, opts && opts->sharded, opts ? opts->shard_begin : 0, opts ? opts->shard_end : 0, nullptr};
  a.take(opts);
  c->ahead->push_back(a);
  return GCRE_OK;
}

void gcre_result_free(gcre_result* r) {
  if (!r) return;
  std::free(r->scores);
  std::free(r->src);
  std::free(r->trg);
  std::free(r->cases);
  std::free(r->ctrls);
  std::free(r->null_max);
  std::memset(r, 0, sizeof *r);
}

int gcre_get_profile(const gcre_ctx* c, gcre_profile* out) {
  if (!c || !out) return GCRE_ERR_ARG;
  *out = c->prof;
  return GCRE_OK;
}

int gcre_resolve_count_locs(const int32_t* trg_uids, int64_t n_uids, const int32_t* keys, const int32_t* counts,
                            const int32_t* locations, int64_t n_keys, int32_t* out_count, int64_t* out_location) {
  if (n_uids < 0 || n_keys < 0 || (n_uids > 0 && (!trg_uids || !out_count || !out_location)) ||
      (n_keys > 0 && (!keys || !counts || !locations)))
    return GCRE_ERR_ARG;
  std::unordered_map<int32_t, std::pair<int32_t, int32_t>> map;   // count_locs, wrapper.cpp:106-112
  map.reserve((size_t)n_keys * 2);
  for (int64_t i = 0; i < n_keys; i++) map[keys[i]] = {counts[i], locations[i]};
  for (int64_t k = 0; k < n_uids; k++) {
    auto it = map.find(trg_uids[k]);   // a missing key reads as {0, 0}, wrapper.cpp:124-126
    out_count[k] = (it == map.end()) ? 0 : it->second.first;
    out_location[k] = (it == map.end()) ? 0 : it->second.second;
  }
  return GCRE_OK;
}

}  // extern "C"

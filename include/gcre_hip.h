/*
 * gcre_hip.h -- C ABI of libgcre_hip.so, the MI355X (gfx950) implementation of geneticsCRE's
 * permutation-tested path-join scorer.
 *
 * This is the drop-in boundary: the entry points below are what a replacement for the reference's
 * src/wrapper.cpp binds (R .Call shim) and what the Python host in
 * geneticscre_amd/api.py binds through ctypes.  Plain pointers and sizes only; nothing throws across
 * the boundary; every function returns 0 on success or a negative gcre_status, and the message is
 * available from gcre_last_error().  A context is used from one host thread at a time.
 *
 * Reference interface replaced (paths relative to /root/reference):
 *   JoinExec ctor / setValueTable / setPermutedCases   src/join_base.cpp:37-125, src/gcre.h:103-180
 *   PathSet ctor / load / select                        src/gcre_paths.h:19-92
 *   JoinExec::join (+ JoinMethod1/2::score_permute)     src/join_base.cpp:189-264, src/methods.h:58-232
 *   ProcessPaths (the 39-argument driver)               src/wrapper.cpp:177-281
 */
#ifndef GCRE_HIP_H
#define GCRE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCRE_ABI_VERSION 4

typedef enum {
  GCRE_OK = 0,
  GCRE_ERR_ASSERT = -1,   /* std::logic_error("assertion") in the reference (gcre_types.h:58-66) */
  GCRE_ERR_RANGE = -2,    /* std::out_of_range("assertion")            (gcre_types.h:68-76) */
  GCRE_ERR_DEVICE = -3,   /* HIP runtime failure or no gfx950 device */
  GCRE_ERR_ARG = -4       /* NULL / malformed argument */
} gcre_status;

typedef struct gcre_ctx gcre_ctx;           /* JoinExec   -- src/gcre.h:103-180 */
typedef struct gcre_pathset gcre_pathset;   /* PathSet    -- src/gcre_paths.h:10-98, rows live in HBM */

/* joined_res + Score -- src/gcre_types.h:32-48.  Arrays are owned by the library until gcre_result_free. */
typedef struct {
  int32_t n;            /* entries, <= top_k, ascending score; may hold the {-inf,-1,-1,0,0} sentinel
                           when the level has fewer than top_k scorable paths (join_base.cpp:194) */
  double* scores;
  int32_t* src;         /* Score.src = row of paths0 / uid index (methods.h:92) */
  int32_t* trg;         /* Score.trg = row of paths1 */
  int32_t* cases;
  int32_t* ctrls;
  int32_t n_perm;       /* = iterations requested */
  float* null_max;      /* per-permutation maximum over this level's paths, f32 (methods.h:101-102) */
} gcre_result;

/* Optional knobs of one join.  Zero-initialise for the reference behaviour. */
typedef struct {
  int32_t sharded;      /* 0: score every joined path (reference behaviour); 1: only [shard_begin, shard_end) */
  int32_t keep_ranged;  /* 0: kept path rows are produced in full, whatever the shard; 1: only rows [keep_begin, keep_end)
                           and the scored shard are produced -- the rest of `res` is left untouched; 2: every row is
                           produced, but only rows [keep_begin, keep_end) and the shard get their permutation count planes
                           (what a later join needs of the rows it reads as paths0; any other use rebuilds them).  For
                           multi-device runs: a device only needs the kept rows its own shards of the later joins read */
  int64_t shard_begin;  /* joined-path ordinal range scored on THIS device (may be empty). */
  int64_t shard_end;
  void* d_null_out;     /* optional device pointer to iterations floats: receives this shard's null maxima
                           (for an RCCL MAX all-reduce by the caller); may be NULL */
  int64_t keep_begin;   /* joined-path ordinals = rows of `res` (see keep_ranged) */
  int64_t keep_end;
  /* Multi-device runs: a shard prunes its table look-ups against the running per-permutation maxima (the reference's
   * `perm_scores[r] = max(...)`, src/methods.h:101-102, is what they bound), and a device that sees 1/N of the paths
   * knows lower maxima than the whole level has.  When `exchange` is set the join calls it exactly `exchanges` times --
   * after the warm-up slice and between the slices (1/2^(E-1), .., 1/4, 1/2 of the shard) of its permutation kernel --
   * with the device buffer d_null_out holding this shard's maxima of permutations [k0, k1) so far (floats, >= 0); the
   * callee MAX-all-reduces them in place across the devices (RCCL) and returns 0 once the buffer may be read; the join
   * goes on with the merged maxima as thresholds.  Every device must pass the same `exchanges`; a join that takes another
   * kernel form still makes its calls, so that the collectives match up.  Results do not depend on it.  d_null_out is
   * required. */
  int32_t exchanges;
  int (*exchange)(void* user, void* d_null, int32_t k0, int32_t k1);
  void* exchange_user;
} gcre_join_opts;

/* Timing of the last join / process_paths call, measured with HIP events on the library's stream. */
typedef struct {
  double null_kernel_ms;      /* sum over launches of the permutation (null) kernel */
  int64_t null_kernel_launches;
  double stats_kernel_ms;     /* real-label scoring + kept-row materialisation */
  double select_ms;           /* top-k selection */
  double total_ms;            /* whole device region */
  int64_t paths;              /* joined paths scored on this device */
  int64_t scores;             /* paths x iterations */
  double null_alg_bytes;      /* algorithmic HBM bytes of the null kernel launches */
  double null_row_loads;      /* sparse kernel: mask-row loads issued (list entries x permutation tiles); 0 = dense kernel */
  int64_t ie_launches;        /* launches of the inclusion-exclusion kernel (gcre_ie.hip) */
  int64_t ie_overlap_lists;   /* joined-path halves scored as N0 + Nz - overlap (the rest streamed their delta list) */
  int64_t ie_hinted_joins;    /* joins that ran on a verified gcre_uids_set_reduced operand */
  int64_t ie_plane_joins;     /* joins whose paths0 count planes were already resident */
  int64_t ie_lookup_tiles;    /* joined-path x 2048-permutation tiles that survived the pruning test (method 1); quad kernel with its flag queue: tiles the bound filter flagged */
  double prepare_ms;          /* host wall time: bit lists / count planes of the operands (once per set and mask epoch) */
  double inspect_ms;          /* host wall time: list offsets (scan), list fill and the syncs around them */
  int64_t ie_quad_launches;   /* of ie_launches: pruned method-1 launches that ran the four-paths-per-wave form (gcre_ieq.hip) */
  int64_t inspect_replays;    /* chunks that started at the null kernel: their inspector output was still in place (gcre_set_inspect_cache) */
} gcre_profile;

/* ---- context: JoinExec::JoinExec, src/join_base.cpp:37-59.  method 1 = unsigned, 2 = signed. ---- */
gcre_ctx* gcre_create(int method, int n_cases, int n_ctrls, int iterations, int device);
void gcre_destroy(gcre_ctx* ctx);   /* also releases every path set, uids object and gene tally still alive on the context: their handles die with it */
const char* gcre_last_error(const gcre_ctx* ctx);   /* ctx may be NULL: error of the last failed gcre_create */
int gcre_abi_version(void);
/* the extra compiler flags the library was built with ("" for the shipped build): a diagnostics build that switches parts of
   a kernel off for a timing experiment (GCRE_*_NO*, results are wrong) is recognisable, __graft_entry__.smoke() asserts "" */
const char* gcre_build_flags(void);
int gcre_device_count(void);   /* gfx950 devices visible to the process (0 when there is none: gcre_create then fails) */

int gcre_set_top_k(gcre_ctx* ctx, int top_k);        /* JoinExec::top_k, src/gcre.h:120 (default 12) */
int gcre_width_ul(const gcre_ctx* ctx);              /* 64-bit words per case/control mask, ceil(n/64) */
int gcre_vlen(const gcre_ctx* ctx);                  /* words per path row as seen by the host = width * method */

/* JoinExec::setValueTable, src/join_base.cpp:62-80.  nrow x ncol doubles; col_major != 0 for an R matrix.  Any table: cells
   it does not have read as -1; NaN, infinities, negatives, signed zeros and values beyond f32 score as in the reference.  A
   signed-method table with a NaN on one side of its diagonal only (vtmax = std::max is then not symmetric) is kept with its
   mirror image and scored by the dense permutation kernel alone, without pruning: much slower at production sizes, and
   said so on stderr unless GCRE_QUIET is set. */
int gcre_set_value_table(gcre_ctx* ctx, const double* table, int nrow, int ncol, int col_major);

/* JoinExec::setPermutedCases, src/join_base.cpp:85-125.  nrow x ncol ints, 1 = label kept. */
int gcre_set_perm_cases(gcre_ctx* ctx, const int32_t* perms, int nrow, int ncol, int col_major);

/* Extension: the same masks already packed, nrow x width_ul words, bit c of row r = "patient c is a case
 * under permutation r" (what setPermutedCases derives).  Same row reuse / truncation rules. */
int gcre_set_perm_masks(gcre_ctx* ctx, const uint64_t* masks, int nrow);

/* ---- path sets ---- */
gcre_pathset* gcre_pathset_zeros(gcre_ctx* ctx, int64_t nrows);                    /* createPathSet, join_base.cpp:157-161 */
gcre_pathset* gcre_pathset_from_dense(gcre_ctx* ctx, const int32_t* data, int64_t nrow, int ncol,
                                      int col_major);                               /* PathSet::load, gcre_paths.h:56-78 */
gcre_pathset* gcre_pathset_from_words(gcre_ctx* ctx, const uint64_t* rows, int64_t nrows);   /* packed rows, vlen words each */
gcre_pathset* gcre_pathset_select(gcre_ctx* ctx, const gcre_pathset* from, const int32_t* idx,
                                  int64_t n);                                       /* PathSet::select, gcre_paths.h:82-92 */
int64_t gcre_pathset_size(const gcre_pathset* ps);
int gcre_pathset_read(gcre_ctx* ctx, const gcre_pathset* ps, uint64_t* out_rows);   /* device -> host, size x vlen words */
void gcre_pathset_free(gcre_pathset* ps);

/*
 * JoinExec::join, src/join_base.cpp:189-264.
 *   uid_count / uid_location : uid_ref.count / .location per row of paths0 (src/gcre_types.h:50-56)
 *   signs                    : UidRelSet::signs, used by method 2 through need_flip (src/gcre.h:71-81)
 *   res                      : receives the joined rows (size must equal the total path count) or NULL
 * Ties between equal scores are resolved towards the smaller joined-path ordinal ("Ties").  Scores are
 * compared as doubles, as the reference compares them (methods.h:91): -0.0 and +0.0 tie, whichever of the two a path
 * scores it reports with its own sign.  The same holds for the per-gene tally and the observed exceedance counts.
 */
int gcre_join(gcre_ctx* ctx, int path_length,
              const int32_t* uid_count, const int64_t* uid_location, int64_t n_uids,
              const int32_t* signs, int64_t n_signs,
              const gcre_pathset* paths0, const gcre_pathset* paths1, gcre_pathset* res,
              const gcre_join_opts* opts, gcre_result* out);
void gcre_result_free(gcre_result* r);

/* UidRelSet (src/gcre.h:49-90) kept resident on the device, for callers that join the same level repeatedly
 * (benchmarks, sharded runs): gcre_join_uids == gcre_join without re-uploading the index. */
typedef struct gcre_uids gcre_uids;
gcre_uids* gcre_uids_create(gcre_ctx* ctx, int path_length, const int32_t* uid_count, const int64_t* uid_location,
                            int64_t n_uids, const int32_t* signs, int64_t n_signs);
int64_t gcre_uids_total_paths(const gcre_uids* uids);   /* UidRelSet::count_total_paths, gcre.h:83-88 */
void gcre_uids_free(gcre_uids* uids);
/* Optional speed hint, no reference counterpart (the reference walks every word of both operands, methods.h:73-88).
 * States that for every joined path (idx, loc) of this index
 *     paths0[idx] | paths1[loc]  ==  paths0[idx] | reduced[index[loc]]
 * e.g. at path length 4 paths1[loc] is the 2-gene path (c, d) whose first gene c already lies on paths0[idx], so
 * `reduced` = the per-gene rows and index[loc] = d.  The null kernel then adds the reduced row's precomputed
 * permutation counts instead of walking paths1[loc].  The claim is checked on the device for every join
 * (reduced row inside the joined row, equal carrier totals); a join for which it fails silently runs on paths1.
 * `index` has one entry per row of paths1 (n >= largest location + 1), values in [0, rows(reduced)); bit 31 of an
 * entry set = (signed method) the reduced row enters with its (+)/(-) halves swapped relative to how paths1[loc]
 * enters (UidRelSet::need_flip, gcre.h:71-81).
 * The caller keeps `reduced` alive while the index is used.  reduced == NULL removes the hint. */
int gcre_uids_set_reduced(gcre_uids* uids, const gcre_pathset* reduced, const int32_t* index, int64_t n);
int gcre_join_uids(gcre_ctx* ctx, const gcre_uids* uids, const gcre_pathset* paths0, const gcre_pathset* paths1,
                   gcre_pathset* res, const gcre_join_opts* opts, gcre_result* out);

/* Inspect-ahead.  A join is an inspector (expansion, real-label statistics and observed scores, kept rows, the lists the
 * permutation kernel streams, top-k selection: nothing of it depends on the permutation masks) followed by its permutation
 * kernel, and the inspector of the NEXT join of a sequence (src/wrapper.cpp:225-276) only reads what THIS join's inspector
 * wrote -- the kept rows -- not what its permutation kernel computes.  gcre_join_ahead registers the next join: the following
 * gcre_join / gcre_join_uids call on the context runs that join's inspector on a stream of its own as soon as its own kernels
 * are in flight, into the registered join index's inspection cache, and the registered join -- the same index, operands, kept
 * set and opts, called next -- starts at its permutation kernel.  Needs the inspection cache (gcre_set_inspect_cache(ctx, 1)
 * for the pass).  It is ON by default: ResidentPlan registers the chain for plans of up to 64 M joined paths (GCRE_AHEAD=1:
 * for any size); GCRE_AHEAD=0 turns it off, and then, or without the cache, the call registers nothing and every join runs
 * whole.  uids = NULL cancels a registration; freeing a registered object cancels it too.  Results never depend on it. */
int gcre_join_ahead(gcre_ctx* ctx, const gcre_uids* uids, const gcre_pathset* paths0, const gcre_pathset* paths1,
                    gcre_pathset* res, const gcre_join_opts* opts);


int gcre_get_profile(const gcre_ctx* ctx, gcre_profile* out);

/*
 * ProcessPaths, src/wrapper.cpp:177-281: the whole six-join sequence on plain arrays.
 * Level order of the six uid tables: 1a, 1b, 2, 3, 4, 5 (wrapper.cpp:177-182).  uid_count/uid_location are the
 * already-resolved count_locs (wrapper.cpp:106-132; gcre_resolve_count_locs below does that lookup).
 */
typedef struct {
  const int32_t* uid_count;
  const int64_t* uid_location;
  int64_t n_uids;
  const int32_t* signs;
  int64_t n_signs;
} gcre_level;

typedef struct {
  gcre_level level[6];
  const int32_t* data_inds[4];   /* 1a, 1b, 2, 3 -- 0-based rows of data1 / data2 (wrapper.cpp:205-208) */
  int64_t n_data_inds[4];
  const int32_t* data1;          /* genes x patients */
  int64_t data1_rows;
  const int32_t* data2;
  int64_t data2_rows;
  int data_col_major;            /* R matrices are column-major */
  const double* value_table;
  int vt_rows, vt_cols, vt_col_major;
  const int32_t* perm_cases;     /* iterations x patients; NULL with 0 rows = keep the masks the context already
                                  * holds (gcre_generate_perm_masks / gcre_set_perm_masks), an error if it has none */
  int perm_rows, perm_col_major;
  int path_length;               /* 1..5 */
  /* one device of several (gcre_process_paths_devices fills these; 0 / 0 / 0 = the whole job on this context): the
   * context scores joined-path ordinals [P * shard_rank / shard_world, P * (shard_rank + 1) / shard_world) of every
   * level and keeps every row; window_perms > 0 fixes the permutation window (all devices must walk the same ones) */
  int shard_rank, shard_world, window_perms;
} gcre_pp_input;

/* out[0..4] = lst1..lst5; entries above path_length have n = -1 (R sees NULL, wrapper.cpp:223). */
int gcre_process_paths(gcre_ctx* ctx, const gcre_pp_input* in, gcre_result out[5]);

/* The same call on several GPUs of one node from ONE process -- what the .Call shim uses, so that the drop-in takes the
 * node like the reference takes `nthreads` cores (src/join_base.cpp:163-185, src/wrapper.cpp:189).  One context and one
 * host thread per device; every device scores 1/n of each level's joined paths (contiguous ordinals, src/join_base.cpp:230
 * workers pull uids the same way) and keeps every row; the per-permutation null maxima are MAX-merged and the top-k
 * tables merged with the sentinel rule on the host when the devices are done (K floats + top_k rows per level and
 * device: the message sizes of SURVEY.md 2.2).  devices = NULL: devices 0 .. n_devices-1; n_devices <= 0: every visible
 * device; a device may be listed twice (rehearsal on one GPU).  Results are bit-identical for any device list.
 * err / errlen: optional buffer for the failing device's message. */
int gcre_process_paths_devices(int method, int n_cases, int n_ctrls, int iterations, int top_k, const int* devices,
                               int n_devices, const gcre_pp_input* in, gcre_result out[5], char* err, size_t errlen);

/* RCCL inside gcre_process_paths_devices.  When every device is listed once and librccl.so loads (dlopen: the library does
 * not link it), each device gets a communicator (ncclCommInitAll) and the K-float null maxima are merged by
 * ncclAllReduce(ncclFloat32, ncclMax) in place on the devices -- once per level and permutation window (merge_scores,
 * src/methods.h:34-37) and at every threshold exchange inside a large join; the top-k tables (top_k rows per device) are
 * merged on the host.  Environment: GCRE_RCCL=0 host-side merge only, GCRE_RCCL=force communicators for a single device
 * too (one-rank collectives).  gcre_rccl_selftest: a one-rank communicator on `device`, one MAX all-reduce, checked;
 * gcre_rccl_collectives: RCCL collectives this process has issued so far. */
int gcre_rccl_selftest(int device, char* err, size_t errlen);
int64_t gcre_rccl_collectives(void);

/* uid resolution of assemble_uids (src/wrapper.cpp:106-132): row k takes (count, location) of the entry
 * keyed by trg_uids[k]; missing keys give (0, 0). */
int gcre_resolve_count_locs(const int32_t* trg_uids, int64_t n_uids,
                            const int32_t* keys, const int32_t* counts, const int32_t* locations, int64_t n_keys,
                            int32_t* out_count, int64_t* out_location);

/* ------------------------------------------------------------------------------------------------------------
 * Callers and data formats either side of the path: native versions of what GWASPA prepares in R.
 * Not needed by the .Call drop-in (R keeps doing this work); used by non-R front ends and by the benchmark.
 * ------------------------------------------------------------------------------------------------------------ */

/* One join level as GWASPA builds it (R/ProcessPaths.R:214-256): uid_ref rows + UidRelSet::signs. */
typedef struct {
  int32_t path_length;
  int64_t n_uids;
  int32_t* src;         /* uid_ref.src */
  int32_t* trg;         /* uid_ref.trg */
  int32_t* count;       /* uid_ref.count */
  int64_t* location;    /* uid_ref.location (-1 where count == 0, R/PathMethods.R:147) */
  int64_t n_signs;
  int32_t* signs;
  int64_t total_paths;  /* UidRelSet::count_total_paths */
} gcre_level_table;

typedef struct {
  gcre_level_table level[6];   /* 1a, 1b, 2, 3, 4, 5 */
  int64_t n_data_inds[4];
  int32_t* data_inds[4];       /* 1a, 1b, 2, 3: 0-based rows of data1 / data2 */
  int64_t n_rels3;             /* getRels3 (src/wrapper.cpp:18-48): one row per 2-edge walk */
  int32_t *r3_src, *r3_trg, *r3_sign, *r3_trg2, *r3_sign2;
} gcre_levels;

/* Relations must be sorted by (src, trg), unique, without self loops; gene ids are 0..n_genes-1 = rows of the data
 * matrix (what GWASPA's filtering leaves, R/ProcessPaths.R:133-167, 210).  Arrays are malloc'ed; free with
 * gcre_levels_free. */
int gcre_build_levels(int32_t n_genes, const int32_t* src, const int32_t* trg, const int32_t* sign, int64_t n_edges,
                      gcre_levels* out);
void gcre_levels_free(gcre_levels* levels);

/* getValuesTable (R/Utils.R:137-159): out[(n_cases+1) x (n_ctrls+1)] row-major, -log two-sided hypergeometric p.
 * Parity with R's stats::dhyper is unpinned (no R in the build image); the scorer treats the table as opaque input. */
int gcre_values_table(int n_cases, int n_ctrls, double* out);
/* Which summation order gcre_values_table uses at this size: 1 = R's index order for every cell (the table R builds wherever
 * libm agrees), 0 = the sorted prefix sum of very large cohorts (past 2.5e11 inner steps, ~14,000 patients: same outcomes, same
 * accumulator, the rounded double can move in its last place).  Fixtures record it next to their input digest.  The test-only
 * GCRE_VT_EXACT_WORK environment variable moves the threshold for both functions alike. */
int gcre_values_table_exact_order(int n_cases, int n_ctrls);

/* getRandIndicesMat + getCaseORControl + setPermutedCases (R/Utils.R:22-46, 246-262; src/join_base.cpp:85-125) fused
 * on the device: permutation r = a uniformly random relabelling that keeps n_cases cases (inside every stratum when
 * `stratum[n]` is given, values 0..n_strata-1, R/Utils.R:8-13).  Deterministic in (seed, r, patient): see
 * gcre_mix64 and k_generate_masks.  Replaces gcre_set_perm_cases for callers that do not need R's RNG stream. */
int gcre_generate_perm_masks(gcre_ctx* ctx, uint64_t seed, const int32_t* stratum, int n_strata);
uint64_t gcre_mix64(uint64_t z);
/* Restrict the joins that follow to permutations [k0, k1) (k0 a multiple of 2048; k1 a multiple of 2048 or = iterations).
 * A join then returns k1 - k0 null maxima; observed scores and top-k lists do not depend on the window.  Lets a caller
 * run a large permutation count in batches whose count planes (one per kept row and 2048-permutation tile) fit in device
 * memory -- gcre_process_paths does so on its own.  Setting masks resets the window to [0, iterations). */
int gcre_set_perm_window(gcre_ctx* ctx, int k0, int k1);
/* Window length (permutations; a multiple of 2048, or iterations when everything fits) for a pipeline whose path sets --
 * the inputs and the kept sets -- hold set_rows[i] rows: the count planes of a set take up to 4 KB per row, method half
 * and tile (method 1: sets above the recipe limit, GCRE_PLANES_OUT_MAX_MB, store none) and should leave half of the free
 * device memory alone. */
int gcre_plan_perm_window(gcre_ctx* ctx, const int64_t* set_rows, int n_sets);
/* Inspection cache.  What a join computes before its permutation (null) kernel -- expanded row numbers, carrier
 * totals, observed scores and their top-k, the kept rows, the inclusion-exclusion lists (JoinExec::join's real-label half,
 * src/join_base.cpp:236-262 + methods.h:90-99) -- does not depend on the permutation masks.  With the cache on, that
 * output stays with the join index (gcre_uids) it was computed for, and a later join on the same index with the same
 * operand rows, kept set, shard, top_k and value table starts at the null kernel: the 2nd..nth permutation window of a
 * large run, or the next pass over resident inputs.  Results are identical either way.  gcre_process_paths turns it on
 * by itself for a call that needs more than one window.  Off by default (the buffers cost ~80 B per joined path).
 * gcre_drop_inspections forgets what is cached (release_memory = 0 keeps the buffers for the next run). */
int gcre_set_inspect_cache(gcre_ctx* ctx, int on);
int gcre_drop_inspections(gcre_ctx* ctx, int release_memory);
/* read permutation mask r back as width_ul words (bit c = patient c is a case under permutation r) */
int gcre_get_perm_mask(gcre_ctx* ctx, int r, uint64_t* out);
/* Tests only: one helper kernel of a join, run on inputs given from the host, its output copied back word for word.
 * gcre_test_range_union: the range check of a hinted join over ranges r = rows loc[r] .. loc[r] + cnt[r] - 1 of p1 (n1 rows of
 * S = method * Wp words; zindex[n1]: the row of pz that stands for each, bit 31 = halves swapped); u_out[n_ranges * S] is the
 * excess per range, *bad_out whether some reduced row is not inside the row it stands for, *piece_rows_out the number of rows
 * above which a range is walked in pieces.  gcre_test_expand: ordinals [first, first + count) of the join index
 * (path_idx[n_uids + 1], location[n_uids], signs[n_signs]) to their rows of paths0 (row0) and paths1 (row1, bit 31 = swap). */
int gcre_test_range_union(gcre_ctx* ctx, const uint64_t* p1, int64_t n1, const uint64_t* pz, int64_t nz, const int32_t* zindex,
                          const int64_t* loc, const int32_t* cnt, int64_t n_ranges, int S, int Wp, int method, uint64_t* u_out,
                          uint32_t* bad_out, int32_t* piece_rows_out);
int gcre_test_expand(gcre_ctx* ctx, const int64_t* path_idx, const int64_t* location, int64_t n_uids, const int32_t* signs,
                     int64_t n_signs, int path_length, int method, int64_t first, int64_t count, uint32_t* row0, uint32_t* row1);
/* Tests only: the method-1 inspector of the inclusion-exclusion form on given row numbers.  Path i joins row row0[i] of p0 to
 * row row1[i] of red, or, with zindex[n_zindex], to row zindex[row1[i]] of it (a hinted join; then excess[n_ranges * vlen] and
 * range_of[rows of p0] are its range table, or both NULL).  The counts come from the row totals of red where
 * GCRE_STATS_IE_COUNTS (default 1) and the sizes say so: red has no more rows than there are paths.  over_entries: room for
 * the lists' parts beyond 8 entries.  Out, per path: tot, cases, ctrls, rowz, linfo, key, and entries[i * ent_stride ..): the
 * list, padding included (its padded length: linfo & 0x0ffffff8); res_out (or NULL): the joined rows; flags[8]: the
 * inspector's flag block (largest total, hint broken, overlap lists, -, overflow entries reserved, longest list). */
int gcre_test_inspect(gcre_ctx* ctx, const gcre_pathset* p0, const gcre_pathset* red, const uint32_t* row0, const uint32_t* row1,
                      int64_t count, const int32_t* zindex, int64_t n_zindex, const uint64_t* excess, const int32_t* range_of,
                      int64_t n_ranges, int64_t over_entries, uint32_t* tot, uint32_t* cases, uint32_t* ctrls, uint32_t* rowz,
                      uint32_t* linfo, uint64_t* key, uint32_t* entries, int64_t ent_stride, uint64_t* res_out, uint32_t* flags);

/* ------------------------------------------------------------------------------------------------------------
 * Decorated p-values (getDecoratedPvalues / computeDecoratedPvalue, R/DecoratedPvalue.R:48-304; GWASPA's second table,
 * R/ProcessPaths.R:330-337).  Every path of length L >= 2 is split at its 2(L-1) cut points -- Forward j = 1..L-1:
 * sub-path 1 = genes 1..j, gene 2 = g(j+1); Backward j = L..2: sub-path 1 = genes L..j, gene 2 = g(j-1) -- and the
 * carriers gene 2 adds to sub-path 1 are tested against the same number of patients drawn without replacement from those
 * sub-path 1 does not cover.  Only the number of cases among the drawn patients matters, so each draw is an urn process
 * (DESIGN.md "Decorated p-values").  Draws come from a counter-based stream keyed by (seed, split, permutation), not
 * from R's RNG: the table matches R in distribution. */

/* One stratum of one split: the two urns drawn in it (DecoratedPvalue.R:240-273). */
typedef struct {
  int32_t pop;      /* |G_s|, G_s = stratum s minus the carriers of sub-path 1, both halves */
  int32_t cases;    /* cases in G_s: the successes of the pos urn */
  int32_t k_pos;    /* |pos2 ∩ G_s| patients drawn from G_s for the pos half */
  int32_t k_neg;    /* |neg2 ∩ G_s| drawn from what the pos draw left of G_s; its successes are controls */
} gcre_dp_stratum;

typedef struct {
  int32_t method;             /* 1: every gene is "pos"; 2: a gene tagged (-) is "neg" (DecoratedPvalue.R:126-130) */
  int32_t n_cases, n_ctrls;   /* patients 0..n_cases-1 are the cases */
  int32_t n_paths;
  const int32_t* path_len;    /* [n_paths], 1..5; a length-1 path has no split */
  const int32_t* path_rows;   /* [n_paths][5]: row of `rows` of each gene, -1 = NA gene (the whole path gets NaN) */
  const int32_t* path_sign;   /* [n_paths][5]: -1 = (-), anything else (+); read by method 2 only; may be NULL */
  const uint64_t* rows;       /* [n_rows][ceil(n/64)] carriers, bit c of word c/64 = patient c (bits >= n ignored) */
  int32_t n_rows;
  const int32_t* stratum;     /* optional [n]: stratum id 0..n_strata-1 of each patient */
  int32_t n_strata;
  int32_t iterations;         /* permutations per split */
  uint64_t seed;
  gcre_dp_stratum* strata_out;   /* output, required with `stratum`: [cap][n_strata] urns, split i at strata_off */
} gcre_dp_input;

/* One split (one row of Decorated.Pvalues.Results). */
typedef struct {
  int32_t path;        /* index into gcre_dp_input.path_len */
  int32_t direction;   /* 0 = "Forward", 1 = "Backward" */
  int32_t j;           /* R's j (1-based cut point of that direction's loop) */
  int32_t valid;       /* 0: the path holds an NA gene -- counts 0, score and p-value NaN */
  int32_t cases1, ctrls1, cases2, ctrls2;   /* Subpaths1_Cases .. Subpaths2_Controls: case_pos + case_neg, ... */
  /* sub-path 1 per half, the neg half counted the other way round (case_neg1 = its controls, DecoratedPvalue.R:223-226) */
  int32_t case_pos1, ctrl_pos1, case_neg1, ctrl_neg1;
  int32_t case_pos2, ctrl_pos2, case_neg2, ctrl_neg2;   /* gene 2 minus sub-path 1 in its own half, counted the same way */
  double score;        /* observed score; NaN from gcre_decorated_splits without a table */
  /* the two urns without strata: draw k from a population of pop holding succ successes (pos half: cases outside pos1;
     neg half: controls outside neg1).  With strata k_pos / k_neg are the totals over the strata, pop / succ are 0, and
     the urns are strata_out[strata_off .. strata_off + n_strata) */
  int32_t k_pos, pop_pos, succ_pos;
  int32_t k_neg, pop_neg, succ_neg;
  int64_t strata_off;  /* -1 without strata */
  int64_t n_ge;        /* permutations whose score >= score (gcre_decorated_pvalues) */
  double pvalue;       /* n_ge / iterations; NaN for an invalid split or 0 iterations */
} gcre_dp_split;

/* The host stage, no device needed: every split's counts, observed score (`table`: nrow x ncol doubles, col_major != 0
 * for an R matrix, read as the device reads its copy -- -1 outside the table; NULL leaves the score NaN) and urn
 * parameters.  Splits follow the paths in order, each path Forward then Backward.  *n_out = the number of splits;
 * GCRE_ERR_RANGE when cap is smaller (nothing is written), or when a row index or a stratum id is out of range. */
int gcre_decorated_splits(const gcre_dp_input* in, const double* table, int nrow, int ncol, int col_major,
                          gcre_dp_split* out, int64_t cap, int64_t* n_out);

/* gcre_decorated_splits, then k_decorated_null on the context's device: in->iterations permutations of every split,
 * scored against the value table of gcre_set_value_table.  Fills score, n_ge and pvalue.  in->method, n_cases and
 * n_ctrls must be the context's; in->strata_out may be NULL here.  perm_counts, optional [n_out][iterations][2]:
 * successes of the pos urn (cases) and of the neg urn (controls) of every permutation. */
int gcre_decorated_pvalues(gcre_ctx* ctx, const gcre_dp_input* in, gcre_dp_split* out, int64_t cap, int64_t* n_out,
                           int32_t* perm_counts);

/* ------------------------------------------------------------------------------------------------------------
 * Permutation tests of caller-given sets: a named path, a gene set, any list of carrier rows.  No reference counterpart
 * (its checkBestPaths, R/CheckResults.R:2-89, rescores named paths without permutations).  A set's members are rows of a
 * 0/1 carrier matrix; each member has a sign, read by method 2 only.
 *   method 1: U = OR of the members; score = VT[|U & cases|][|U & ctrls|] (methods.h:90)
 *   method 2: P = OR of the (+) members, N = OR of the (-) members (a row listed under both signs lands in both, no
 *             conflict removal: CheckResults.R:40-44); score = VT[|P & cases|][|P & ctrls|] + VT[|N & ctrls|][|N & cases|]
 *             (methods.h:255, CheckResults.R:69-73)
 * Null score of permutation r (mask_r = its cases): the f32 value the join's null kernels fold into their maxima --
 * method 1 t32[p][|U| - p], p = |U & mask_r|; method 2 (float)(vtmax[pp][|P| - pp] + vtmax[|N| - pn][pn]),
 * pp = |P & mask_r|, pn = |N & mask_r|; NaN and negatives fold as 0 (methods.h:96-103, :220-230).  So the maximum over
 * every joined path of a level, passed as sets, is that level's null_max bit for bit. */
typedef struct {
  int64_t n_sets;
  const int64_t* set_off;   /* [n_sets + 1]: set s = members[set_off[s] .. set_off[s+1]), at least one */
  const int32_t* members;   /* rows of `rows`; -1 = an NA gene (the set gets valid = 0) */
  const int32_t* signs;     /* per member, parallel to `members`: +1 / -1; NULL = all +1 */
  const uint64_t* rows;     /* [n_rows][ceil(n_cols/64)] carriers, bit c of word c/64 = patient c (bits >= n_cols ignored) */
  int64_t n_rows;
  int32_t n_cols;           /* patients: must be the context's n_cases + n_ctrls (columns < n_cases are the cases) */
} gcre_set_input;

/* One set's record. */
typedef struct {
  int64_t set;         /* index into the input */
  int32_t valid;       /* 0: an NA member -- counts 0, score and p-value NaN, not in family_max */
  int32_t cases, ctrls;   /* keep_score's Cases / Controls (methods.h:256-257): cases_pos + cases_neg, ctrls_pos + ctrls_neg */
  /* checkBestPaths' names (CheckResults.R:62-65): |P & cases|, |P & ctrls|, |N & ctrls|, |N & cases| (method 1: P = U, N empty) */
  int32_t cases_pos, ctrls_pos, cases_neg, ctrls_neg;
  double score;        /* observed score from the context's value table */
  int64_t n_ge;        /* permutations r < iterations with (double)null_r >= score (R/ProcessPaths.R:316) */
  double pvalue;       /* n_ge / iterations; NaN for an invalid set or 0 iterations */
} gcre_set_score;

/* Every set of `in` against the context's value table and all `iterations` permutation masks (whatever
 * gcre_set_perm_window says; strata come in through the masks).  *n_out = n_sets.  family_max, optional [iterations]:
 * per permutation the maximum of null_r over the valid sets (all zeros without one): max-T over a family the caller
 * chooses.  Errors, nothing launched: GCRE_ERR_ARG -- a set without members, a sign other than +1 / -1, n_cols not
 * n_cases + n_ctrls; GCRE_ERR_RANGE -- a member row out of range, n_sets > cap; GCRE_ERR_ASSERT -- no value table, or
 * iterations > 0 and no masks set.  DESIGN.md §3.6. */
int gcre_score_sets(gcre_ctx* ctx, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out,
                    float* family_max);

/* Conditional (residual) set scores: many (set, given set) pairs in one call.  Entry i scores set
 * s = which[i] with the carriers of set g = given[i] set aside: with P_s, N_s the unions gcre_score_sets defines (method 1:
 * U_s alone) and C_g the carrier row gcre_set_overlap defines -- the OR of ALL members of g, whatever their signs and the
 * method, bits >= n_cols ignored; g's own full row, never a residual itself -- the entry is scored as gcre_score_sets scores
 * a set whose unions are P_s & ~C_g and N_s & ~C_g: counts, observed score, n_ge and pvalue against all `iterations` masks.
 * n_cases / n_ctrls are unchanged: the removed patients count as non-carriers.  The rows are built on the device
 * (k_set_residual) from the gene rows and the set list, uploaded once.
 * which [n_which]: repeats allowed (leave-one-gene-out: one entry per gene, the one-gene set as the given set); NULL =
 * 0 .. n_sets-1, and then n_which must be n_sets.  given [n_which]: -1 = nothing set aside; NULL = all -1; given[i] ==
 * which[i] is allowed (an empty residual).  out[i].set = which[i], *n_out = n_which.  An entry whose set has an NA member
 * gets valid = 0 as in gcre_score_sets.  family_max, optional [iterations]: the maximum of null_r over the valid entries
 * (all zeros without one).  The entries are walked in slabs of GCRE_GIVEN_SLAB_SETS (environment, read per call; default:
 * what fits in 1 GiB of device rows); the results do not depend on it.
 * Errors, nothing launched: everything gcre_score_sets refuses of the context and the set list; GCRE_ERR_RANGE -- a `which`
 * entry outside 0 .. n_sets-1, a `given` entry outside -1 .. n_sets-1, n_which > cap; GCRE_ERR_ARG -- a `given` entry naming
 * a set with an NA member, n_which < 0, NULL `which` with n_which != n_sets.  n_which == 0 returns at once. */
int gcre_score_sets_given(gcre_ctx* ctx, const gcre_set_input* in, const int64_t* which, const int64_t* given,
                          int64_t n_which, gcre_set_score* out, int64_t cap, int64_t* n_out, float* family_max);
/* kernels launched by gcre_score_sets_given on the context since gcre_create (tests: a refusal launches nothing). */
int64_t gcre_given_launches(const gcre_ctx* ctx);

/* Step-down, k-FWER and FDR over the family of the given sets.  `out`, *n_out: exactly what
 * gcre_score_sets gives.  With N[i][r] = the f32 null score of valid set i under permutation r as stated above, obs_i its
 * observed score, every comparison as doubles against (double)N, over the valid sets:
 *   D_j              = {i : obs_i > obs_j}: tied sets never exclude one another, a set with a NaN score is in no D
 *   n_ge_stepdown[j] = #{r : max over i not in D_j of N[i][r] >= obs_j}    (Westfall-Young step-down, before the monotone step)
 *   exceed[j]        = #{(i, r) : N[i][r] >= obs_j}                        (the pooled null: expected false positives, FDR)
 *   observed[j]      = #{i : obs_i >= obs_j}
 *   kmax[k][r]       = the (k+1)-th largest of N[.][r], 0 where the family has fewer valid sets (k-FWER); kmax[0] is
 *                      gcre_score_sets' family_max bit for bit
 * A set with a NaN observed score gets 0 / 0 / 0; an invalid set (an NA member) -1 / 0 / -1 and an all-NaN row of null_scores.
 * So the best set's n_ge_stepdown is #{r : kmax[0][r] >= obs}; out[j].n_ge <= n_ge_stepdown[j] <= #{r : kmax[0][r] >= obs_j},
 * the single-step count; exceed[j] is the sum over i of #{r : N[i][r] >= obs_j}.  iterations == 0: `out` as gcre_score_sets
 * fills it, zeros for every valid set, nothing of the family launched.
 * N is kept on the device for a slab of whole 512-permutation tiles at a time, valid sets x slab permutations x 4 bytes
 * under GCRE_FAMILY_MAX_MB (environment, read per call, default 1024; GCRE_FAMILY_SLAB_PERMS bounds a slab further); no
 * result depends on the slabs.  fam_out [n_sets]; kmax optional [GCRE_FAMILY_KMAX][iterations]; null_scores optional
 * [n_sets][iterations] = N.
 * Errors, nothing launched and no output array written (*n_out as gcre_score_sets leaves it): everything gcre_score_sets
 * refuses; GCRE_ERR_ARG -- NULL fam_out, one 512-permutation tile of the valid sets above GCRE_FAMILY_MAX_MB. */
#define GCRE_FAMILY_KMAX 10
typedef struct {
  int64_t n_ge_stepdown;
  uint64_t exceed;
  int64_t observed;
} gcre_family_score;
int gcre_score_sets_family(gcre_ctx* ctx, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out,
                           gcre_family_score* fam_out, float* kmax, float* null_scores);
/* k_family_null / k_family_scan / k_family_hist launches on the context since gcre_create. */
int64_t gcre_family_launches(const gcre_ctx* ctx);

/* Westfall-Young min-P over the family of the given sets: every null score is replaced by the nominal
 * permutation p-value its permutation's data would have got from that set's OWN null distribution, and the minimum is
 * taken over the family -- sets whose raw null scores are not comparable (paths of mixed length, unions of many genes)
 * then weigh alike, which max-T on raw scores (family_max, gcre_score_sets_family) does not give.  One set of permutations
 * serves both roles (Ge, Dudoit & Speed 2003).  `out`, *n_out: exactly what gcre_score_sets gives.  With N[i][r] as above,
 * over the valid sets, comparisons against obs as doubles and among the values of one row on the f32 values:
 *   c_i              = out[i].n_ge = #{r : (double)N[i][r] >= obs_i}; 0 for a NaN score
 *   R[i][r]          = #{r' < iterations : N[i][r'] >= N[i][r]}, 1 .. iterations: iterations x the nominal p-value of r
 *   min_count[r]     = min over the valid sets i of R[i][r]
 *   n_le_minp[j]     = #{r : min_count[r] <= c_j}                              (single-step min-P)
 *   D_j              = {i : c_i < c_j}: tied sets never exclude one another, a set with a NaN score is in no D
 *   n_le_stepdown[j] = #{r : min over i not in D_j of R[i][r] <= c_j}           (step-down, before the monotone step)
 * So #{r : R[j][r] <= c_j} = c_j <= n_le_stepdown[j] <= n_le_minp[j], with equality of the two for the sets of the smallest
 * c, and a family of one valid set gives c for both.  A set with a NaN observed score gets 0 / 0; an invalid set (an NA
 * member) -1 / -1 and an all-0xFFFFFFFF row of null_counts.  iterations == 0: `out` as gcre_score_sets fills it, zeros for
 * every valid set, nothing of this stage launched.  min_count is all 0xFFFFFFFF without a valid set.
 * The valid sets are walked least significant first (NaN scores, then c descending) in slabs of whole rows: a row keeps
 * its null scores and its counts, 8 bytes per permutation of every 512-permutation tile, and a slab stays under
 * GCRE_MINP_MAX_MB (environment, read per call, default 1024; GCRE_MINP_SLAB_SETS bounds a slab further); no result depends
 * on the slabs.  mp_out [n_sets]; min_count optional [iterations]; null_counts optional [n_sets][iterations] = R.
 * Errors, nothing launched and no output array written (*n_out as gcre_score_sets leaves it): everything gcre_score_sets
 * refuses; GCRE_ERR_ARG -- NULL mp_out, one row of the working set above GCRE_MINP_MAX_MB. */
typedef struct { int64_t n_le_minp; int64_t n_le_stepdown; } gcre_minp_score;
int gcre_score_sets_minp(gcre_ctx* ctx, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out,
                         gcre_minp_score* mp_out /* [n_sets] */,
                         uint32_t* min_count     /* optional [iterations] */,
                         uint32_t* null_counts   /* optional [n_sets][iterations] = R */);
/* k_minp_gather / k_family_null / k_minp_rank / k_minp_scan launches of gcre_score_sets_minp on the context since
 * gcre_create (gcre_family_launches does not count them, nor the reverse). */
int64_t gcre_minp_launches(const gcre_ctx* ctx);

/* Competitive tests of the given sets (Goeman & Buhlmann 2007): does a set score higher, on the OBSERVED
 * labels, than random gene sets of the same size and the same carrier frequencies?  The null is over genes, not labels: no
 * permutation mask is read, and a context with iterations == 0 and no masks is the usual one.  `out`, *n_out: exactly what
 * gcre_score_sets gives, so one call yields both p-values.
 * in->rows are the whole gene POOL, not only the members.  bin [n_rows]: 0 .. n_bins-1, or -1; NULL = one bin holding every
 * row.  The pool of bin B is the rows with bin[row] == B in ascending row order, N_B of them.  A row with bin -1 is never
 * drawn, and a member on such a row is FIXED: it stays itself in every draw.
 * Draw b (0 .. draws-1) of set s replaces every member that is not fixed, in member order j = 0, 1, ... (the position in the
 * set's list), by a row of its own bin that no earlier member of this draw has received; the member keeps its sign.  With
 *   base = dp_perm_base(dp_split_key(seed, s), b)      (the keys of gcre_decorated_pvalues; gcre_mix64 below)
 * attempt t = 0, 1, ... of member j reads u = gcre_mix64(base + 64 j + t) and proposes pool entry floor(u N_B / 2^64) (the
 * 128-bit product); the first proposal not yet handed out in this draw is taken.  After A failed attempts the member gets
 * the lowest pool entry of its bin not yet handed out; A = 64 (GCRE_COMPETE_ATTEMPTS, environment, read per call, lowers it
 * to 1 .. 64: tests).  A set with k members to draw from a bin needs 2 k <= N_B, so every attempt succeeds with probability
 * 1/2 or more.  A draw may hand out rows that are members of the set; draws of different sets and different b are
 * independent and a pure function of (seed, s, b).
 * Null score of a draw: the unions of the drawn rows as gcre_score_sets defines them for the context's method (method 1 the
 * OR of all rows, method 2 P / N by sign), counted against the observed labels (columns < n_cases are the cases), and the
 * f64 value of the context's table for those counts: the expression of the observed score, and for method 2 its order of the
 * addition -- a draw that hands every member its own row reproduces the observed score bit for bit.
 *   n_ge[s] = #{b < draws : null[s][b] >= obs_s} as doubles (a NaN on either side never counts); -1 for an invalid set (an
 *   NA member); zeros with draws == 0, which launches nothing of this stage.
 * null_scores, optional [n_sets][draws] (NaN rows for invalid sets); picks, optional [draws][total members]: the row each
 * member received, in the order of in->members (fixed members their own row, -1 for the members of invalid sets).  The
 * draws are walked in slabs whose optional outputs stay under GCRE_COMPETE_MAX_MB on the device (environment, read per
 * call, default 1024; GCRE_COMPETE_SLAB_DRAWS bounds a slab further); no result depends on the slabs.
 * Errors, nothing launched and no output array written (*n_out as gcre_score_sets leaves it): everything gcre_score_sets
 * refuses; GCRE_ERR_ARG -- NULL n_ge, draws < 0, n_bins < 1, a bin value outside -1 .. n_bins-1, a set that breaks
 * 2 k <= N_B, a set of more than GCRE_COMPETE_MAX_MEMBERS members, the optional outputs of one draw above
 * GCRE_COMPETE_MAX_MB.
 * The number is a rank among matched random sets conditional on the labels; it is not a family-wise statement. */
#define GCRE_COMPETE_MAX_MEMBERS 1024
int gcre_score_sets_compete(gcre_ctx* ctx, const gcre_set_input* in, const int32_t* bin, int32_t n_bins, int64_t draws,
                            uint64_t seed, gcre_set_score* out, int64_t cap, int64_t* n_out, int64_t* n_ge,
                            double* null_scores, int32_t* picks);
/* k_compete_null launches of gcre_score_sets_compete on the context since gcre_create (no other launch counter counts
 * them, nor the reverse). */
int64_t gcre_compete_launches(const gcre_ctx* ctx);

/* Variable-threshold tests of the given sets (Price et al. 2010): the best score over nested prefixes of a
 * set's member list, with the same maximum taken under every permutation, so that the selection of the prefix is paid for
 * inside the null.  `out`, *n_out: exactly what gcre_score_sets gives for the full sets, so one call yields both p-values.
 * Steps.  Member i of the flat member list ends a step if cut[i] != 0; the last member of every set always ends one; cut
 * NULL = every member is a cut.  Step k (0, 1, ...) of set s is the set made of its members up to and including the k-th
 * cut member, with their signs, and is scored as gcre_score_sets scores that set: the same counts, the same f64 observed
 * expression, the same f32 null value N[step][r] (NaN and negatives folded to 0).
 *   score        = the observed score of step best_step
 *   best_step    = the smallest step that attains the maximum of the observed step scores, NaN steps skipped (-1 and a NaN
 *                  score if every step is NaN)
 *   best_members = members of that prefix (0 for NaN); steps = the steps of the set
 *   cases_pos .. ctrls_neg = the counts of that step (zeros for NaN)
 *   T[s][r]      = max over the steps of set s of N[step][r]
 *   n_ge         = #{r < iterations : (double)T[s][r] >= score}; 0 for a NaN score, -1 for an invalid set (an NA member)
 * iterations == 0: nothing of this stage is launched; every record keeps `steps`, n_ge = 0 (-1 for an invalid set), a NaN
 * score and best_step = -1.  An invalid set has a NaN score, best_step = -1 and its `steps`.
 * family_max, optional [iterations]: max of T[s][r] over the valid sets (all zeros without one) -- bit for bit
 * gcre_score_sets' family_max over the step sets.  null_max, optional [n_sets][iterations] = T (NaN rows for invalid sets).
 * step_scores, optional [members of the list]: the observed score of the step that ends at member i, NaN where i ends no
 * step and for invalid sets.
 * The step rows are built on the device (k_prefix_rows) from the gene rows and the set list, uploaded once.  The valid sets
 * are walked in slabs of whole sets whose step rows -- and null_max rows, when asked -- stay under GCRE_PREFIX_MAX_MB on the
 * device (environment, read per call, default 1024; GCRE_PREFIX_SLAB_SETS bounds a slab further); no result depends on the
 * slabs.
 * Errors, nothing launched and no output array written (*n_out as gcre_score_sets leaves it): everything gcre_score_sets
 * refuses; GCRE_ERR_ARG -- NULL px_out, one valid set whose step rows (and null_max row) exceed GCRE_PREFIX_MAX_MB.
 * n_ge / iterations is a self-contained permutation p-value of the maximum over the caller's nested prefixes, one set at a
 * time; the order and the cuts must not be chosen from the labels. */
typedef struct {
  double score;
  int64_t n_ge;
  int32_t best_step, best_members, steps;
  int32_t cases_pos, ctrls_pos, cases_neg, ctrls_neg;
} gcre_prefix_score;
int gcre_score_sets_prefix(gcre_ctx* ctx, const gcre_set_input* in, const uint8_t* cut /* [members], optional */,
                           gcre_set_score* out, int64_t cap, int64_t* n_out,
                           gcre_prefix_score* px_out      /* [n_sets] */,
                           float* family_max              /* optional [iterations] */,
                           float* null_max                /* optional [n_sets][iterations] */,
                           double* step_scores            /* optional [members] */);
/* k_prefix_rows / k_set_observed / k_prefix_pick / k_prefix_null launches of gcre_score_sets_prefix on the context since
 * gcre_create (no other launch counter counts them, nor the reverse); -1 for a NULL context. */
int64_t gcre_prefix_launches(const gcre_ctx* ctx);

/* Split-half stability of the given sets (Meinshausen & Buhlmann 2010, Shah & Samworth 2013): how often does
 * a set still reach a cut-off when it is scored on a random half of the cases and of the controls (half A), on the
 * complementary half (half B), and on both?  The draws subsample the PATIENTS; the labels stay as observed.  No permutation
 * mask is read: the draws are independent of the context's masks, and a context with iterations == 0 is the usual one.
 * `out`, *n_out: exactly what gcre_score_sets gives on the full cohort, so one call yields both.
 * Draw b (0 .. draws-1) is a mask S_b over the n = n_cases + n_ctrls patients with exactly m_cases bits among the columns
 * < n_cases and exactly m_ctrls among the rest, made by the rule of gcre_generate_perm_masks (Knuth's selection sampling)
 * with two strata, a patient's stratum being its label, and the needs (m_cases, m_ctrls):
 *   seed'  = gcre_mix64(seed ^ 0x73756273616d706c)
 *   base_b = gcre_mix64(seed' ^ (0x51ed270b7f3c9a1d * (b + 1)))
 * patient c, in column order, reads u = gcre_mix64(base_b + c) and is taken when floor(u rem / 2^64) < need (the 128-bit
 * product), rem the patients of its stratum not yet walked (c included) and need those still to be taken.  A pure function
 * of (seed, b, c).
 * Scores.  With P, N the unions gcre_score_sets defines (method 1: one union alone), half A's counts are |P & S_b & cases|,
 * |P & S_b & ctrls| and likewise for N; its score is the f64 expression of the observed score -- for method 2 in its order of
 * the addition -- read from table_a [nrow_a][ncol_a], row-major, the value table of a cohort of m_cases cases and m_ctrls
 * controls.  Half B's counts are the set's totals minus half A's, its score is read from table_b, the table of the
 * n_cases - m_cases cases and n_ctrls - m_ctrls controls left; table_b NULL = half B is not scored.  Cells a table does not
 * have read as -1, as in gcre_set_value_table.  With m = (n_cases, n_ctrls) and table_a the context's table every A score is
 * the observed score bit for bit; with m = (0, 0) and table_b the context's table every B score is.
 * Counts, as doubles, a NaN on either side never counting; cut [n_sets][n_cut] holds every set's own cut-offs:
 *   n_a[s][j]    = #{b : A_sb >= cut[s][j]}
 *   n_b[s][j]    = #{b : B_sb >= cut[s][j]}
 *   n_both[s][j] = #{b : A_sb >= cut[s][j] and B_sb >= cut[s][j]}
 * all [n_sets][n_cut]; n_b and n_both may be NULL also with table_b.  A set with an NA member gets -1 in every count and NaN
 * rows in scores_a / scores_b, optional [n_sets][draws].  draws == 0: zeros, nothing of this stage launched.
 * The draws are walked in slabs of whole 512-draw tiles; a slab's masks and its optional outputs on the device stay under
 * GCRE_SUBSAMPLE_MAX_MB (environment, read per call, default 1024; one tile at the least; GCRE_SUBSAMPLE_SLAB_DRAWS bounds
 * a slab further).  The counts are integer sums and every draw belongs to one slab: no result depends on the slabs.
 * Errors, nothing launched and no output array written (*n_out as gcre_score_sets leaves it): everything gcre_score_sets
 * refuses; GCRE_ERR_ARG -- draws < 0, m_cases outside 0 .. n_cases, m_ctrls outside 0 .. n_ctrls, NULL table_a, a table
 * without a row or a column, n_cut outside 0 .. GCRE_SUBSAMPLE_MAX_CUTS, n_cut > 0 with NULL cut or NULL n_a, n_b / n_both /
 * scores_b without table_b, a NaN in cut, the optional outputs of one 512-draw tile above GCRE_SUBSAMPLE_MAX_MB.
 * The counts are selection frequencies under subsampling of THIS cohort: descriptive, no p-value and no family-wise
 * statement.  n_both / n_a says how often the untouched half confirms a selection only if neither the sets nor the cuts
 * were chosen on the full cohort's labels; otherwise it is optimistic. */
#define GCRE_SUBSAMPLE_MAX_CUTS 8
int gcre_score_sets_subsample(gcre_ctx* ctx, const gcre_set_input* in, int32_t m_cases, int32_t m_ctrls, int64_t draws,
                              uint64_t seed, const double* table_a, int nrow_a, int ncol_a, const double* table_b, int nrow_b,
                              int ncol_b, const double* cut, int32_t n_cut, gcre_set_score* out, int64_t cap, int64_t* n_out,
                              int64_t* n_a, int64_t* n_b, int64_t* n_both, double* scores_a, double* scores_b);
/* k_table_to_diag / k_subsample_masks / k_subsample_null launches of gcre_score_sets_subsample on the context since
 * gcre_create -- one per table, then two per slab of draws (no other launch counter counts them, nor the reverse); -1 for a
 * NULL context. */
int64_t gcre_subsample_launches(const gcre_ctx* ctx);

/* Multi-hit tests of the given sets: are the patients who carry AT LEAST m members of a set enriched in
 * cases?  Every other set statistic scores the union of a set's members, where a patient with one hit and one with four
 * count the same.  The best score over the caller's levels m is the statistic, and the same maximum is taken under every
 * permutation, so that the selection of m is paid for inside the null.  `out`, *n_out: exactly what gcre_score_sets gives
 * for the full sets, so one call yields both p-values.
 * Levels.  `levels` holds n_levels (1 .. GCRE_DOSE_MAX_LEVEL) strictly ascending integers in 1 .. GCRE_DOSE_MAX_LEVEL; the same
 * levels apply to every set.  Level row i of set s, within the context's n patients:
 *   method 1: the patients who carry at least levels[i] of the set's listed members, whatever the signs; a member listed
 *             twice counts twice
 *   method 2: a (+) half, the patients who carry at least levels[i] of the (+) members, and a (-) half, the same over the (-)
 *             members: two independent counts
 * and is scored as gcre_score_sets scores a set with these union rows: the same counts (the (-) half the other way round),
 * the same f64 observed expression, the same f32 null value N[row][r] (NaN and negatives folded to 0).  Level 1 is the set's
 * union rows, bit for bit; a level above the number of members is an empty row, scored like any row of non-carriers.
 *   score        = the observed score of level row best_index
 *   best_index   = the smallest index that attains the maximum of the observed level scores, NaN levels skipped (-1 and a
 *                  NaN score if every level is NaN)
 *   best_level   = levels[best_index] (0 for NaN); levels = n_levels
 *   cases_pos .. ctrls_neg = the counts of that level row (zeros for NaN)
 *   T[s][r]      = max over the levels of set s of N[row][r]
 *   n_ge         = #{r < iterations : (double)T[s][r] >= score}; 0 for a NaN score, -1 for an invalid set (an NA member)
 * iterations == 0: nothing of this stage is launched; every record keeps `levels`, n_ge = 0 (-1 for an invalid set), a NaN
 * score, best_index = -1 and best_level = 0.  An invalid set has a NaN score, best_index = -1, best_level = 0.
 * family_max, optional [iterations]: max of T[s][r] over the valid sets (all zeros without one).  null_max, optional
 * [n_sets][iterations] = T (NaN rows for invalid sets).  level_scores, optional [n_sets][n_levels]: the observed score of
 * every level row, NaN for invalid sets.
 * The level rows are built on the device (k_dose_rows: a bit-sliced count per patient, compared with every level) from the
 * gene rows and the set list, uploaded once.  The valid sets are walked in slabs of whole sets whose level rows -- and
 * null_max rows, when asked -- stay under GCRE_PREFIX_MAX_MB on the device (environment, read per call, default 1024;
 * GCRE_PREFIX_SLAB_SETS bounds a slab further); no result depends on the slabs.
 * Errors, nothing launched and no output array written (*n_out as gcre_score_sets leaves it): everything gcre_score_sets
 * refuses; GCRE_ERR_ARG -- NULL dose_out, n_levels outside 1 .. GCRE_DOSE_MAX_LEVEL, NULL levels, a level outside
 * 1 .. GCRE_DOSE_MAX_LEVEL, levels not strictly ascending, one valid set whose level rows (and null_max row) exceed
 * GCRE_PREFIX_MAX_MB.
 * n_ge / iterations is a self-contained permutation p-value of the maximum over the caller's levels, one set at a time; the
 * levels must not be chosen from the labels.  Not built: step-down, min-P and competitive nulls of this statistic, levels
 * above 15, per-gene weights, doses that count alleles. */
#define GCRE_DOSE_MAX_LEVEL 15
typedef struct {
  double score;
  int64_t n_ge;
  int32_t best_index, best_level, levels;
  int32_t cases_pos, ctrls_pos, cases_neg, ctrls_neg;
  int32_t pad;
} gcre_dose_score;
int gcre_score_sets_dose(gcre_ctx* ctx, const gcre_set_input* in, const int32_t* levels, int32_t n_levels,
                         gcre_set_score* out, int64_t cap, int64_t* n_out,
                         gcre_dose_score* dose_out      /* [n_sets] */,
                         float* family_max              /* optional [iterations] */,
                         float* null_max                /* optional [n_sets][iterations] */,
                         double* level_scores           /* optional [n_sets][n_levels] */);
/* k_dose_rows / k_set_observed / k_prefix_pick / k_prefix_null launches of gcre_score_sets_dose on the context since
 * gcre_create (no other launch counter counts them, nor the reverse); -1 for a NULL context. */
int64_t gcre_dose_launches(const gcre_ctx* ctx);

/* Sequential permutation p-values of the given sets (Besag & Clifford 1991, the adaptive permutation of
 * PLINK): every set is permuted until its null score has reached its observed score `h` times, then it stops; the p-value is
 * n_hit / n_perm.  A set that is plainly null stops after about h / p permutations, an interesting one runs on to max_perms,
 * which may be far above what a context can hold: the masks are drawn in batches as they are needed and are never resident
 * as a whole, and the context's own masks are not read -- a context with iterations == 0 is the usual one.
 * `out`, *n_out: exactly what gcre_score_sets gives on this context (n_ge / pvalue against the context's own masks), so one
 * call yields both.
 * Definition, independent of the batches.  mask_r, 0 <= r < max_perms (r is 64-bit), is the mask gcre_generate_perm_masks(seed,
 * stratum, n_strata) gives permutation r, bit for bit: base_r = gcre_mix64(seed ^ (0x51ed270b7f3c9a1d * (r + 1))), patient c in
 * column order reads u = gcre_mix64(base_r + c) and becomes a case when floor(u rem / 2^64) < need, rem the patients of its
 * stratum not yet walked (c included) and need the cases of the stratum still to be placed.  No tag in between: for r below a
 * context's iterations these are the context's generated permutations.  With null_s(mask) the f32 null score of
 * gcre_score_sets (above) and score_s the observed score,
 *   e_s[r] = ((double)null_s(mask_r) >= score_s)              a NaN score never counts
 * If e_s has at least h ones in [0, max_perms): n_perm = the 1-based position of the h-th one, n_hit = h, stopped = 1.
 * Otherwise n_perm = max_perms, n_hit = the number of ones, stopped = 0.  A set with an NA member gets n_hit = n_perm = -1
 * and stopped = 0.  max_perms == 0: nothing of this stage is launched, every valid set gets zeros.
 * The outputs are integers and a pure function of (sets, rows, signs, table, seed, strata, h, max_perms).  Batches are whole
 * 512-permutation tiles: the first holds 4,096 permutations, every later one four times the one before, up to the tiles whose
 * masks and bit rows (one bit per active set and permutation) stay under GCRE_SEQ_MAX_MB on the device (environment, read per
 * call, default 1024; one tile at the least); GCRE_SEQ_BATCH_PERMS bounds a batch further.  Neither they, nor the order of the
 * active list, nor the launch shape change a value.
 * Errors, nothing launched and no output array written (*n_out as gcre_score_sets leaves it): everything gcre_score_sets
 * refuses; GCRE_ERR_ARG -- NULL seq_out, h outside 1 .. 2^31 - 1, max_perms outside 0 .. 2^40, `stratum` with n_strata < 1;
 * GCRE_ERR_RANGE -- a stratum id outside 0 .. n_strata-1.
 * n_hit / n_perm is a nominal p-value, one set at a time, with a relative error of about 1 / sqrt(h) wherever it is above
 * h / max_perms; for the sets that did not stop, (n_hit + 1) / (n_perm + 1) is the usual conservative estimate.  The sets stop
 * at different permutations, so there is no common null matrix.  Not built: family-wise versions (max-T, step-down, min-P) of
 * it, sequential stopping of the competitive statistics and of the joins (the prefix and dose statistics:
 * gcre_score_sets_prefix_sequential, below), an early stop for sets that are clearly significant. */
typedef struct {
  int64_t n_hit;       /* exceedances counted: h when stopped; -1 for an invalid set */
  int64_t n_perm;      /* permutations used: the position of the h-th exceedance, or max_perms; -1 for an invalid set */
  int32_t stopped;     /* 1: the h-th exceedance was reached */
  int32_t pad;
} gcre_seq_score;
int gcre_score_sets_sequential(gcre_ctx* ctx, const gcre_set_input* in, uint64_t seed, const int32_t* stratum, int n_strata,
                               int64_t h, int64_t max_perms, gcre_set_score* out, int64_t cap, int64_t* n_out,
                               gcre_seq_score* seq_out /* [n_sets] */);
/* k_seq_masks / k_seq_null / k_seq_retire launches of gcre_score_sets_sequential on the context since gcre_create -- three
 * per batch (no other launch counter counts them, nor the reverse); -1 for a NULL context. */
int64_t gcre_sequential_launches(const gcre_ctx* ctx);

/* Stratified set scores (the Cochran-Mantel-Haenszel idea): every stratum of the cohort -- a sub-cohort, a
 * sex, an ancestry cluster -- is scored on its own counts against the value table of ITS cases and controls, the terms are
 * summed, and the same sum is taken under every permutation of the context.  gcre_generate_perm_masks(seed, stratum) keeps a
 * pooled p-value valid when case fraction and carrier frequency both differ between the strata, but the pooled SCORE of a
 * gene that is merely commoner in the case-rich stratum is large under the observed labels and under every such permutation
 * alike; this sum is not.  `out`, *n_out: exactly what gcre_score_sets gives (the pooled score), so one call yields both.
 * Inputs.  stratum [n]: ids 0 .. n_strata-1, n_strata 1 .. GCRE_STRATA_MAX; Z_s = the patients of stratum s, with cases_s of
 * them among the columns < n_cases.  One raw row-major value table per stratum: T_s = tables + tab_off[s], nrow[s] x ncol[s],
 * at least 1 x 1, the table of a cohort of cases_s cases and |Z_s| - cases_s controls; cells it does not have read as -1,
 * as in gcre_set_value_table.  The context's own table is read only for `out`.
 * Definition.  With P, N the unions gcre_score_sets defines (method 1: one union alone) and a label mask m -- the observed
 * labels (the columns < n_cases), or the mask of permutation r:
 *   term_s(m) = T_s[ |P & Z_s & m| ][ |P & Z_s \ m| ]   method 2:  + T_s[ |N & Z_s \ m| ][ |N & Z_s & m| ], added in this order
 *   score(m)  = ((+0.0 + term_0) + term_1) + ...         ascending s, f64, additions only
 *   score     = score(observed);   n_ge = #{r < iterations : score(mask_r) >= score}   as doubles, a NaN on either side
 *               never counting; -1 for an invalid set (an NA member), whose score is NaN
 * terms, optional [n_sets][n_strata]: term_s(observed), NaN rows for invalid sets.  counts, optional [n_sets][n_strata][4]:
 * cases_pos, ctrls_pos, cases_neg, ctrls_neg of the set inside every stratum, as gcre_set_score counts them (zeros for
 * invalid sets).  null_scores, optional [n_sets][iterations]: score(mask_r), NaN rows for invalid sets.  family_max, optional
 * [iterations]: the maximum over the valid sets of score(mask_r), a NaN or negative score entering as +0 (all zeros without
 * a valid set).  iterations == 0: score, terms and counts as above, n_ge = 0.
 * The masks must keep the strata: a look-up outside "cases_s cases in stratum s" means nothing, so every resident mask is
 * counted against every Z_s on the device first, and a context whose masks were not drawn by gcre_generate_perm_masks with
 * these strata (or set by the caller to the same effect) is refused with GCRE_ERR_ARG.  This one refusal comes after
 * launches: `out` holds gcre_score_sets' records, every output of this stage its defaults (NaN scores, n_ge 0 / -1).
 * The valid sets are walked in slabs of whole sets whose stratum rows -- and null_scores rows, when asked -- stay under
 * GCRE_STRATA_MAX_MB on the device (environment, read per call, default 1024; one set at the least; GCRE_STRATA_SLAB_SETS
 * bounds a slab further); no result depends on the slabs.
 * Errors, nothing launched and no output array written (*n_out as gcre_score_sets leaves it): everything gcre_score_sets
 * refuses; GCRE_ERR_ARG -- NULL px_out, NULL stratum, n_strata outside 1 .. GCRE_STRATA_MAX, NULL tables / nrow / ncol /
 * tab_off, a table without a row or a column, one 512-permutation tile of null_scores above GCRE_STRATA_MAX_MB;
 * GCRE_ERR_RANGE -- a stratum id outside 0 .. n_strata-1.
 * n_ge / iterations is a nominal permutation p-value of the summed score, one set at a time.  The terms and counts are
 * descriptive; no test of heterogeneity between the strata is attached.  Not built: stratified joins, weights per stratum,
 * stratified prefix / dose / sequential / min-P statistics, more than 16 strata. */
#define GCRE_STRATA_MAX 16
typedef struct {
  double score;        /* the sum of the observed terms; NaN for an invalid set */
  int64_t n_ge;        /* permutations whose sum reaches it; -1 for an invalid set */
} gcre_strata_score;
int gcre_score_sets_strata(gcre_ctx* ctx, const gcre_set_input* in, const int32_t* stratum, int32_t n_strata,
                           const double* tables, const int32_t* nrow, const int32_t* ncol, const int64_t* tab_off,
                           gcre_set_score* out, int64_t cap, int64_t* n_out,
                           gcre_strata_score* px_out      /* [n_sets] */,
                           double* terms                  /* optional [n_sets][n_strata] */,
                           int32_t* counts                /* optional [n_sets][n_strata][4] */,
                           double* null_scores            /* optional [n_sets][iterations] */,
                           double* family_max             /* optional [iterations] */);
/* Kernels gcre_score_sets_strata launched for its own stage on the context since gcre_create: k_strata_masks, the check of
 * the masks (with permutations), one k_table_to_diag per stratum, then k_strata_rows, k_strata_observed and (with
 * permutations) k_strata_null per slab (no other launch counter counts them, nor the reverse); -1 for a NULL context. */
int64_t gcre_strata_launches(const gcre_ctx* ctx);

/* Covariate-adjusted permutation masks (Epstein et al. 2012): case labels redrawn with per-patient odds,
 * conditional on the number of cases of every stratum -- Fisher's non-central hypergeometric law with one patient per class.
 * Every statistic of this library is a count over the context's resident masks, so these masks put a continuous covariate
 * (ancestry components, age, depth) into the null of the joins and of every set statistic at once.  The adjustment is on the
 * null, not on the statistic, and the p-values are only as good as the model that gave the odds.
 * Inputs.  odds [n]: one finite double >= 0 per patient column (the cases are the columns < n_cases, as everywhere); stratum
 * [n] or NULL: ids 0 .. n_strata-1, n_strata 1 .. GCRE_STRATA_MAX; Z_s = the patients of stratum s, cases_s of them cases.
 * Target law.  Inside stratum s mask r is a subset A of Z_s with |A| = cases_s and P(A) proportional to the product of odds_c
 * over A; strata are independent.  Equal odds: the uniform law of gcre_generate_perm_masks (NOT its bits).
 * Calibration (host).  Per stratum the tilt t_s is found by bisection so that p_c = t_s odds_c / (1 + t_s odds_c) sums to
 * cases_s, and thr_c = min(floor(p_c 2^32), 2^32 - 1).  From there on the thresholds ARE the definition: what is sampled is
 * conditional Bernoulli with p_c = thr_c / 2^32, exactly.  cases_s = 0: every thr 0; cases_s = the patients of Z_s with
 * positive odds: 2^32 - 1 for those.  | sum thr_c / 2^32 - cases_s | < |Z_s| (2^-32 + 2^-44) + |Z_s|^2 2^-52.
 * The draw is exact rejection in integers.  With
 *   seed'    = gcre_mix64(seed ^ 0x7765696768746564)          key_r   = gcre_mix64(seed' ^ (0x51ed270b7f3c9a1d * (r + 1)))
 *   base_rs  = gcre_mix64(key_r ^ (0xd1b54a32d192ed03 * (s + 1)))      pair_rsj = gcre_mix64(base_rs + j)
 * attempt a = 0, 1, 2, ... of (r, s) reads u = gcre_mix64(pair_rsj + c) with j = a >> 1 for the patient in COLUMN c and labels
 * it a case when the high half of u (a even) or the low half (a odd) is below thr_c.  The accepted attempt a*(r, s) is the
 * SMALLEST a whose case count over Z_s is exactly cases_s; mask r is the union over s of the accepted attempts.  Nothing
 * depends on grid, batch, launch order or memory layout.  About sqrt(2 pi V_s) attempts per (r, s), V_s = sum p (1 - p).
 * max_attempts: a cap (above 2^31 it acts as 2^31), not a tuning knob; 2^20 is a sensible value.  attempts_out, optional
 * [iterations][n_strata] (one column without `stratum`): a*(r, s).
 * iterations == 0, the streams, the transposed copy and the reset of the permutation window: as gcre_generate_perm_masks.
 * Errors, nothing launched: GCRE_ERR_ARG with a message naming the stratum -- NULL odds, an odds value that is negative, NaN
 * or infinite, a stratum with fewer patients of positive odds than cases, n_strata outside 1 .. GCRE_STRATA_MAX, a stratum id
 * out of range, max_attempts < 1; GCRE_ERR_RANGE -- a stratum whose estimate sqrt(2 pi V_s) alone exceeds max_attempts.
 * After the search launch: GCRE_ERR_RANGE saying how many permutations were left over without an accepted attempt below
 * max_attempts; no mask bit was written, and the context's masks, whether it has any, and its window are what they were.
 * Weighted draws in the sequential set scores: gcre_score_sets_sequential_weighted, below.  Not built: weighted draws in the
 * subsample set scores (they make their own masks), weighted urns for decorated p-values, an exact sampler without rejection,
 * odds of +infinity (forced cases). */
int gcre_generate_weighted_masks(gcre_ctx* ctx, uint64_t seed, const double* odds, const int32_t* stratum, int32_t n_strata,
                                 int64_t max_attempts, uint32_t* attempts_out /* optional [iterations][n_strata] */);
/* The thresholds and sqrt(2 pi V_s) alone; host only, no device is touched.  thr_out [n]; expected_attempts_out optional
 * [n_strata] (one entry without `stratum`).  Refuses what the call above refuses of odds and strata; the message is read with
 * a NULL context. */
int gcre_weighted_thresholds(int32_t n, int32_t n_cases, const double* odds, const int32_t* stratum, int32_t n_strata,
                             uint32_t* thr_out, double* expected_attempts_out /* optional [n_strata] */);
/* k_weighted_search / k_weighted_write launches on the context since gcre_create: two per successful call, one for a call
 * that met the cap, none for one refused up front (no other launch counter counts them, nor the reverse); -1 for a NULL
 * context. */
int64_t gcre_weighted_launches(const gcre_ctx* ctx);

/* Weighted sequential p-values: gcre_score_sets_sequential with the covariate-adjusted masks of
 * gcre_generate_weighted_masks, drawn in batches that are never resident as a whole.  A p-value below 1 / iterations under a
 * null that holds a continuous covariate; `out`, *n_out, `seq_out`, h, max_perms, the batches and their environment variables
 * as gcre_score_sets_sequential; odds, stratum, n_strata, max_attempts as gcre_generate_weighted_masks.  A context with
 * iterations == 0 will do.
 * Definition.  mask_r, 0 <= r < max_perms (r is 64-bit), is mask r of gcre_generate_weighted_masks(seed, odds, stratum,
 * n_strata, max_attempts), bit for bit: the same thresholds, a*(r, s) the smallest accepted attempt below the cap.  Let R be the
 * smallest r < max_perms for which some stratum has no accepted attempt below max_attempts (none: infinity).  The rule of
 * gcre_score_sets_sequential is applied to permutations 0 .. min(max_perms, R) - 1.  R >= max_perms: the usual answer.  R <
 * max_perms and every valid set has stopped with n_perm <= R: the answer is complete and returned.  Otherwise -- a set with a
 * NaN score never stops, so it is always among these -- the call is refused with GCRE_ERR_RANGE and a message that names R, the
 * stratum, the cap and how many sets were still active; `out` then holds gcre_score_sets' records and seq_out its defaults
 * (zeros, -1 for an invalid set).  This depends on the inputs alone: not on batch size, schedule or the order of the active
 * list.  No mask at or beyond R is drawn or scored.
 * A batch takes its masks and one dword per stratum and permutation (the accepted attempts) under GCRE_SEQ_MAX_MB.  Each
 * weighted permutation costs about sqrt(2 pi V_s) attempts over the whole stratum, where a uniform one costs one hash per
 * patient.
 * Errors, nothing launched and no output array written: everything gcre_score_sets, gcre_score_sets_sequential (h, max_perms,
 * seq_out) and gcre_generate_weighted_masks (odds, strata, max_attempts, the estimate above the cap) refuse up front, the
 * messages opening with score_sets_sequential_weighted.
 * gcre_sequential_launches counts its kernels -- k_seq_weighted_search, k_seq_weighted_write, k_seq_null, k_seq_retire: four
 * per batch; for a batch cut at R the search alone, or all four when permutations remain in front of R.
 * gcre_weighted_launches does not move.  Not built: family-wise versions, weighted draws in the subsample scores. */
int gcre_score_sets_sequential_weighted(gcre_ctx* ctx, const gcre_set_input* in, uint64_t seed, const double* odds,
                                        const int32_t* stratum, int n_strata, int64_t max_attempts, int64_t h, int64_t max_perms,
                                        gcre_set_score* out, int64_t cap, int64_t* n_out, gcre_seq_score* seq_out /* [n_sets] */);

/* Sequential p-values of the two adaptive set tests: the variable-threshold test (gcre_score_sets_prefix)
 * and the multi-hit test (gcre_score_sets_dose) with permutations drawn in batches as they are needed, every set until the
 * maximum over its steps (levels) has reached its best observed score h times.  No resident mask is read: a context with
 * iterations == 0 will do, and max_perms may be far above what a context holds.
 * `cut` / `levels`, `px_out` / `dose_out`, `step_scores` / `level_scores` as gcre_score_sets_prefix / gcre_score_sets_dose take
 * and fill them, except n_ge: 0 for a valid set, -1 for an invalid one.  seed, stratum, n_strata, h, max_perms, seq_out and the
 * batches as gcre_score_sets_sequential.  odds NULL: its uniform masks (max_attempts is not read).  odds given: the masks,
 * the left-over permutation R and the refusal of gcre_score_sets_sequential_weighted.
 * Definition.  With T_s(mask) = max over the steps k of set s of the f32 null score of step row k (a NaN step of the table still
 * takes part, folded as 0), and score_s the best observed step score (NaN steps skipped), e_s[r] = ((double)T_s(mask_r) >=
 * score_s); then the rule of gcre_score_sets_sequential.  A set whose steps are all NaN has a NaN score: uniform, it keeps
 * zeros; weighted, it never stops and forces the refusal where there is an R.
 * The sets are walked in the slabs of gcre_score_sets_prefix (GCRE_PREFIX_MAX_MB, GCRE_PREFIX_SLAB_SETS); every slab runs the
 * whole sequential loop from permutation 0 and draws the masks again -- they are a function of (seed, r), so no value depends
 * on the slabs, but a second slab pays for the draw a second time.  Weighted: every slab is run, the sets still active at R are
 * summed over the slabs, and the call is refused with GCRE_ERR_RANGE if that sum is positive; seq_out then keeps its defaults.
 * max_perms == 0: nothing of this stage is launched; px_out / dose_out keep a NaN score, seq_out zeros.
 * Errors, nothing launched and no output array written: everything gcre_score_sets, gcre_score_sets_prefix / _dose (without a
 * null_max matrix), gcre_score_sets_sequential and, with odds, gcre_generate_weighted_masks refuse up front.
 * n_hit / n_perm is a nominal p-value of the maximum, one set at a time.  Not built: a family-wise value of it, a group order
 * re-sorted after retirement, an early stop for sets that are clearly significant.
 * gcre_seq_prefix_launches: the kernels of the two entries on the context since gcre_create -- per slab three (rows, observed
 * scores, pick), then three per batch (four weighted; the search alone for a batch with nothing in front of R); no other
 * launch counter counts them, nor the reverse; -1 for a NULL context. */
int gcre_score_sets_prefix_sequential(gcre_ctx* ctx, const gcre_set_input* in, const uint8_t* cut /* [members], optional */,
                                      uint64_t seed, const double* odds /* NULL: uniform */, const int32_t* stratum, int n_strata,
                                      int64_t max_attempts, int64_t h, int64_t max_perms, gcre_set_score* out, int64_t cap,
                                      int64_t* n_out, gcre_prefix_score* px_out /* [n_sets] */, gcre_seq_score* seq_out /* [n_sets] */,
                                      double* step_scores /* [members], optional */);
int gcre_score_sets_dose_sequential(gcre_ctx* ctx, const gcre_set_input* in, const int32_t* levels, int32_t n_levels, uint64_t seed,
                                    const double* odds /* NULL: uniform */, const int32_t* stratum, int n_strata,
                                    int64_t max_attempts, int64_t h, int64_t max_perms, gcre_set_score* out, int64_t cap,
                                    int64_t* n_out, gcre_dose_score* dose_out /* [n_sets] */, gcre_seq_score* seq_out /* [n_sets] */,
                                    double* level_scores /* [n_sets][n_levels], optional */);
int64_t gcre_seq_prefix_launches(const gcre_ctx* ctx);

/* ------------------------------------------------------------------------------------------------------------
 * Carrier overlaps of caller-given sets: which sets are carried by the same patients.  No reference
 * counterpart.
 * Carrier row of set s: C_s = OR of ALL its members, whatever their signs and whatever the context's method (a patient
 * who carries a variant in any gene of the path), bits >= n_cols ignored.
 *   size[s]      = { |C_s & cases|, |C_s & ctrls| }  (cases = columns < n_cases); { -1, -1 } for a set with an NA member
 *   both[i][j]   = { |C_a[i] & C_b[j] & cases|, |C_a[i] & C_b[j] & ctrls| }; { 0, 0 } when either set has an NA member
 * a / b: set indices, repeats allowed; NULL = 0 .. n_sets-1 (then na / nb must be n_sets).  size [n_sets][2] and
 * both [na][nb][2] are int32, either may be NULL.  Needs neither a value table nor permutation masks.
 * The rows are uploaded once and `a` is walked in slabs so that the device output of one launch of k_set_overlap stays
 * under GCRE_OVERLAP_SLAB_MB (environment, default 256; one row of 64 x 64 pair tiles at the least); the results do not
 * depend on it.  Any na, nb >= 0; 0 returns at once.  Errors, nothing launched: GCRE_ERR_ARG -- a NULL argument, n_cols
 * not n_cases + n_ctrls, a set without members, a sign other than +1 / -1; GCRE_ERR_RANGE -- a member row or a set index
 * out of range. */
int gcre_set_overlap(gcre_ctx* ctx, const gcre_set_input* in, const int64_t* a, int64_t na,
                     const int64_t* b, int64_t nb, int32_t* size, int32_t* both);
/* k_set_overlap launches of the context since gcre_create (tests: an argument error launches nothing). */
int64_t gcre_overlap_launches(const gcre_ctx* ctx);

/* ------------------------------------------------------------------------------------------------------------
 * Greedy clumping of caller-given sets by shared carriers, on the device.  No reference counterpart.
 * The sets, their carrier rows, `size` and the shared counts are those of gcre_set_overlap.  `order` [n_order] names the
 * sets to clump, best first, each at most once and none with an NA member.  Walk it: a set not yet assigned becomes the
 * lead of a new clump (ids 0, 1, .. in walk order) and every later unassigned set whose overlap with it is >= r joins;
 * overlap = both / den in f64, correctly rounded, 0.0 where den is 0, with both / |A| / |B| counted over all patients
 * (patients 0) or the cases (1) and den = |A| + |B| - both (measure 0, jaccard) or min(|A|, |B|) (1, containment).
 * Outputs per set: clump [n_sets] the clump id, lead [n_sets] the lead's set index (a lead names itself), value [n_sets]
 * the overlap with the lead (NaN on a lead), shared [n_sets][2] the carriers shared with the lead ((-1, -1) on a lead); a
 * set outside `order` gets -1 / -1 / NaN / (-1, -1).  size [n_sets][2], optional, as gcre_set_overlap fills it.
 * No pair count leaves the device.  Errors, nothing launched: what gcre_set_overlap refuses of the set list; GCRE_ERR_ARG
 * -- r outside (0, 1] or NaN, measure or patients not 0 or 1, a set listed twice, a listed set with an NA member,
 * n_order x the bytes of a device row (the patients as bits, padded to 128 bytes) above GCRE_CLUMP_MAX_MB (environment,
 * read per call, default 32768); GCRE_ERR_RANGE -- an order entry out of range.  n_order == 0 launches nothing. */
int gcre_clump_sets(gcre_ctx* ctx, const gcre_set_input* in, const int64_t* order, int64_t n_order, double r,
                    int measure, int patients, int32_t* size, int64_t* clump, int64_t* lead, double* value,
                    int32_t* shared);
/* kernels launched by gcre_clump_sets on the context since gcre_create (tests: a refusal launches nothing). */
int64_t gcre_clump_launches(const gcre_ctx* ctx);

/* ------------------------------------------------------------------------------------------------------------
 * Carrier tallies of caller-given sets: how many of the listed sets each patient carries.  No reference
 * counterpart.  Exact integer counts, descriptive only: no test statistic; the carriers of sets that were selected on
 * the case / control labels are enriched in cases by construction.
 * Entry i names set s = which[i]; repeats are allowed and a set listed twice is counted twice; which = NULL means
 * 0 .. n_sets-1, and then n_which must be n_sets.  group [n_which]: the group of entry i, -1 .. n_groups-1, -1 = not
 * counted; NULL = everything in group 0, and then n_groups must be 1.  Planes H = 1 + by_sign:
 *   by_sign 0: the one plane is the carrier row C_s gcre_set_overlap defines (the OR of ALL members, whatever their signs
 *              and the context's method, bits >= n_cols ignored);
 *   by_sign 1: plane 0 is P_s, the OR of the +1 members, plane 1 is N_s, the OR of the -1 members, read from `signs`
 *              whatever the context's method, without conflict removal (as gcre_score_sets states for method 2);
 *              signs = NULL: everything is in P.
 *   counts[g][h][q] = #{ i : group[i] == g, set which[i] has no NA member, bit q of plane h of set which[i] }
 *                     int32 [n_groups][H][n_cols]
 *   group_sets[g], optional [n_groups]: the entries counted into group g
 *   *skipped, optional: the entries with group >= 0 whose set has an NA member: their carriers are not known, they are
 *                     counted nowhere
 * Needs neither a value table nor permutation masks.  The gene rows, a member table and a segment list go up once;
 * k_set_patient_counts adds the rows up in bit-sliced counters, one wave per (segment of one group's entries, 2,048
 * patients).  Segments hold at most GCRE_PATIENT_SEG entries (environment, read per call; default: what spreads the call
 * over about 4,096 waves, 64 to 1,024 entries); the results do not depend on it.  n_which == 0, or every entry -1 or NA,
 * launches nothing and writes zeros.
 * Errors, nothing launched: what gcre_set_overlap refuses of the set list; GCRE_ERR_ARG -- by_sign not 0 or 1,
 * n_groups < 1, n_which < 0, NULL `which` with n_which != n_sets, NULL `group` with n_groups != 1, NULL counts,
 * n_which >= 2^31 - 16 (a 32-bit cell cannot overflow), n_groups x H x n_cols x 4 bytes (or the member table) above
 * GCRE_PATIENT_MAX_MB (environment, read per call, default 1024); GCRE_ERR_RANGE -- a `which` entry outside
 * 0 .. n_sets-1, a `group` entry outside -1 .. n_groups-1. */
int gcre_set_patient_counts(gcre_ctx* ctx, const gcre_set_input* in, const int64_t* which, int64_t n_which,
                            const int32_t* group, int32_t n_groups, int by_sign, int32_t* counts,
                            int64_t* group_sets, int64_t* skipped);
/* kernels launched by gcre_set_patient_counts on the context since gcre_create (tests: a refusal launches nothing). */
int64_t gcre_patient_launches(const gcre_ctx* ctx);

/* ------------------------------------------------------------------------------------------------------------
 * Burden tests of per-patient weights: permutation p-values of a weighted sum over the cases.  No
 * reference counterpart.  weights int32 [n_rows][n_cols], every one >= 0, n_cols = n_cases + n_ctrls of the context,
 * columns < n_cases are the cases: a row of gcre_set_patient_counts' counts, or any other non-negative integer load.
 * For every row g and every one of the context's `iterations` permutation masks (all of them: the window of
 * gcre_set_perm_window is the joins' business; strata come in through the masks):
 *   total     = sum_q w[g][q]
 *   observed  = sum_{q < n_cases} w[g][q]
 *   null[g][r]= sum_{q : bit q of mask r} w[g][q]          int64, exact: below 2^47
 *   n_ge      = #{ r : null[g][r] >= observed }            the upper tail; a tie counts in both tails
 *   n_le      = #{ r : null[g][r] <= observed }            the lower tail
 *   p_upper   = n_ge / iterations, p_lower = n_le / iterations (R/ProcessPaths.R:316's rule); NaN at 0 iterations
 *   planes    = the bit length of the row's largest weight: the bit planes the device reads of it
 * null_sums, optional [n_rows][iterations]: every null sum.  Where every mask holds the same number of cases the sum
 * orders the permutations as the difference of the mean load of cases and controls does.
 * A p-value on weights that were selected on these very labels -- the tallies of a run's own significant paths -- is
 * meaningless: tally in a second cohort, or over sets chosen without the labels (gene sets).
 * The weights go up in slabs of rows whose planes and sums stay under GCRE_BURDEN_MAX_MB (environment, read per call,
 * default 1024; GCRE_BURDEN_SLAB_ROWS bounds the rows of a slab: tests); the results do not depend on the slabs.
 * k_burden_planes cuts the rows into bit planes, k_burden_null adds 2^b popcount(plane_b & mask) into 64-bit sums with
 * integer atomics, k_burden_finish counts the tails.  n_rows == 0 returns at once; iterations == 0 fills total,
 * observed and planes, zero counts and NaN, and launches nothing; a row of zeros has planes = 0 and
 * n_ge = n_le = iterations, and nothing is launched for it.
 * Errors, nothing launched: GCRE_ERR_ARG -- NULL out, n_rows < 0, NULL weights with n_rows > 0, n_cols other than
 * n_cases + n_ctrls, a negative weight, one row's planes and sums above GCRE_BURDEN_MAX_MB; GCRE_ERR_ASSERT --
 * iterations > 0 and no permutation masks set. */
typedef struct { int64_t total, observed, n_ge, n_le; int32_t planes; double p_upper, p_lower; } gcre_burden;
int gcre_patient_burden(gcre_ctx* ctx, const int32_t* weights, int64_t n_rows, int32_t n_cols, gcre_burden* out,
                        int64_t* null_sums);
/* kernels launched by gcre_patient_burden on the context since gcre_create (tests: a refusal launches nothing). */
int64_t gcre_burden_launches(const gcre_ctx* ctx);

/* ------------------------------------------------------------------------------------------------------------
 * Per-gene best-path table: for every gene, the best joined path of a join that runs through it.  No
 * reference counterpart (it keeps the top K of a level and nothing else).  A join's inspector leaves the observed score,
 * operand rows, cases and controls of EVERY joined path on the device; a tally armed for the join folds them, chunk by
 * chunk, into one entry per gene slot before they are overwritten.  Nothing is rescored, the join's own result does not
 * change, and a join without a tally launches exactly what it launched before.
 *
 * A joined path with ordinal p = path_idx[i] + j (uid row i, j < count[i]) has src = i and trg = location[i] + j (Score.src
 * / .trg) and touches the slots genes0[src][0..w0) and genes1[trg][0..w1) (-1 = none; a slot listed twice counts once).
 * Per slot the tally keeps the touching path with the largest observed score, ties to the smallest ordinal (the rule of
 * the top-k lists); only paths the join scores count (gcre_join_opts.sharded: the shard), and only scores above -inf.
 * The table is bit-identical whatever the chunking, the inspection cache, the launch-ahead chain, the permutation window
 * or the null kernel form.  A level's null_max bounds every entry of that level: #{null_max >= score} / K is a family-wise
 * p-value over all paths of the length, the number a top-k row gets. */
typedef struct gcre_gene_tally gcre_gene_tally;

/* genes0: [n_rows0][w0] int32 slots of the rows of paths0 (n_rows0 must equal the uid rows of the join it is armed for),
 * genes1: [n_rows1][w1] of the rows of paths1 (n_rows1 must exceed every paths1 row the join reads); w 1..3, values
 * -1..n_slots-1.  NULL for a table = that operand contributes no gene (level 1 and 2: paths0).  The tables are copied.
 * NULL on error (GCRE_ERR_ARG with a message: nothing is launched on a malformed table).  Several joins may fold into one
 * tally when their ordinals mean the same paths (the shards of one join). */
gcre_gene_tally* gcre_gene_tally_create(gcre_ctx* ctx, int32_t n_slots, const int32_t* genes0, int64_t n_rows0, int32_t w0,
                                        const int32_t* genes1, int64_t n_rows1, int32_t w1);
/* The next gcre_join / gcre_join_uids call on the context folds into `tally`, then the context is disarmed (whether the
 * join succeeds or not).  NULL disarms.  The row counts are checked against the join before anything is launched. */
int gcre_join_set_tally(gcre_ctx* ctx, gcre_gene_tally* tally);
/* The same for the next gcre_process_paths call: level = index into gcre_pp_input.level (0..5 = 1a, 1b, 2, 3, 4, 5).
 * A call that is one device of several (shard_world > 1, which is how gcre_process_paths_devices runs its contexts)
 * refuses an armed tally with GCRE_ERR_ARG: merging tallies across devices is left to callers of the join interface. */
int gcre_process_paths_set_tally(gcre_ctx* ctx, int level, gcre_gene_tally* tally);
/* Waits for the folds in flight, then one entry per slot (any output may be NULL): score -inf, ordinal / src / trg -1 and
 * counts 0 where no scored path touches the slot. */
int gcre_gene_tally_read(gcre_gene_tally* tally, double* score, int64_t* ordinal, int32_t* src, int32_t* trg,
                         int32_t* cases, int32_t* ctrls);
void gcre_gene_tally_free(gcre_gene_tally* tally);   /* gcre_destroy frees the ones still alive */

/* ------------------------------------------------------------------------------------------------------------
 * Null exceedance counts: for a list of thresholds, how many (joined path, permutation) pairs of a join
 * have a null score at or above each one, and how many joined paths an observed score.  No reference counterpart: every
 * p-value of the reference is against the per-permutation MAXIMUM over the paths (family-wise); these counts give the
 * other standard permutation answer -- exceed / B = the expected number of paths a permutation pushes past a score (the
 * per-family error rate), and with `observed` the permutation FDR and q-values (report.fdr_columns).
 *
 *   null[p][r]   the f32 value the join's null kernels fold into their maxima for joined path p and permutation r, as
 *                stated for gcre_score_sets above (NaN and negatives fold to 0)
 *   exceed[j]    #{(p, r) : p scored by the join, r in the permutation window, (double)null[p][r] >= thresholds[j]}
 *   observed[j]  #{p scored by the join : observed score of p >= thresholds[j]}, scores above -inf only
 * "scored by the join" is the shard of a sharded join, every joined path otherwise.  Both are sums: shards and permutation
 * windows add.  Unlike the gene tally the object is NOT idempotent -- a join counted twice is counted twice --, so it
 * records how many permutations and joined paths went into it.  The counts are bit-identical whatever the chunking, the
 * inspection cache, the launch-ahead chain or the form of the join's own null kernel, and the join's result does not
 * change; a join without an object launches exactly what it launched before. */
typedef struct gcre_exceed gcre_exceed;

/* thresholds: [m] doubles in any order, copied; 1 <= m <= 10,000 (the top_k limit).  +-inf are allowed.  NULL on error
 * (GCRE_ERR_ARG with a message: m out of range, a NaN threshold). */
gcre_exceed* gcre_exceed_create(gcre_ctx* ctx, const double* thresholds, int32_t m);
/* The next gcre_join / gcre_join_uids call on the context counts into `x`, then the context is disarmed (whether the join
 * succeeds or not).  NULL disarms.  A tally and an exceed object may be armed for the same join. */
int gcre_join_set_exceed(gcre_ctx* ctx, gcre_exceed* x);
/* The same for the next gcre_process_paths call, level 0..5 as for the tally.  The call counts the null values of every
 * permutation window it walks (perms_counted grows by `iterations`) and the observed scores once.  One device of several
 * (shard_world > 1) refuses an armed object with GCRE_ERR_ARG. */
int gcre_process_paths_set_exceed(gcre_ctx* ctx, int level, gcre_exceed* x);
/* Waits for what is in flight.  exceed / observed: [m] in the order of the thresholds given (either may be NULL).
 * perms_counted: the sum of the window lengths of the joins counted; paths_counted: the joined paths whose observed scores
 * were counted. */
int gcre_exceed_read(gcre_exceed* x, uint64_t* exceed, uint64_t* observed, int64_t* perms_counted, int64_t* paths_counted);
int gcre_exceed_reset(gcre_exceed* x);   /* all counts back to zero */
void gcre_exceed_free(gcre_exceed* x);   /* gcre_destroy frees the ones still alive */

/* Per-permutation counts: next to exceed[j], the distribution over the permutations it is the sum of,
 *   V[j][r] = #{p scored by the join : (double)null[p][r] >= thresholds[j]},   r = 0 .. iterations-1 (absolute, whatever
 * the permutation window), from which report.false_count_columns takes k-FWER, the median and the (1 - alpha) bound of the
 * number of false positives.  on != 0 allocates and zeroes the device array (u32 [m][iterations rounded up to 2048]);
 * 0 frees it.  GCRE_ERR_ARG with a message: after anything was counted into x (gcre_exceed_reset lifts this), a context
 * with 0 iterations, m x iterations above 2^26 (256 MB of cells), an object of another (or a destroyed) context.  Counts
 * add as exceed does: shards cell by cell, windows fill disjoint ranges, a join counted twice is counted twice.  A cell is
 * 32 bits wide: a count that would take the joined paths counted into one permutation's cells past 2^32-1 is refused before
 * any launch with GCRE_ERR_RANGE (reset first).  An object without them launches exactly what it launched before. */
int gcre_exceed_keep_perm_counts(gcre_exceed* x, int on);
/* Waits for what is in flight.  out: [m][iterations], row j in the order of the thresholds given; equal thresholds get
 * equal rows; permutations no counted join's window covered read 0; every row sums to exceed[j].  GCRE_ERR_ARG when x
 * keeps no per-permutation counts. */
int gcre_exceed_read_perm_counts(gcre_exceed* x, uint64_t* out /* [m][iterations] */);

/* Step-down max-T (Westfall & Young 1993, Alg. 4.1): the family-wise p-values of a level's top rows with
 * the better rows taken out of the family.  x keeps per-permutation counts and was counted over exactly one full pass of one
 * join (perms_counted == iterations); its m thresholds are observed scores of joined paths of that join, all finite.
 * in->n_sets == m, and set j IS the joined path whose observed score is threshold j: its members are the path's rows, signed
 * as for gcre_score_sets.  With D_j = the sets whose threshold is strictly above threshold j (compared as doubles: tied rows do
 * not exclude one another) and null[p][r] as stated for gcre_score_sets,
 *   n_ge[j] = #{r < iterations : max over the join's paths p outside D_j of (double)null[p][r] >= thresholds[j]}
 * -- the raw step-down p-value is n_ge[j] / iterations; report.stepdown_columns takes the monotone step.  It is computed as
 * V[j][r] - E[j][r] >= 1: V the counts x holds, E[j][r] = #{i in D_j : (double)null[i][r] >= thresholds[j]} from
 * k_stepdown_null over the m sets, compared by k_stepdown_finish.  n_ge[j] never exceeds #{r : null_max[r] >= thresholds[j]}
 * and equals it for the best row.  x is not changed: calling it twice gives the same answer.
 * Waits for what is in flight.  Errors before any launch: GCRE_ERR_ARG -- x keeps no per-permutation counts, nothing or not
 * exactly one full pass was counted, x not among its context's live objects (the check gcre_exceed_keep_perm_counts makes: the
 * call takes no context of its own, so there is no other one to belong to), n_sets != m, a threshold that is not finite, an NA
 * member; and everything gcre_score_sets refuses.  After k_set_observed and before the two kernels: GCRE_ERR_ARG naming the
 * first set whose observed score is not its threshold bit for bit (the rows must be the rows the thresholds came from).  After
 * them: GCRE_ERR_ASSERT "the sets are not distinct joined paths of the counted join" when some permutation counts more
 * top rows than joined paths at a threshold (n_ge is then not written).  Memory: m x iterations (rounded up to 2048) u32 cells,
 * freed on return. */
int gcre_exceed_stepdown(gcre_exceed* x, const gcre_set_input* in, int64_t* n_ge /* [m] */);
/* k_stepdown_null / k_stepdown_finish launches of the context since gcre_create (tests: a refusal launches nothing). */
int64_t gcre_stepdown_launches(const gcre_ctx* ctx);

/* ------------------------------------------------------------------------------------------------------------
 * Hit lists: every joined path of a join whose observed score reaches a cut-off -- the rows a top-K list
 * would hold if K were unbounded and the list ended at the cut-off.  No reference counterpart: the reference reports the
 * top_k <= 10,000 best rows of a level and nothing below them.  With the cut-off report.significance_cutoff takes from a
 * level's null maxima the list is "everything significant at family-wise level alpha", however long.
 *
 *   hits   {p scored by the join : observed score of p >= cutoff}, compared as doubles, scores above -inf only
 * (a cut-off of either zero admits scores of both zeros; -inf admits every score; NaN and -inf scores are never hits).
 * "scored by the join" is the shard of a sharded join, every joined path otherwise.  A record is the path's ordinal
 * (path_idx[i] + j for uid row i), its score, src / trg as in a top-k list (Score.src / .trg: the uid row i and
 * location[i] + j), cases and controls.  The list ADDS: shards of one join append into one list, and -- like the
 * exceedance counts, unlike the gene tally -- it is NOT idempotent: a join collected twice is listed twice
 * (gcre_hits_reset starts over), so it records how many joined paths were looked at.  A list needs no permutations
 * (0 iterations work) and may be armed together with a tally and an exceed object.  The list and the count are identical
 * whatever the chunking, the inspection cache, the launch-ahead chain, the permutation window or the form of the join's
 * null kernel, and the join's result does not change; a join without a list launches exactly what it launched before.
 * Overflow: `found` counts every hit, also those beyond `cap`; a list that overflowed cannot be read (which records it
 * kept is not defined) -- reset it, or make a larger one, and collect again. */
typedef struct gcre_hits gcre_hits;

/* cutoff: any double but NaN (+-inf are allowed).  cap: records the list can hold, 1 .. 2^26; 32 x cap bytes of device
 * memory are allocated here.  NULL on error (GCRE_ERR_ARG with a message: a NaN cut-off, cap out of range; GCRE_ERR_DEVICE:
 * no memory). */
gcre_hits* gcre_hits_create(gcre_ctx* ctx, double cutoff, int64_t cap);
/* The next gcre_join / gcre_join_uids call on the context appends to `h`, then the context is disarmed (whether the join
 * succeeds or not).  NULL disarms. */
int gcre_join_set_hits(gcre_ctx* ctx, gcre_hits* h);
/* The same for the next gcre_process_paths call, level 0..5 as for the tally.  The call collects the level once, not once
 * per permutation window.  One device of several (shard_world > 1) refuses an armed list with GCRE_ERR_ARG. */
int gcre_process_paths_set_hits(gcre_ctx* ctx, int level, gcre_hits* h);
/* Waits for what is in flight.  found: joined paths at or above the cut-off (may exceed cap); paths: joined paths looked
 * at.  Either may be NULL. */
int gcre_hits_count(gcre_hits* h, int64_t* found, int64_t* paths);
/* Waits for what is in flight.  n must equal `found` (GCRE_ERR_ARG otherwise); GCRE_ERR_RANGE when found > cap.  On error
 * the outputs are untouched.  Records come best first: score descending as doubles (+-0 tie), then ordinal ascending --
 * the tie rule of the top-k lists.  Any output may be NULL. */
int gcre_hits_read(gcre_hits* h, int64_t n, double* score, int64_t* ordinal, int32_t* src, int32_t* trg,
                   int32_t* cases, int32_t* ctrls);
int gcre_hits_reset(gcre_hits* h);   /* an empty list again: found = paths = 0 */
void gcre_hits_free(gcre_hits* h);   /* gcre_destroy frees the ones still alive */
/* k_hits_collect launches of the context since gcre_create (tests: a refusal launches nothing). */
int64_t gcre_hits_launches(const gcre_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif

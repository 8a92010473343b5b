// gcre_kernels.h -- launch interface between the host library (gcre_host.hip and the gcre_host_*.hip files beside it) and the gfx950 kernels
// (gcre_kernels.hip).  Internal; the public boundary is include/gcre_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

namespace gcre {

// GCRE_LAUNCH_TRACE (tests, read at gcre_create): every launcher that clamps its grid names on stderr the blocks (or rounds)
// the input asks for and the ones it launches, so that a test can tell that it drove a kernel past its cap
extern bool g_launch_trace __attribute__((visibility("hidden")));
inline void trace_launch(const char* kernel, long long want, long long got) {
  if (g_launch_trace) fprintf(stderr, "launch %s want=%lld got=%lld\n", kernel, want, got);
}

// Device layout (DESIGN.md "Data layout in HBM"):
//   path rows : uint64 [rows][S], S = M * Wp, Wp = ceil(n/64) rounded up to 4 words (32-byte chunks);
//               method 2 keeps the (+) half in words [0,Wp) and the (-) half in [Wp,2Wp)
//   masks     : uint32 [W32p][Kpad], W32p = 2*Wp dwords, word-major / permutation-minor
//               (the reference's layout, src/join_base.cpp:109, at 32-bit granularity), Kpad % 512 == 0
//   tables    : "diagonal-major": entry [t][i] = table[i][t-i] at index t*(t+1)/2 + i, t = carriers on the
//               path -- one path only ever touches one diagonal (src/methods.h:96-100)
struct Geometry {
  int method;   // M
  int n;        // patients
  int n_cases;
  int W;        // ceil(n/64)
  int Wp;       // padded words per half
  int S;        // row stride in uint64
  int K;        // iterations requested
  int Kpad;
  int TD;       // number of table diagonals = 64*Wp + 1
};

constexpr int kPermTileMax = 2048;     // Kpad granularity (the sparse kernel's permutation tile)
constexpr int kNullBlock = 256;        // threads per block of the null kernel

struct NullArgs {
  const uint32_t* p0;       // paths0 rows (dword view)
  const uint32_t* p1;       // paths1 rows
  const uint32_t* masks;    // [W32p][Kpad]
  const uint32_t* row0;     // per joined path in this launch: row of paths0
  const uint32_t* row1;     // row of paths1, bit 31 = swap (+)/(-) halves of path1 (method 2)
  const uint32_t* tot;      // M entries per path: carriers (M=1) or carriers in (+),(-) halves (M=2)
  const float* t32;         // M=1: sanitised f32 null table, diagonal-major
  const double* d64;        // M=2: f64 vtmax, diagonal-major
  const double* d64n;       // M=2: the table the (-) half reads (d64, or its mirror image: launch_table_to_diag)
  uint32_t* null_bits;      // [Kpad] running maxima as u32 bit patterns of non-negative floats
  int64_t npaths;           // joined paths in this launch
  int64_t npt;              // path tiles
  int S32;                  // row stride in dwords
  int W32p;                 // dwords per half
  int Kpad;
  int nkt;                  // permutation tiles
  int pgroups;              // blocks per permutation tile
};

struct NullConfig {
  int R;        // permutations per lane
  int TPW;      // joined paths per wave per tile
  int perm_tile;   // 64 * R
  int path_tile;   // 4 * TPW
};

NullConfig null_config(int method, int K);
// grid is derived from the args (nkt * pgroups blocks)
hipError_t launch_null(const NullArgs& a, int method, const NullConfig& cfg, hipStream_t stream);

// ---- sparse / bit-sliced null kernel (gcre_sparse.hip) ----
struct SparseSeg {
  uint32_t row0;    // row of paths0 shared by the segment's joined paths
  uint32_t first;   // first joined path of the segment, relative to the launch
  uint32_t n;       // joined paths in the segment
};

struct SparseArgs {
  const uint32_t* mt;        // transposed masks [nkt][mt_rows][64]; row mt_rows-1 is all zero
  const uint32_t* tot;       // carriers per joined path of the launch
  const SparseSeg* segs;
  const uint64_t* loff0;     // CSR bit lists of paths0: offsets [rows+1] ...
  const uint32_t* lidx0;     // ... and entries = patient << 8 (byte offset of the patient's mask row), 4-padded
  const uint64_t* doff;      // per joined path of the launch: [count+1] offsets into dlist
  const uint32_t* dlist;     // entries of the bits paths1 adds on top of paths0, same encoding, 4-padded
  const float* t32;          // method 1 null table
  const double* d64;         // method 2 null table (vtmax)
  uint32_t* null_bits;
  int64_t nsegs;
  int nkt;                   // 2048-permutation tiles
  int waves_per_xcd;         // persistent waves per XCD (grid = 8 * waves_per_xcd / 4 blocks)
  uint32_t mt_rows;
  uint32_t zoff;             // byte offset of the all-zero mask row = (mt_rows - 1) * 256
};
constexpr int kSparseTile = 2048;
constexpr int kSparseSegMax = 64;
hipError_t launch_null_sparse(const SparseArgs& a, int method, int planes, hipStream_t stream);
int sparse_max_waves_per_cu(int method, int planes);   // resident waves per CU of the variant chosen for `planes` counter planes
// ---- inclusion-exclusion null kernel on count planes (gcre_ie.hip) ----
constexpr int kRecSegWords = 12;
// linfo word of a list, written by the inspectors (gcre_inspect.hip):
//   bit 0       mode: 1 = overlap list, 0 = delta list
//   bits 1-2    plane groups of the producing row that can be non-zero, minus one (only k_fill_rec_segs' copy of the word)
//   bits 3-27   padded length: a multiple of 8, at least 8
//   bits 28-31  padding entries
// so that the list's true length = padded length - padding is known without walking it (the bound filter of k_null_ie_m1)
constexpr uint32_t kLinfoLenMask = 0x0ffffff8u;
__host__ __device__ __forceinline__ constexpr uint32_t linfo_make(uint32_t len8, uint32_t mode, uint32_t len) { return len8 | mode | ((len8 - len) << 28); }
__host__ __device__ __forceinline__ constexpr uint32_t linfo_with_groups(uint32_t info, uint32_t extra) { return info | (extra << 1); }
__host__ __device__ __forceinline__ constexpr bool linfo_overlap(uint32_t info) { return (info & 1u) != 0u; }
__host__ __device__ __forceinline__ constexpr uint32_t linfo_groups(uint32_t info) { return (info >> 1) & 3u; }
__host__ __device__ __forceinline__ constexpr uint32_t linfo_len(uint32_t info) { return info & kLinfoLenMask; }
__host__ __device__ __forceinline__ constexpr uint32_t linfo_pad(uint32_t info) { return info >> 28; }
__host__ __device__ __forceinline__ constexpr uint32_t linfo_true_len(uint32_t info) { return linfo_len(info) - linfo_pad(info); }
constexpr int kLadderLevels = 256;   // pruning thresholds j / kLadderPerUnit, j = 0 .. kLadderLevels-1
constexpr int kLadderPerUnit = 8;
constexpr int kLadder2Levels = 352;  // signed method: rows r <-> threshold r / (2 kLadderPerUnit), up to 4/3 of the method-1 range
struct IeArgs {
  const uint32_t* mt;        // transposed masks, as SparseArgs
  const uint32_t* tot;       // carriers per joined path (and half) of the launch
  const uint32_t* rowz;      // per joined path: row of the reduced operand | swap << 31
  const SparseSeg* segs;
  const uint32_t* planes0;   // count planes of paths0 [tile][row*M+h][g0][64][4], or nullptr: stream loff0/lidx0
  const uint32_t* planesz;   // count planes of the reduced operand [tile][row*M+h][gz][64][4] (mode-1 paths)
  uint32_t rows0, rowsz, rows_out;   // row-halves (rows * M) of the three plane arrays
  // paths0 without stored planes but with the recipe of the join that produced it (rec_slot != nullptr): row r of
  // paths0 = row rec_row0[r] of set A | row rec_rowz[r] of set Z (bit 31: halves swapped), list info / slot / overflow per
  // list (row * M + half) as that join's inspector left them; rec_rows_a / rec_rows_z = row-halves of A / Z
  const uint32_t* rec_row0;
  const uint32_t* rec_rowz;
  const uint32_t* rec_linfo;
  const uint32_t* rec_lover;
  const uint32_t* rec_slot;
  const uint32_t* rec_over;
  const uint32_t* rec_planes_a;
  const uint32_t* rec_planes_z;
  uint32_t rec_rows_a, rec_rows_z;
  int rec_ga, rec_gz;
  const uint64_t* loff0;
  const uint32_t* lidx0;
  const uint32_t* linfo;     // per list (path*M + half): padded length (multiple of 8, >= 8) | mode (bit 0: 1 = overlap list)
  const uint32_t* lover;     // per list: where entries 8.. live in `dover` (lists longer than 8)
  const uint32_t* dlist;     // per list: its first 8 entries at [list*8, list*8+8)
  const uint32_t* dover;
  const float* t32;
  const double* d64;
  const uint32_t* ladder;    // [kLadderLevels + 2][ladder_stride] hi << 16 | lo (method 1); rows kLadderLevels, +1: all inside / all outside
  uint32_t* null_bits;
  uint64_t* timing;          // diagnostics build (-DGCRE_IE_TIMING): 12 per-section cycle sums and counts over all waves
  uint32_t* stats;           // optional: [0] += joined-path tiles that were looked up (not pruned)
  uint32_t* planes_out;      // optional: planes of the joined paths [tile][(out_first+q)*M+h][go][64][4]
  int64_t out_first;
  int64_t nsegs;
  int64_t seg_begin, seg_end;        // slice of the segment table this launch walks
  uint32_t score_begin, score_end;   // joined paths of the launch outside [begin, end) only produce planes
  const uint32_t* rec_segs;          // pruned method-1 kernel with a recipe: kRecSegWords words per segment (k_fill_rec_segs)
  int batch;                         // segments per ticket
  uint32_t* queue;                   // pruned kernels: the eight ticket counters of the launch (16 words apart), zero on entry
  uint32_t score_segs;               // the same range in segments: the table's first score_segs segments (they do not straddle)
  int nkt, waves_per_xcd, K;
  int g0, gz, go;            // plane groups (4 planes each) of the three plane arrays
  int lad_mode;              // method-1 kernel: 0 thresholds from the running maxima, 1 look nothing up, 2 look everything up
  uint32_t g00_rows;         // signed kernel: vtmax[0][0] <= g00_rows / (2 kLadderPerUnit), what an EMPTY half contributes to a
                             // path's null score (0 for the hypergeometric table); 0xffffffff: not bounded (NaN)
  int ladder_stride;         // = number of table diagonals
  uint32_t mt_rows, zoff;
  // quad form of the pruned method-1 kernel (gcre_ieq.hip): entry = first segment | (segments - 1) << 30, up to four
  // consecutive segments of `segs` that join the same paths1 rows
  const uint32_t* quads;
  int64_t quad_begin, quad_end;
  // the added rows' planes in the quad kernel: rowsz * gz, the 1-KB units of one tile; z_wide: a tile of them is 4 GiB
  // or more (or GCRE_IE_ZWIDE=1), a row is then reached through a descriptor of its own instead of a 32-bit byte offset
  uint32_t z_tile_units, z_wide;
  // quad kernel: 1 = a path-tile's flagged permutations are queued and scored one per lane (GCRE_IE_FLAGQ, the default),
  // 0 = the second look at the ladder and the exact pass
  uint32_t flagq;
};
hipError_t launch_null_ie_quad(const IeArgs& a, int planes, hipStream_t stream);   // gcre_ieq.hip
int ieq_max_waves_per_cu(int planes, int gz, bool rec, bool wide);
int ieq_quad_segs();   // segments a quad may hold (gcre_ieq.hip)
// r_tot (optional): carriers of the recipe's rows; bits 1-2 of the gathered list-info word then say how many groups of 4
// count planes of the row can be non-zero, minus one (counts never exceed the carrier total).  queue (optional): the 8 x 16
// ticket counters of the pruned launch that follows, zeroed on the way (nsegs > 0)
hipError_t launch_fill_rec_segs(const SparseSeg* segs, int64_t nsegs, const uint32_t* r_row0, const uint32_t* r_rowz,
                                const uint32_t* r_linfo, const uint32_t* r_lover, const uint32_t* r_slot, const uint32_t* r_tot,
                                uint32_t* out, uint32_t* queue, hipStream_t stream);
hipError_t launch_null_ie(const IeArgs& a, int method, int planes, bool general, hipStream_t stream);
int ie_max_waves_per_cu(int method, int planes, int gz, bool out, bool rec);
// the signed method's pruned kernel (gcre_ie2.hip); rec_rows_a / rec_rows_z count row-halves
hipError_t launch_null_ie_m2(const IeArgs& a, int planes, hipStream_t stream);
int ie2_max_waves_per_cu(int planes, int gz, bool out, bool rec);
int ie2_steps();   // steps of the staircase cover of F + G <= theta (GCRE_M2_STEPS)
hipError_t launch_build_planes(const uint32_t* mt, uint32_t mt_rows, int nkt, const uint64_t* loff, const uint32_t* lidx,
                               int64_t nrowhalves, int groups, uint32_t* planes, hipStream_t stream);
hipError_t launch_build_ladder(const float* t32, int TD, uint32_t* ladder, hipStream_t stream);
hipError_t launch_build_ladder2(const double* dmax, int TD, uint32_t* ladder, hipStream_t stream);   // signed method, half thresholds
// exclusive prefix sum of n u32 counts into n+1 u64 offsets; the low 2 bits of a count do not add, they are copied
// into the low bits of its offset (list lengths are multiples of 4, bit 0 carries the IE list mode) (scratch: >= (n+1023)/1024 + 1 u64)
hipError_t launch_scan_u32_u64(const uint32_t* cnt, int64_t n, uint64_t* off, uint64_t* scratch, hipStream_t stream);
// per joined path: entries of paths1's list whose bit is clear in the paths0 row, 16-padded, at dlist[doff[i]..)
hipError_t launch_delta_fill(const uint32_t* p0, int S32, int W32p, int method, const uint32_t* row0,
                             const uint32_t* row1, int64_t count, const uint64_t* loff1, const uint32_t* lidx1,
                             const uint64_t* doff, uint32_t zoff, uint32_t* dlist, hipStream_t stream);
hipError_t launch_row_bits(const uint32_t* rows, int64_t nrows, int S32, int W32p, uint32_t* cnt, hipStream_t stream);
hipError_t launch_row_fill(const uint32_t* rows, int64_t nrows, int S32, int W32p, const uint64_t* off, uint32_t zoff,
                           uint32_t* idx, hipStream_t stream);
hipError_t launch_build_mt(const uint32_t* masks, int W32p, int Kpad, int nkt, uint32_t mt_rows, uint32_t* mt,
                           hipStream_t stream);

hipError_t launch_pack_dense(const int32_t* data, int64_t nrow, int ncol, int col_major, uint64_t* rows, int S,
                             hipStream_t stream);
hipError_t launch_select(const uint64_t* from, const int32_t* idx, int64_t n, int S, uint64_t* out, hipStream_t stream);
hipError_t launch_masks_from_ints(const int32_t* perms, int nrows_in, int ncol, int col_major, const Geometry& g,
                                  uint32_t* masks, hipStream_t stream);
hipError_t launch_masks_from_words(const uint64_t* packed, int nrows_in, const Geometry& g, uint32_t* masks,
                                   hipStream_t stream);

// joined-path ordinal -> (row of paths0, row of paths1 | swap<<31)
hipError_t launch_expand(const int64_t* path_idx, const int64_t* location, int64_t n_uids, const int32_t* signs,
                         int path_length, int method, int64_t first, int64_t count, uint32_t* row0, uint32_t* row1,
                         hipStream_t stream);

// The flag block of a chunk's inspector (StatsArgs::max_tot, ::bad, ::ov_count; IeArgs::stats): 8 words, zeroed by the host
// in front of the inspector.  Word kFlagOverReserved is the JOIN's, not the chunk's: the long-list area of a kept set's recipe
// fills across the chunks of the join, so the host writes the join's count of entries reserved so far (JoinRun::over_next)
// into it in front of every inspector launch that fills a recipe -- a chunk replayed from the inspection cache never touched
// the block, and an ahead inspection ran on another one.  Words 6-7 belong to the join too.
enum FlagWord : int {
  kFlagMaxTot = 0,         // largest carrier total of the chunk
  kFlagHintBroken = 1,     // some joined path differs from paths0 | reduced row
  kFlagOverlapLists = 2,   // lists in overlap mode
  kFlagLookupTiles = 3,    // joined-path tiles the pruned kernel looked up
  kFlagOverReserved = 4,   // entries reserved in the long-list area
  kFlagMaxLen = 5,         // longest list (padded)
  kFlagRangeUnion = 6,     // 6-7: verdict of the range-union check of a hinted join (k_range_union)
  kFlagWords = 8,
};

struct StatsArgs {
  const uint64_t* p0;
  const uint64_t* p1;
  const uint32_t* row0;
  const uint32_t* row1;
  const uint64_t* case_mask;   // [Wp]
  const double* dvt;           // f64 value table, diagonal-major
  uint64_t* key;               // order-preserving u64 image of the real score (0 = never a candidate)
  uint32_t* tot;               // M per path
  uint32_t* cases;
  uint32_t* ctrls;
  uint64_t* res;               // kept rows, indexed by absolute ordinal (first + i), or nullptr
  uint32_t* max_tot;           // optional: running maximum of the carrier totals (sizes the sparse kernel's counters)
  uint32_t* dcnt;              // optional: popcount(path1 & ~path0) rounded up to 4, per joined path (and half)
  // inclusion-exclusion form (all optional): pz = reduced operand, zindex[row of paths1] = its row (nullptr: same row)
  const uint64_t* pz;
  const int32_t* zindex;
  uint32_t* rowz;              // out: reduced row | swap << 31 per joined path
  uint32_t* bad;               // out: set to 1 when some joined path differs from paths0 | reduced row
  int ie_bias;                 // overlap list chosen when overlap + ie_bias < delta; negative: never
  int ie_rule;                 // 1: overlap list whenever it fits the 8-entry slot or is shorter than the delta list (method 1: the
                               // quad kernel has the added row's planes at hand anyway); 0: the bias rule
  // k_stats_ie only: the lists themselves, written in the same pass (no scan, no fill kernel).  List d = path*M + half
  // has its first 8 entries in slot[d*8 .. d*8+8) and the rest, when it is longer, in over[lover[d] ..); both padded
  // with `zoff` to a multiple of 8.  linfo[d] = padded length | mode (bit 0: 1 = overlap list).
  const uint64_t* excess;      // hinted joins: [ranges][S] union of paths1 & ~reduced over each uid range (k_range_union), or nullptr
  const int32_t* range_of;     // uid (row of paths0) -> its range
  uint32_t* linfo;
  uint32_t* lover;
  uint32_t* slot;
  uint32_t* over;
  uint32_t over_cap;           // entries `over` can hold; ov_count beyond it means: grow and run again
  uint32_t* ov_count;          // entries reserved in `over` so far
  uint32_t zoff;
  // k_stats_ie2h (method 2): CSR offsets of the reduced operand's bit lists (two per row), set only when every row of it
  // has an empty half
  const uint64_t* lz_off;
  // k_stats_ie2 (method 1): carriers | carriers among the cases << 16 of every row of the reduced operand (k_row_counts), or
  // nullptr: the inspector counts the joined row's words itself
  const uint32_t* z_counts;
  int64_t first;
  int64_t count;
  int S;
  int Wp;
};
// The long-list area (StatsArgs::over) is handed out in chunks: a wave of an inspector reserves kOverChunk entries at a
// time (more when one round of its lists needs more), so a launch can leave most of a chunk per wave unused.  An
// inspector's grid is at most kInspectMaxBlocks blocks of kInspectBlockWaves waves: the host sizes the area's slack
// from these.
constexpr uint32_t kOverChunk = 2048;
constexpr int kInspectBlockWaves = 4;
constexpr int kInspectMaxBlocks = 256 * 16;
constexpr int kStatsIeBlockPaths = 4 * kInspectBlockWaves;   // k_stats_ie: four paths per wave and pass, the most waves per path
hipError_t launch_stats(const StatsArgs& a, int method, hipStream_t stream);
hipError_t launch_stats_ie(const StatsArgs& a, int method, hipStream_t stream);   // gcre_inspect.hip
// counts[r] = carriers | carriers among the cases << 16 of row r (rows of Wp words, 64 * Wp < 65536: both fit 16 bits)
hipError_t launch_row_counts(const uint64_t* rows, int64_t nrows, int Wp, const uint64_t* case_mask, uint32_t* counts,
                             hipStream_t stream);
// The range check of a hinted join walks each distinct uid range -- `rows` consecutive paths1 rows from `first` -- once.  A
// range of more than kRangePieceRows rows (a hub gene's) is cut into pieces of that many (the last one shorter), marked by
// bit 31 of `rows`; `cut` lists the ranges that were cut.  16 rows: what one wave of k_range_union reads in a single round
// (four 16-lane groups, four rows each in flight).  The benchmark's level 4: 16,881 ranges, median 7 rows, 99th percentile
// 84, longest 3,467; 2,172 ranges are cut, 21,765 pieces in all (profiles/helpers_before.txt).
constexpr int kRangePieceRows = 16;
struct RangePiece {
  int64_t first;     // paths1 row
  int32_t range;     // row of U
  int32_t rows;      // 1 .. kRangePieceRows; | 0x80000000: one piece of several
};
hipError_t launch_range_union(const uint64_t* p1, const uint64_t* pz, const int32_t* zindex, const RangePiece* pieces,
                              int64_t npieces, const int32_t* cut, int64_t ncut, int S, int Wp, int method, uint64_t* excess,
                              uint32_t* bad, hipStream_t stream);

// ---- top-k selection over key[0..count) ----
hipError_t launch_hist(const uint64_t* key, int64_t count, int shift, uint64_t prefix, uint32_t* hist256,
                       hipStream_t stream);
// all eight digit passes queued back to back, the state between them stays on the device: afterwards st->prefix is the
// need-th largest key, st->greater the number of keys in higher buckets, st->need / st->eq_count the wanted / present
// number of keys equal to it.  With a candidate buffer (`cand`, `cand_cap` keys; `note`: two words of scratch) only the
// first two passes and one compaction read all keys: the other six read the keys that share the 16 bits chosen by then,
// unless more than cand_cap do -- then they read all keys as without a buffer.  The state is the same on every road.
struct SelectState {
  uint64_t prefix;
  int64_t need;
  int64_t greater;
  uint32_t eq_count;
  uint32_t pad;
};
hipError_t launch_radix_select(const uint64_t* key, int64_t count, int64_t need, uint32_t* hist256, SelectState* st,
                               uint64_t* cand, uint32_t cand_cap, uint32_t* note, hipStream_t stream);
// appends every i with key[i] > thr (any order) to out[], counter in *n_out
hipError_t launch_collect_gt(const uint64_t* key, int64_t count, uint64_t thr, uint32_t* out, uint32_t* n_out,
                             uint32_t cap, hipStream_t stream);
// The keys of the two zeros.  score_key is the order-preserving image of a double's BITS, so -0.0 lands one key below +0.0,
// while as scores they are equal (the reference compares doubles, methods.h:91): wherever keys decide a tie, the two are
// one class.  A path keeps its own key, so the score it reports has its own sign.
constexpr uint64_t kKeyPlusZero = 0x8000000000000000ull;
constexpr uint64_t kKeyMinusZero = 0x7fffffffffffffffull;
// per 1024-entry chunk: number of key[i] == thr or == alt (alt = thr: one key; the two zero keys: the zeros' tie class)
hipError_t launch_eq_count(const uint64_t* key, int64_t count, uint64_t thr, uint64_t alt, uint32_t* chunk_cnt,
                           hipStream_t stream);
// first `m` (in index order) entries with key[i] == thr or == alt, written at out[rank]; chunk_base = exclusive scan of
// chunk_cnt
hipError_t launch_eq_collect(const uint64_t* key, int64_t count, uint64_t thr, uint64_t alt, const uint32_t* chunk_base,
                             uint32_t m, uint32_t* out, hipStream_t stream);
hipError_t launch_gather_winners(const uint32_t* sel, uint32_t nsel, const uint64_t* key, const uint32_t* cases,
                                 const uint32_t* ctrls, const uint32_t* row0, const uint32_t* row1, uint64_t* o_key,
                                 uint32_t* o_cases, uint32_t* o_ctrls, uint32_t* o_row0, uint32_t* o_row1,
                                 hipStream_t stream);
hipError_t launch_generate_masks(uint64_t seed, int K, int n, int n_strata, const int32_t* stratum, const uint32_t* cases_in,
                                 const uint32_t* size_of, uint32_t* work, int W32p, int Kpad, uint32_t* masks,
                                 hipStream_t stream);
// *asym (method 2; zero on entry) becomes 1 when vtmax is not symmetric: std::max(a, b) keeps a NaN in its first argument and
// drops one in its second, so a NaN on one side of the diagonal only makes vtmax[r][c] != vtmax[c][r].  The (-) half of a
// path reads vtmax[tn - b][b] (methods.h:227), the kernels index a diagonal by b: for such a table they read the (-) half
// from the mirror image launch_mirror_diag writes (dmaxn[t][i] = dmax[t][t - i]).
hipError_t launch_table_to_diag(const double* table, int nrow, int ncol, int col_major, int n, int TD, double* dvt,
                                float* t32, double* dmax, uint32_t* asym, hipStream_t stream);
hipError_t launch_mirror_diag(const double* dmax, int TD, double* dmaxn, hipStream_t stream);
hipError_t launch_fill_u32(uint32_t* p, int64_t n, uint32_t v, hipStream_t stream);
hipError_t launch_max_merge(uint32_t* dst, const uint32_t* src, int n, hipStream_t stream);

// ---- decorated p-values (gcre_decorated.hip) ----
// One split as k_decorated_null reads it: the sub-path-1 counts its scores add to, gene 2's observed counts, the two urns
// (without strata) or a run of DpStratum entries, and the key of its random stream.
struct DpUrns {
  int32_t case_pos1, ctrl_pos1, case_neg1, ctrl_neg1;   // gcre_dp_split's
  int32_t case_pos2, ctrl_pos2, case_neg2, ctrl_neg2;   // observed gene-2 counts (k_decorated_observed)
  int32_t k_pos, pop_pos, succ_pos, k_neg;
  int32_t pop_neg, succ_neg;
  int32_t st_off, st_n;   // st_n > 0: the urns are DpStratum[st_off, st_off + st_n) (only strata that draw)
  uint64_t key;           // dp_split_key(seed, split)
  uint64_t pad;
};
struct DpStratum { int32_t pop, cases, k_pos, k_neg; };

// splitmix64 finaliser: the counter-based random stream of the permutation masks and of the decorated draws
__host__ __device__ inline uint64_t gcre_mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// Draw t of permutation r of split s reads u = gcre_mix64(dp_perm_base(dp_split_key(seed, s), r) + t); t counts the draws
// of the split's urns in order (strata ascending, pos before neg), skipped draws included.
__host__ __device__ inline uint64_t dp_split_key(uint64_t seed, int64_t s) {
  return gcre_mix64(seed ^ (0xd1b54a32d192ed03ull * (uint64_t)(s + 1)));
}
__host__ __device__ inline uint64_t dp_perm_base(uint64_t key, int64_t r) {
  return gcre_mix64(key ^ (0x51ed270b7f3c9a1dull * (uint64_t)(r + 1)));
}

// obs[s] = the observed score of split s from d_dvt (what k_decorated_null compares against)
hipError_t launch_decorated_observed(const DpUrns* urns, int S, int method, const double* dvt, double* obs,
                                     hipStream_t stream);
// n_ge[s] += permutations r < K of split s whose score >= obs[s]; perm_counts (optional) [S][K][2] = urn successes
hipError_t launch_decorated_null(const DpUrns* urns, const DpStratum* strata, int S, int K, int method, const double* dvt,
                                 const double* obs, unsigned long long* n_ge, int32_t* perm_counts, hipStream_t stream);

// ---- permutation tests of caller-given sets (gcre_sets.hip) ----
constexpr int kSetPermTile = 512;   // permutations per block of k_set_null
struct SetNullArgs {
  const uint32_t* rows;         // [nsets][M][W32p] union rows of the launched sets: (+) half, then (-) half (method 2)
  const uint32_t* masks;        // [W32p][Kpad]
  const uint32_t* tot;          // [nsets][M] carriers per half
  const uint32_t* thr;          // [nsets] f32 bit pattern: permutation r counts iff bits(null_r) >= thr
  const float* t32;             // M=1: sanitised f32 null table, diagonal-major
  const double* d64;            // M=2: f64 vtmax, diagonal-major
  const double* d64n;           // M=2: the table the (-) half reads (d64, or its mirror image)
  unsigned long long* n_ge;     // [nsets], zero on entry
  uint32_t* fam_bits;           // [Kpad] maxima over the sets as u32 bit patterns (zero on entry), or nullptr
  int64_t nsets;
  int64_t npt;                  // set tiles (set_null_tile_sets sets each)
  int W32p, Kpad, K;
  int nkt;                      // permutation tiles of kSetPermTile
  int pgroups;                  // blocks per permutation tile
};
int set_null_tile_sets(int method);
// obs[s] = the observed score of set s from d_dvt; cnt[s] = cases_pos, ctrls_pos, cases_neg, ctrls_neg
hipError_t launch_set_observed(const int32_t* cnt, int64_t S, int method, const double* dvt, double* obs,
                               hipStream_t stream);
hipError_t launch_set_null(const SetNullArgs& a, int method, hipStream_t stream);

// ---- residual union rows of (set, given set) pairs (gcre_given.hip) ----
// Entry e: the unions of set which[e] without the carriers of set given[e], in SetNullArgs' row layout, with the counts and
// totals SetUnion::build gives such rows.
struct SetResidualArgs {
  const uint32_t* rows;         // [n_rows][W2] the caller's gene rows as dwords (bits beyond the patients are ignored)
  const int64_t* set_off;       // [n_sets + 1] the caller's set list as it is
  const int32_t* members;       // rows of every set; none of a launched entry's sets is NA
  const int32_t* signs;         // per member +1 / -1, or nullptr = all +1 (read by method 2)
  const int64_t* which;         // [n] the set of every entry
  const int64_t* given;         // [n] the set whose carriers are set aside, -1 = none
  uint32_t* out;                // [n][M][W32p] residual rows: (+) half, then (-) half (method 2); zero beyond the patients
  int32_t* cnt;                 // [n][4] cases_pos, ctrls_pos, cases_neg, ctrls_neg
  uint32_t* tot;                // [n][M] carriers per half
  int64_t n;                    // entries
  int W2;                       // dwords per gene row
  int W32p;                     // dwords per half of an output row, >= W2
  int n_patients, n_cases;
};
hipError_t launch_set_residual(const SetResidualArgs& a, int method, hipStream_t stream);

// ---- per-gene best-path tally (gcre_genes.hip) ----
constexpr int kGeneWidthMax = 3;   // gene slots a path inherits from one operand row, at most
// One scored stretch of a chunk, as its inspector left it, folded into a join's per-slot table.
struct GeneFoldArgs {
  const uint64_t* key;          // [count] score keys (score_key: monotone in the score, 0 = not a score)
  const uint32_t* row0;         // [count] paths0 row = uid row (Score.src)
  const uint32_t* row1;         // [count] paths1 row (Score.trg), bit 31 = the signed method's half swap
  const uint32_t* cases;        // [count]
  const uint32_t* ctrls;        // [count]
  int64_t count;
  int64_t first;                // joined-path ordinal of element 0
  const int32_t* genes0;        // [rows of paths0][w0] slots, -1 = none; unused when w0 == 0
  const int32_t* genes1;        // [rows of paths1][w1]
  int w0, w1;                   // 0..kGeneWidthMax
  int n_slots;
  int prior;                    // != 0: bkey may hold entries (an earlier chunk or join was folded into the table)
  uint64_t* ck;                 // [n_slots] chunk-local best key, 0 on entry and on exit
  uint32_t* cidx;               // [n_slots] chunk-local index of the best path, 0xffffffff on entry and on exit
  uint64_t* bkey;               // [n_slots] the join's table: key (0 = no scored path), ordinal, rows, counts
  int64_t* bord;
  int32_t *bsrc, *btrg, *bcases, *bctrls;
};
// k_gene_fold, k_gene_index, k_gene_merge on `stream`, in that order
hipError_t launch_gene_fold(const GeneFoldArgs& a, int cus, hipStream_t stream);

// ---- null exceedance counts (gcre_exceed.hip) ----
constexpr int kExceedMax = 10000;      // thresholds of one object (the top_k limit)
// up to here the bins of a block are a u32 histogram in LDS: 16 KB next to the 8 KB of queues in k_exceed_ie (k_null_ie's
// maxima take 32 KB), 8 KB next to the 16 KB mask tile and the queues in k_exceed_dense
constexpr int kExceedLdsBinsIe = 4096;
constexpr int kExceedLdsBinsDense = 2048;
// The scored stretch of a chunk against the permutations of the window, in k_null's mapping: the fields of NullArgs
// (row0 / row1 / tot start at the stretch's first path; nothing beyond [0, npaths) is read), and the thresholds.
struct ExceedArgs {
  const uint32_t* p0;
  const uint32_t* p1;
  const uint32_t* masks;
  const uint32_t* row0;
  const uint32_t* row1;
  const uint32_t* tot;
  const float* t32;
  const double* d64;
  const double* d64n;         // method 2: the table the (-) half reads (d64, or its mirror image)
  const uint32_t* pat;        // [m] ascending f32 bit patterns: a null value v counts for threshold j iff bits(v) >= pat[j]
  unsigned long long* hist;   // [m] bin j += values v with pat[j] <= bits(v) and (j == m-1 or bits(v) < pat[j+1])
  int64_t npaths;
  int64_t npt;
  int S32, W32p, Kpad;
  int K;                      // permutations of the window: columns K.. of the last tile never count
  int nkt, pgroups;
  int m;
  int lds_bins;               // m (<= kExceedLdsBinsDense): per-block histogram in LDS; 0: straight into `hist`
  // per-permutation counts; nullptr: none, and the kernels are the ones they were
  uint32_t* pc;               // [m][pc_stride] cell [bin][k0 + r] += 1 with every value of window permutation r binned
  int pc_stride;              // >= k0 + K
  int k0;                     // absolute index of the window's first permutation
};
// the same three for the inclusion-exclusion form
struct ExceedPerm {
  uint32_t* pc = nullptr;
  int stride = 0;
  int k0 = 0;
};
hipError_t launch_exceed_dense(const ExceedArgs& a, int method, const NullConfig& cfg, hipStream_t stream);
// The inclusion-exclusion form: the chunk's IeArgs as k_null_ie takes them (segments [seg_begin, seg_end), paths inside
// [score_begin, score_end) count; planes_out, null_bits, stats, ladder, queue are not read), `planes` counter planes.
// lds_bins: m (<= kExceedLdsBinsIe) or 0.
hipError_t launch_exceed_ie(const IeArgs& a, int method, int planes, const uint32_t* pat, unsigned long long* hist, int m,
                            int lds_bins, hipStream_t stream, const ExceedPerm& perm = ExceedPerm());
int exceed_ie_max_waves_per_cu(int method, int planes, int lds_bins, bool perm_counts = false);
struct ExceedObsArgs {
  const uint64_t* key;        // [count] score keys (0 = not a score: never counts)
  const uint64_t* tkey;       // [m] ascending threshold keys (>= 1)
  unsigned long long* hist;   // [m] bins as ExceedArgs::hist
  int64_t count;
  int m;
  int lds_bins;
};
hipError_t launch_exceed_observed(const ExceedObsArgs& a, int cus, hipStream_t stream);

// ---- hit lists (gcre_hits.hip) ----
constexpr int64_t kHitsCapMax = (int64_t)1 << 26;   // records of one list: 2 GB of device memory at 32 B each
// One scored stretch of a chunk, as its inspector left it (the fields of GeneFoldArgs), compacted into a join's hit list.
struct HitsArgs {
  const uint64_t* key;          // [count] score keys (0 = not a score: never a hit)
  const uint32_t* row0;         // [count] paths0 row = uid row (Score.src)
  const uint32_t* row1;         // [count] paths1 row (Score.trg), bit 31 = the signed method's half swap
  const uint32_t* cases;        // [count]
  const uint32_t* ctrls;        // [count]
  int64_t count;
  int64_t first;                // joined-path ordinal of element 0
  uint64_t tkey;                // a path is a hit iff key != 0 && key >= tkey
  unsigned long long* cursor;   // hits found so far: grows by every hit, also past `cap`
  int64_t cap;                  // records the arrays below hold; a hit whose slot is >= cap is counted and not written
  int64_t* ord;                 // [cap] joined-path ordinal
  uint64_t* hkey;               // [cap] the path's own key
  int32_t *src, *trg, *hcases, *hctrls;   // [cap] each
};
hipError_t launch_hits_collect(const HitsArgs& a, int cus, hipStream_t stream);

// ---- step-down max-T counts of a level's top rows (gcre_stepdown.hip) ----
// k_set_null's launch geometry (set_null_tile_sets sets per tile, kSetPermTile permutations per block) over the top rows.
struct StepdownArgs {
  const uint32_t* rows;         // [nsets][M][W32p] union rows, as SetNullArgs
  const uint32_t* masks;        // [W32p][Kpad]
  const uint32_t* tot;          // [nsets][M] carriers per half
  const float* t32;
  const double* d64;
  const double* d64n;
  const uint32_t* pat;          // [m] ascending f32 bit patterns (gcre_exceed)
  const int32_t* cap;           // [nsets] the last sorted index strictly below the set's own threshold (f64), -1: none
  uint32_t* E;                  // [m][stride] zero on entry: cell [bin][r] += 1, bin = min(the value's bin, cap)
  int64_t nsets;
  int64_t npt;
  int W32p, Kpad, K;
  int nkt, pgroups;
  int m, stride;                // stride >= K
};
hipError_t launch_stepdown_null(const StepdownArgs& a, int method, hipStream_t stream);
struct StepdownFinishArgs {
  const uint32_t* pc;           // [m][stride] the join's per-permutation counts per bin
  const uint32_t* E;            // [m][stride]
  uint32_t* n_ge;               // [m] zero on entry: permutations r < K with V[b][r] > E[b][r], per sorted threshold
  uint32_t* bad;                // [1] zero on entry: permutations with E > V in some bin
  int m, stride, K;
};
hipError_t launch_stepdown_finish(const StepdownFinishArgs& a, hipStream_t stream);

// ---- step-down, k-FWER and FDR over a family of caller-given sets (gcre_family.hip) ----
// N [nsets][stride]: the null scores of a slab of `nkt` whole permutation tiles as u32 bit patterns of non-negative floats,
// row = the set's rank in ascending observed order.  Columns >= live (the padding of the last tile) are never counted.
constexpr int kFamilyKmax = 10;        // GCRE_FAMILY_KMAX: the largest values of a column k_family_scan keeps
constexpr int kFamilyHistBins = 4096;  // bins of k_family_hist's LDS histogram: one pass over N per that many thresholds
struct FamilyNullArgs {
  const uint32_t* rows;         // [nsets][M][W32p] union rows, as SetNullArgs
  const uint32_t* masks;        // [W32p][Kpad]
  const uint32_t* tot;          // [nsets][M] carriers per half
  const float* t32;
  const double* d64;
  const double* d64n;
  const uint32_t* rank;         // [nsets] the row of N a set's values go to, a permutation of 0 .. nsets-1
  uint32_t* N;                  // [nsets][stride]
  int64_t nsets;
  int64_t npt;                  // set tiles (set_null_tile_sets sets each)
  int64_t stride;               // nkt * kSetPermTile
  int W32p, Kpad, K;
  int kt0, nkt;                 // the slab: permutation tiles [kt0, kt0 + nkt) of kSetPermTile
  int pgroups;                  // blocks per permutation tile
};
hipError_t launch_family_null(const FamilyNullArgs& a, int method, hipStream_t stream);
struct FamilyScanArgs {
  const uint32_t* N;            // [nsets][stride]
  const uint32_t* meta;         // [nsets padded to 64, with zeros] by row: the f32 threshold pattern; bit 31 = the last row of a tie group
  uint32_t* n_ge;               // [nsets] by row, adds at the last row of every tie group: live columns (< 2^31 in all) whose
                                // running maximum reaches the group's threshold
  uint32_t* kmax;               // [kFamilyKmax][kstride] the column's largest values, descending (0: no such set), or nullptr
  int64_t nsets, stride, kstride;
  int live;                     // live columns of the slab
  int k0;                       // the slab's first permutation: column c is kmax's column k0 + c
};
hipError_t launch_family_scan(const FamilyScanArgs& a, hipStream_t stream);
struct FamilyHistArgs {
  const uint32_t* N;            // [nsets][stride]
  const uint32_t* pat;          // [m] ascending distinct f32 threshold patterns
  unsigned long long* hist;     // [m] adds: live values whose largest reached pattern is this one
  int64_t nsets, stride;
  int live, m;
};
hipError_t launch_family_hist(const FamilyHistArgs& a, int cus, hipStream_t stream);

// ---- min-P over a family of caller-given sets (gcre_minp.hip) ----
// A slab is a run of rows of the walk order (NaN scores first, then the count c descending) with ALL permutation tiles:
// N [rows][stride] from k_family_null, R [rows][stride] the within-row counts "values >= mine" over the live columns.
constexpr int kMinpChunk = 16384;      // values of a row k_minp_rank sorts in LDS at a time (64 KiB)
struct MinpGatherArgs {
  const uint32_t* rows;         // [nsets][rw] union rows as the set stage left them
  const uint32_t* tot;          // [nsets][m]
  const uint32_t* order;        // [nsets] row of the input per row of the walk, a permutation of 0 .. nsets-1
  uint32_t* rows_out;           // [nsets][rw]
  uint32_t* tot_out;            // [nsets][m]
  int64_t nsets;
  int rw, m;                    // dwords per set (M * W32p), halves per set (M)
};
hipError_t launch_minp_gather(const MinpGatherArgs& a, hipStream_t stream);
struct MinpRankArgs {
  const uint32_t* N;            // [nsets][stride] bit patterns of non-negative floats
  uint32_t* R;                  // [nsets][stride] column r < K: #{r' < K : N[.][r'] >= N[.][r]}; the other columns 0xffffffff
  int64_t nsets, stride;        // stride: a multiple of 16 at or above K
  int K;
};
hipError_t launch_minp_rank(const MinpRankArgs& a, hipStream_t stream);
struct MinpScanArgs {
  const uint32_t* R;            // [nsets][stride]
  const uint32_t* meta;         // [nsets] by row: the count c; bit 31 = the last row of a counted tie group
  uint32_t* q;                  // [K] the running minimum per permutation: read at the start, written at the end
  uint32_t* n_le;               // [nsets] by row, adds at the last row of every counted tie group: permutations with q <= c
  int64_t nsets, stride;
  int K;
};
hipError_t launch_minp_scan(const MinpScanArgs& a, hipStream_t stream);

// ---- competitive set tests: matched random sets on the observed labels (gcre_compete.hip) ----
// One wave of k_compete_null takes a valid set and a run of `dpw` draws of the slab [b0, b0 + nb): per draw it makes the
// picks by the rule of gcre_compete.h, ORs the picked gene rows over the patients and looks the score up in the f64 table.
struct CompeteSet {
  int64_t set;                      // index in the caller's list: the key of its random stream
  int32_t moff, k;                  // its members are entries [moff, moff + k) of `mem` / `signs`
};
struct CompeteMemberDev { int32_t off, n; };   // gcre_compete::CompeteMember: off < 0 fixed on row n, else pool rows [off, off + n)
struct CompeteArgs {
  const uint32_t* rows;             // [n_rows][Wd] the caller's gene rows as dwords, Wd a multiple of 4 (16-byte lanes)
  const int32_t* pool_rows;         // the pool table: rows by bin, ascending (read-only: scalar loads)
  const CompeteMemberDev* mem;      // [members of the list]
  const int32_t* signs;             // [members of the list] +1 / -1, or nullptr (method 2 reads them)
  const CompeteSet* sets;           // [V] the valid sets (read-only: scalar loads)
  const double* dvt;                // the observed-score table, diagonal-major
  const double* obs;                // [V] observed scores as k_set_observed left them
  unsigned long long* n_ge;         // [V] adds: draws whose null score >= obs
  double* null_out;                 // optional [V][stride]: column b - b0
  int32_t* picks_out;               // optional [nb][tm]: the row every member received (members of invalid sets are not written)
  uint64_t seed;
  int64_t b0;                       // first draw of the slab
  int64_t stride;                   // columns of null_out
  int64_t tm;                       // members of the whole list
  int32_t V, nb;                    // valid sets, draws of the slab
  int32_t dpw, groups;              // draws per wave, waves per set = ceil(nb / dpw)
  int32_t Wd;                       // dwords per gene row
  int32_t n, n_cases;               // patients; columns below n_cases are the cases
  int32_t attempts;                 // 1 .. 64
  int32_t maxk;                     // the most members of a valid set
};
hipError_t launch_compete_null(const CompeteArgs& a, int method, hipStream_t stream);

// ---- split-half stability: sets scored on random halves of the cohort (gcre_subsample.hip) ----
// k_subsample_masks writes the masks of draws [b0, b0 + nb) by the rule of gcre_subsample.h (seed1 = subsample_seed(seed)) in
// SetNullArgs' mask layout, [W32p][Kpad] dwords with the columns nb .. Kpad-1 and the rows beyond the patients zero;
// k_subsample_null scores the launched sets on every draw (half A) and on its complement (half B) with k_set_null's geometry.
struct SubsampleArgs {
  const uint32_t* rows;         // [nsets][M][W32p] union rows of the launched sets: (+) half, then (-) half (method 2)
  const uint32_t* masks;        // [W32p][Kpad] the slab's draws
  const uint32_t* tot;          // [nsets][M][2] carriers per half-row among the cases, among the controls
  const double* dvt_a;          // half A's table, diagonal-major, diagonals 0 .. m_cases + m_ctrls
  const double* dvt_b;          // the complement's, diagonals 0 .. n - m_cases - m_ctrls, or nullptr: half B is not scored
  const double* cut;            // [nsets][n_cut] (read-only: scalar loads), nullptr with n_cut == 0
  unsigned long long* n_a;      // [nsets][n_cut] adds: draws whose A score >= cut
  unsigned long long* n_b;      // ... whose B score >= cut (with dvt_b)
  unsigned long long* n_both;   // ... both (with dvt_b)
  double* scores_a;             // optional [nsets][stride]: column = draw of the slab
  double* scores_b;             // optional, with dvt_b
  int64_t nsets;
  int64_t npt;                  // set tiles (set_null_tile_sets sets each)
  int64_t stride;               // columns of scores_a / scores_b, >= Kpad
  int W32p, Kpad, K;            // K: draws of the slab
  int nkt;                      // draw tiles of kSetPermTile
  int pgroups;                  // blocks per draw tile
  int n_cases;                  // columns below it are the cases
  int n_cut;
};
hipError_t launch_subsample_masks(uint64_t seed1, int64_t b0, int nb, int n_cases, int n_ctrls, int m_cases, int m_ctrls, int W32p,
                                  int Kpad, uint32_t* masks, hipStream_t stream);
hipError_t launch_subsample_null(const SubsampleArgs& a, int method, hipStream_t stream);

// ---- sequential permutation p-values: every set stops at its h-th exceedance (gcre_sequential.hip) ----
// One batch of permutations [r0, r0 + nb), never resident beyond it.  k_seq_masks writes their masks by the rule of
// gcre_sequential.h (k_generate_masks' rule) in SetNullArgs' mask layout, [W32p][stride] dwords with the columns nb .. stride-1
// and the rows beyond the patients zero.  k_seq_null runs the count loop of gcre_count_tile.h over the sets of the active list and writes,
// per active slot, the batch's bit row; k_seq_retire stops the slots whose h-th exceedance lies in it and lists the others.
struct SeqMaskArgs {
  uint64_t seed;
  uint64_t r0;                  // the first permutation of the batch
  const int32_t* stratum;       // [n] (read-only: scalar loads), or nullptr: one stratum
  const uint32_t* cases_in;     // [n_strata] cases of every stratum
  const uint32_t* size_of;      // [n_strata] patients of every stratum
  uint32_t* work;               // [2 n_strata][stride] need / rem of every column, only above kSeqRegStrata strata
  uint32_t* masks;              // [W32p][stride]
  int n, n_strata;
  int nb;                       // permutations of the batch, <= stride
  int W32p, stride;             // stride: a multiple of 64
};
constexpr int kSeqRegStrata = 4;   // up to so many strata keep need / rem in registers
struct SeqNullArgs {
  const uint32_t* rows;         // [sets][M][W32p] union rows, as SetNullArgs
  const uint32_t* masks;        // [W32p][stride] the batch's masks
  const uint32_t* tot;          // [sets][M] carriers per half
  const uint32_t* thr;          // [sets] f32 bit pattern: a permutation counts iff bits(null) >= thr
  const float* t32;             // M=1: sanitised f32 null table, diagonal-major
  const double* d64;            // M=2: f64 vtmax, diagonal-major
  const double* d64n;           // M=2: the table the (-) half reads
  const uint32_t* active;       // [nactive] set indices (read-only: scalar loads), in any order
  unsigned long long* bits;     // [nactive][stride / 64]: bit i of slot a = permutation r0 + i reached set active[a]'s score
  int64_t nactive;
  int64_t npt;                  // set tiles (set_null_tile_sets sets each) of the active list
  int W32p, stride, K;          // K: permutations of the batch; the columns K .. nkt * kSetPermTile - 1 write 0
  int nkt;                      // permutation tiles of kSetPermTile
  int pgroups;                  // blocks per permutation tile
};
struct SeqRetireArgs {
  const unsigned long long* bits;   // [nactive][wstride]
  const uint32_t* active;           // [nactive]
  uint32_t* next;                   // [>= nactive] the slots that go on, in any order
  uint32_t* n_next;                 // one dword, zero on entry: how many
  uint32_t* prior;                  // [sets] exceedances so far, < h while a set is active
  long long* n_perm;                // [sets] 0 while a set has not stopped, then the 1-based position of its h-th exceedance
  uint64_t r0;
  int64_t nactive;
  int64_t wstride;                  // words per slot
  int nw;                           // words of a slot that hold the batch: nkt * kSetPermTile / 64
  uint32_t h;
};
hipError_t launch_seq_masks(const SeqMaskArgs& a, hipStream_t stream);
hipError_t launch_seq_null(const SeqNullArgs& a, int method, hipStream_t stream);
hipError_t launch_seq_retire(const SeqRetireArgs& a, hipStream_t stream);

// ---- variable-threshold set tests: the best prefix of a set's member list (gcre_prefix.hip) ----
// One slab of whole sets.  Slot e of the slab is set which[e] of the caller's list; its step rows are rows [row0[e],
// row0[e + 1]) of the slab, in SetNullArgs' row layout.  k_prefix_rows builds them and their counts, k_set_observed scores
// them, k_prefix_pick takes every slot's best step and k_prefix_null the maximum over a slot's steps under every permutation.
struct PrefixWaveDev { int32_t slot, steps; int64_t row0; };   // gcre_prefix::PrefixWave: slot < 0 = no set
struct PrefixPick {
  double score;                 // the best observed score over the slot's steps, NaN if every step is NaN
  int32_t best_step;            // the smallest step that attains it, -1 for NaN
  int32_t cnt[4];               // cases_pos, ctrls_pos, cases_neg, ctrls_neg of that step (zeros for NaN)
  int32_t pad;
};
struct PrefixArgs {
  // k_prefix_rows
  const uint32_t* gene_rows;    // [n_rows][W2] the caller's gene rows as dwords (bits beyond the patients are ignored)
  const int64_t* set_off;       // [n_sets + 1] the caller's set list as it is
  const int32_t* members;       // rows of every set; none of a launched set is NA
  const int32_t* signs;         // per member +1 / -1, or nullptr = all +1 (read by method 2)
  const uint8_t* cut;           // per member: != 0 ends a step; nullptr = every member does
  const int64_t* which;         // [nslots] the set of every slot
  const int64_t* row0;          // [nslots + 1] first step row of every slot
  uint32_t* rows;               // [nrows][M][W32p] step rows: (+) half, then (-) half (method 2); zero beyond the patients
  int32_t* cnt;                 // [nrows][4] cases_pos, ctrls_pos, cases_neg, ctrls_neg; zero on entry (k_prefix_rows adds)
  // k_prefix_pick
  const double* obs;            // [nrows] observed score of every step row (k_set_observed)
  uint32_t* tot;                // [nrows][M] carriers per half
  uint32_t* thr;                // [nslots] f32 bit pattern: a permutation counts iff bits(T) >= thr
  PrefixPick* pick;             // [nslots]
  // k_prefix_null
  const PrefixWaveDev* waves;   // [nblocks][4] the block table
  const uint32_t* masks;        // [W32p][Kpad]
  const float* t32;             // M=1: sanitised f32 null table, diagonal-major
  const double* d64;            // M=2: f64 vtmax, diagonal-major
  const double* d64n;           // M=2: the table the (-) half reads
  unsigned long long* n_ge;     // [nslots], zero on entry
  uint32_t* null_max;           // optional [nslots][Kpad]: T as u32 bit patterns
  uint32_t* fam_bits;           // optional [Kpad] maxima over the slots (zero on entry; accumulates over the slabs)
  int64_t nslots, nrows;
  int nblocks;                  // blocks of four slots
  int W2;                       // dwords per gene row
  int W32p, Kpad, K;
  int nkt;                      // permutation tiles of kSetPermTile
  int n_patients, n_cases;
};
hipError_t launch_prefix_rows(const PrefixArgs& a, int method, hipStream_t stream);
hipError_t launch_prefix_pick(const PrefixArgs& a, int method, hipStream_t stream);
hipError_t launch_prefix_null(const PrefixArgs& a, int method, hipStream_t stream);

// ---- multi-hit set tests: the patients who carry at least m members of a set (gcre_dose.hip) ----
// k_dose_rows builds what k_prefix_rows builds -- the rows and counts of a PrefixArgs slab -- from a per-patient count of the
// set's members: row row0[e] + l of slot e is "carries at least level l of the set's members".  The rest of the slab's walk
// is the prefix stage's own (k_set_observed, k_prefix_pick, k_prefix_null).
struct DoseArgs {
  const uint32_t* gene_rows;    // [n_rows][W2] the caller's gene rows as dwords (bits beyond the patients are ignored)
  const int64_t* set_off;       // [n_sets + 1] the caller's set list as it is
  const int32_t* members;       // rows of every set; none of a launched set is NA
  const int32_t* signs;         // per member +1 / -1, or nullptr = all +1 (read by method 2)
  const int64_t* which;         // [nslots] the set of every slot
  uint32_t* rows;               // [nslots * n_levels][M][W32p] level rows: (+) half, then (-) half (method 2); zero beyond the patients
  int32_t* cnt;                 // [nslots * n_levels][4] cases_pos, ctrls_pos, cases_neg, ctrls_neg; zero on entry (the kernel adds)
  uint64_t levels;              // level l in bits [4 l, 4 l + 4): 1 .. 15, ascending
  int64_t nslots;
  int n_levels;                 // 1 .. 15
  int W2;                       // dwords per gene row
  int W32p;
  int n_patients, n_cases;
};
hipError_t launch_dose_rows(const DoseArgs& a, int method, hipStream_t stream);

// ---- sequential p-values of the two adaptive set tests (gcre_seq_prefix.hip) ----
// One batch of permutations (SeqNullArgs' masks and bit rows) against the step rows of one PrefixArgs slab.  Slot i of the
// active list is slot active[i] of the slab, its step rows [row0[e], row0[e + 1]).  Block (kt, g) stays on permutation tile
// kt and walks the groups g, g + pgroups, ... of four consecutive slots of the active list, one slot per wave.
struct SeqPrefixArgs {
  const uint32_t* rows;         // [nrows][M][W32p] the slab's step rows
  const uint32_t* masks;        // [W32p][stride] the batch's masks
  const uint32_t* tot;          // [nrows][M] carriers per half
  const uint32_t* thr;          // [nslots] f32 bit pattern of every slot's best observed score (k_prefix_pick)
  const int64_t* row0;          // [nslots + 1] first step row of every slot (read-only: scalar loads)
  const float* t32;             // M=1: sanitised f32 null table, diagonal-major
  const double* d64;            // M=2: f64 vtmax, diagonal-major
  const double* d64n;           // M=2: the table the (-) half reads
  const uint32_t* active;       // [nactive] slots of the slab (read-only: scalar loads), in any order
  unsigned long long* bits;     // [nactive][stride / 64]: bit i of slot a = the maximum of permutation r0 + i reached the score
  int64_t nactive;
  int64_t ngroups;              // ceil(nactive / 4)
  int W32p, stride, K;          // K: permutations of the batch; the columns K .. nkt * kSetPermTile - 1 write 0
  int nkt;                      // permutation tiles of kSetPermTile
  int pgroups;                  // blocks per permutation tile
};
hipError_t launch_seq_prefix_null(const SeqPrefixArgs& a, int method, hipStream_t stream);

// ---- stratified set scores: per-stratum counts and tables, summed (gcre_strata.hip) ----
// k_strata_masks turns the stratum ids into S indicator rows; the check launch counts every resident mask against them.
// Then one slab of whole sets: slot e of the slab has the S consecutive rows [e S, e S + S), row e S + s = "union & Z_s" in
// SetNullArgs' row layout.  k_strata_rows builds them and their counts from the union rows the set stage left,
// k_strata_observed makes the totals, the observed terms and their sum, k_strata_null the sum under every permutation.
struct StrataArgs {
  // k_strata_masks, the check
  const int32_t* stratum;       // [n_patients] ids 0 .. S-1
  uint32_t* zrows;              // [S][W32p] indicator rows; zero beyond the patients
  const uint32_t* cases_in;     // [S] cases of every stratum: what every mask must count inside Z_s
  unsigned int* violations;     // one dword, zero on entry: (stratum, permutation) pairs that do not
  // k_strata_rows
  const uint32_t* urows;        // [nslots][M][W32p] the slab's union rows as the set stage left them
  uint32_t* rows;               // [nslots S][M][W32p] stratum rows: (+) half, then (-) half (method 2)
  int32_t* cnt;                 // [nslots S][4] cases_pos, ctrls_pos, cases_neg, ctrls_neg; zero on entry (k_strata_rows adds)
  // k_strata_observed
  const double* dvt;            // the S diagonal-major tables, one behind the other
  const int64_t* doff;          // [S] where table s starts, in doubles (read-only: scalar loads)
  uint32_t* tot;                // [nslots S][M] carriers per half
  double* obs;                  // [nslots] the sum of the observed terms
  double* terms;                // optional [nslots][S]
  // k_strata_null
  const PrefixWaveDev* waves;   // [nblocks][4] the block table (gcre_prefix.h, every slot with S steps)
  const uint32_t* masks;        // [W32p][Kpad]
  unsigned long long* n_ge;     // [nslots], zero on entry
  double* null_scores;          // optional [nslots][Kpad]
  unsigned long long* fam_bits; // optional [Kpad] maxima over the slots as bit patterns of non-negative doubles (zero on
                                // entry; accumulates over the slabs)
  int64_t nslots;
  int nblocks;                  // blocks of four slots
  int S;                        // strata, 1 .. 16
  int W32p, Kpad, K;
  int nkt;                      // permutation tiles of kSetPermTile
  int n_patients, n_cases;
};
hipError_t launch_strata_masks(const StrataArgs& a, hipStream_t stream);
hipError_t launch_strata_check(const StrataArgs& a, hipStream_t stream);
hipError_t launch_strata_rows(const StrataArgs& a, int method, hipStream_t stream);
hipError_t launch_strata_observed(const StrataArgs& a, int method, hipStream_t stream);
hipError_t launch_strata_null(const StrataArgs& a, int method, hipStream_t stream);

// ---- covariate-adjusted permutation masks (gcre_weighted.hip; the law and the rule: gcre_weighted.h) ----
// k_weighted_search finds the accepted attempt of every (permutation, stratum), one wave each, and writes no mask bit;
// k_weighted_write, launched only when nothing was left over, rebuilds the accepted attempts' bits a lane per permutation.
struct WeightedArgs {
  uint64_t seed1;               // wt_seed(seed)
  const int32_t* cols;          // per stratum, one behind the other: the columns of Z_s ...
  const uint32_t* cthr;         // ... and their thresholds, in the same order
  const uint32_t* soff;         // [S + 1] where stratum s starts in cols / cthr
  const uint32_t* cases_in;     // [S]
  uint32_t* att;                // [S][K] accepted attempts, kWeightedNone where the cap was met
  unsigned int* left;           // one dword, zero on entry: (r, s) pairs without an accepted attempt
  uint32_t cap;                 // max_attempts
  // k_weighted_write
  const int32_t* stratum;       // [n] or NULL (one stratum)
  const uint32_t* thr;          // [n] thresholds by column
  uint32_t* masks;              // [W32p][Kpad]
  int S, K, n, W32p, Kpad;
};
hipError_t launch_weighted_search(const WeightedArgs& a, hipStream_t stream);
hipError_t launch_weighted_write(const WeightedArgs& a, hipStream_t stream);

// ---- weighted sequential p-values: one batch of covariate-adjusted masks (gcre_seq_weighted.hip) ----
// Permutations [r0, r0 + nb) of the weighted rule in k_seq_null's batch layout.  k_seq_weighted_search finds the accepted
// attempts of the batch's columns and the first column without one; k_seq_weighted_write, launched on the columns in front of
// it, writes their masks as k_seq_masks would: [W32p][stride] dwords, the columns nb .. stride-1 and the rows beyond the
// patients zero.
struct SeqWeightedArgs {
  uint64_t seed1;               // wt_seed(seed)
  uint64_t r0;                  // the first permutation of the batch
  const int32_t* cols;          // per stratum, one behind the other: the columns of Z_s ...
  const uint32_t* cthr;         // ... and their thresholds, in the same order
  const uint32_t* soff;         // [S + 1] where stratum s starts in cols / cthr
  const uint32_t* cases_in;     // [S]
  uint32_t* att;                // [S][att_stride] accepted attempts of the batch's columns, kWeightedNone where the cap was met
  uint32_t* first;              // one dword, 0xffffffff on entry: the smallest column with a stratum that met the cap
  uint32_t cap;                 // max_attempts
  // k_seq_weighted_write
  const int32_t* stratum;       // [n] or NULL (one stratum)
  const uint32_t* thr;          // [n] thresholds by column
  uint32_t* masks;              // [W32p][stride]
  int S, n, W32p;
  int nb;                       // columns of the batch: searched (<= att_stride), written (<= stride)
  int att_stride;               // columns of `att` per stratum
  int stride;                   // columns of `masks` per row: a multiple of 64
};
hipError_t launch_seq_weighted_search(const SeqWeightedArgs& a, hipStream_t stream);
hipError_t launch_seq_weighted_write(const SeqWeightedArgs& a, hipStream_t stream);

// ---- carrier-overlap counts of caller-given sets (gcre_overlap.hip) ----
constexpr int kOverlapTile = 64;    // pairs per edge of a block's tile
constexpr int kOverlapChunk = 32;   // dwords of a row per staged chunk (128 bytes): rows are padded to a multiple of it
struct OverlapArgs {
  const uint32_t* rows;         // [valid sets + 1][Wdp] carrier rows as dwords, zero beyond the n patients; the last is all zeros
  const int32_t* ia;            // [na] row of `rows` per pair row of this launch (the zero row: a set with an NA member)
  const int32_t* ib;            // [nb] the same for the pair columns
  int32_t* both;                // [na][nb][2] cases, controls
  int64_t na, nb;
  int64_t ntb;                  // column tiles: ceil(nb / kOverlapTile)
  int Wdp;                      // dwords per row, a multiple of kOverlapChunk
  int n_cases;                  // columns below it are the cases
  int zero_row;                 // the all-zero row of `rows`
};
hipError_t launch_set_overlap(const OverlapArgs& a, hipStream_t stream);

// ---- greedy carrier clumping on the device (gcre_clump.hip) ----
// Everything is indexed by POSITION in the walk order.  A round takes the next <= kClumpCand unassigned positions as
// candidate leads, resolves them among themselves (k_clump_leads) and lets the true leads absorb every later row
// (k_clump_assign).  The state of a round lives on the device, so rounds are queued without the host looking.
constexpr int kClumpCand = 64;      // candidate leads of a round = the `a` edge of k_clump_assign's tile
struct ClumpState {                 // 16 bytes: what the host reads once per batch of rounds
  int32_t cursor;                   // every position below it is assigned; >= n: the walk is over
  int32_t ncand;                    // candidates of the last round (0: an empty round)
  int32_t nlead;                    // ... and the true leads among them, compacted in `leads`
  int32_t next_clump;               // clump ids handed out so far
};
enum ClumpStat { kClumpRounds = 0, kClumpTilesRun = 1, kClumpTilesSkipped = 2, kClumpStats = 4 };
struct ClumpArgs {
  uint32_t* U;                      // [n + 1][Wdp] union rows in k_set_overlap's layout; row n is all zeros
  int32_t* cnt;                     // [n][2] carriers of every position: cases, controls
  uint32_t* free_;                  // [n] 1 = not assigned yet
  int32_t* clump;                   // [n] outputs per position: clump id,
  int32_t* lead;                    // [n] the lead's POSITION (a lead names itself),
  double* value;                    // [n] the measure against the lead (NaN on a lead),
  int32_t* shared;                  // [n][2] carriers shared with the lead ((-1, -1) on a lead)
  ClumpState* state;
  int32_t* leads;                   // [kClumpCand] positions of the round's true leads, in walk order
  unsigned long long* stats;        // [kClumpStats]
  int64_t n;                        // positions
  int Wdp;                          // dwords per union row, a multiple of kOverlapChunk
  int n_cases;
  int measure;                      // 0 jaccard, 1 containment
  int patients;                     // 0 all, 1 cases
  double r;
};
struct ClumpUnionArgs {
  const uint32_t* rows;             // [n_rows][W2] the caller's gene rows as dwords
  const int32_t* members;           // [n][M] rows of every position's set, -1 = no further member
  int M, W2, n_patients;
};
hipError_t launch_clump_union(const ClumpArgs& a, const ClumpUnionArgs& u, hipStream_t stream);
// one round: k_clump_leads, then k_clump_assign over the tiles from `tile0` on (positions below 64 * tile0 are assigned)
hipError_t launch_clump_round(const ClumpArgs& a, int64_t tile0, hipStream_t stream);

// ---- carrier tallies per patient (gcre_patients.hip) ----
// The kept entries are sorted by group and cut into segments of one group each.  One wave adds a segment's carrier rows
// up over one tile of kPatientTile patients in bit-sliced counters of kPatientPlanes planes (gcre_bitslice.h) and flushes
// them into the group's 32-bit cells before they can overflow: after at most 2^kPatientPlanes - 1 entries.
constexpr int kPatientPlanes = 12;
constexpr int kPatientTile = 2048;                   // patients per wave: one dword column per lane
constexpr int32_t kPatientNegBit = 1 << 30;          // by_sign: set on a table entry whose member has sign -1
struct PatientSeg {
  int32_t begin, count;             // entries [begin, begin + count) of the table
  int32_t group;
  int32_t width;                    // the most members of one of its entries, <= M: the member columns the wave reads
};
struct PatientCountArgs {
  const uint32_t* rows;             // [n_rows][W2] the caller's gene rows as dwords (bits beyond the patients are ignored)
  const int32_t* members;           // [M][n] member m of every kept entry's set, -1 = no further member (read-only: scalar loads)
  const PatientSeg* segs;           // [nseg] (read-only)
  uint32_t* cells;                  // [n_groups][H][n_patients], zeroed
  int64_t n, nseg;                  // kept entries, segments
  int M, W2, n_patients;
  int H;                            // 1: all members into one plane; 2: the (+) members, then the (-) members
};
hipError_t launch_set_patient_counts(const PatientCountArgs& a, hipStream_t stream);

// ---- burden tests of per-patient weights (gcre_burden.hip) ----
// The rows of a slab that have a non-zero weight are listed (`act`); each gets the bit planes its largest weight needs,
// [Wp] 64-bit words per plane in SetNullArgs' row layout.  An item is up to kBurdenItemPlanes consecutive planes of one
// row: one wave of k_burden_null counts it against a tile of kSetPermTile permutations.
constexpr int kBurdenItemPlanes = 4;
constexpr int kBurdenMaxPlanes = 31;                 // weights are non-negative int32
struct BurdenItem {
  int32_t row;                      // row of the slab: sums[row][..]
  int32_t plane;                    // its first plane, as an index into the slab's planes
  int32_t count;                    // 1 .. kBurdenItemPlanes planes
  int32_t base;                     // the bit the first plane holds
};
struct BurdenPlaneArgs {
  const int32_t* w;                 // [slab rows][n] weights, >= 0
  const int32_t* act;               // [nact] rows of the slab with a non-zero weight
  const int32_t* nplanes;           // [nact] 1 .. kBurdenMaxPlanes
  const int32_t* pbase;             // [nact] first plane of the row
  uint32_t* planes;                 // [sum nplanes][2 * Wp], every word written (zero beyond the patients)
  int64_t nact;
  int n, Wp;
};
struct BurdenNullArgs {
  const uint32_t* planes;           // [..][W32p] (read-only: scalar loads)
  const uint32_t* masks;            // [W32p][Kpad]
  const BurdenItem* items;          // [nitems] (read-only)
  unsigned long long* sums;         // [slab rows][Kpad], zeroed; permutations K .. Kpad are never written
  int64_t nitems, npt;              // npt = ceil(nitems / 4) item tiles
  int nkt, pgroups;                 // permutation tiles; item tiles walked in parallel: grid = nkt * pgroups
  int W32p, Kpad, K;
};
struct BurdenFinishArgs {
  const unsigned long long* sums;   // [slab rows][Kpad]
  const int32_t* act;               // [nact]
  const int64_t* observed;          // [nact]
  unsigned long long* tails;        // [nact][2] n_ge, n_le, zeroed
  int64_t nact;
  int Kpad, K;
};
hipError_t launch_burden_planes(const BurdenPlaneArgs& a, hipStream_t stream);
hipError_t launch_burden_null(const BurdenNullArgs& a, hipStream_t stream);
hipError_t launch_burden_finish(const BurdenFinishArgs& a, hipStream_t stream);

}  // namespace gcre

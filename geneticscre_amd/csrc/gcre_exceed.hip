// gcre_exceed.hip -- null exceedance counts (gcre_exceed): for a list of thresholds, how many (joined path,
// permutation) pairs of a join have a null score at or above each, and how many joined paths an observed score.
//   * k_exceed_ie        the hot path: the count work of the general inclusion-exclusion kernel k_null_ie (gcre_ie.hip: base
//                        counters from planes / recipe / streamed list, per path B + Nz - S or B + S, per-XCD item order,
//                        score_begin / score_end) -- a copy, so that the null kernels' code objects do not move -- with
//                        another finish (below).  It keeps no running maxima, writes no planes and never touches null_bits
//   * k_exceed_dense     fallback and cross-check: k_null's mapping (gcre_kernels.hip: mask tile through LDS, joined-path
//                        words as wave-uniform scalar loads, lanes own R permutations) with the same finish
//   * k_exceed_observed  one lane per joined path over a chunk's score keys against the sorted threshold keys
// The finish: the value every (path, permutation) folds into the join's maxima is compared, as its u32 bit pattern, against
// the LOWEST threshold's pattern (one register).  Null values are non-negative floats, ordered as their bits; the host turns
// threshold t into the pattern of the smallest float x with (double)x >= t (0 for t <= 0: everything counts).  Only when
// some lane of the wave passes are the passing values compacted into the wave's LDS queue (ballot + mbcnt) and drained by
// one loop that locates each among the sorted patterns (binary search) and counts it in ONE bin, that of the largest
// pattern not above it; exceed[j] is the sum of the bins from j upwards, taken on the host in 64 bits.
//
// Bins are a per-block u32 histogram in LDS while the thresholds fit (kExceedLdsBinsIe / kExceedLdsBinsDense: what leaves
// the occupancy of the count loop alone), moved into the u64 bins in global memory with 64-bit vector atomics; beyond that
// a drained value adds to the global bin itself (a pass is rare for any threshold a user cares about).  32-bit bins cannot
// overflow between flushes:
//   dense  a block adds at most 4 TPW x 64 R <= 16,384 hits per path tile (TPW R <= 64 in every instance) and flushes
//          after kExceedFlushTiles = 65,536 path tiles: 2^30 per bin at the very most
//   ie     a wave adds at most 2,048 hits per (path, tile) and flushes ALL the block's bins (atomic exchange with 0, so
//          the other waves may go on adding) after kExceedFlushPaths = 262,144 of them; a bin holds what the four waves
//          added since their own last flush: 4 x 2^18 x 2^11 = 2^31 at the very most
// Every global write is a vector atomic.
//
// Per-permutation counts (PC instantiations): a passing value goes into the queue together with its
// permutation's index inside the tile (16 bits, in a queue of its own), and the drain loop, next to the histogram bin, adds
// 1 to the u32 cell pc[bin * stride + absolute permutation] in global memory -- no LDS staging: a pass is rare, and one
// (bin, permutation) cell is hit by different waves at different times.  The instantiations without PC are the code they
// were: `if constexpr`, and the three fields at the end of the argument structs, which they do not read.
#include "gcre_ie_common.h"


namespace gcre {
namespace {

typedef u32 __attribute__((ext_vector_type(2))) u32x2;
typedef u32 __attribute__((ext_vector_type(8))) u32x8;

__device__ __forceinline__ u32 exc_diag(u32 t) { return (u32)(((u64)t * (u64)(t + 1)) >> 1); }

constexpr int kExceedFlushTiles = 65536;
constexpr int kExceedFlushPaths = 262144;
constexpr int kExceedQueue = 512;   // entries of a wave's queue: 8 values per lane and round
constexpr int kObsBlock = 256;
constexpr int kObsBlocksPerCu = 8;

template <int R>
__device__ __forceinline__ void exc_mask_row(const u32* lds_row, int lane, u32 (&m)[R]) {
  if constexpr (R == 1) {
    m[0] = lds_row[lane];
  } else if constexpr (R == 2) {
    u32x2 v = *(const u32x2*)(lds_row + lane * 2);
    m[0] = v.x; m[1] = v.y;
  } else if constexpr (R == 4) {
    u32x4 v = *(const u32x4*)(lds_row + lane * 4);
    m[0] = v.x; m[1] = v.y; m[2] = v.z; m[3] = v.w;
  } else {
    static_assert(R == 8, "R in {1,2,4,8}");
    u32x4 v = *(const u32x4*)(lds_row + lane * 4);
    u32x4 w = *(const u32x4*)(lds_row + 256 + lane * 4);
    m[0] = v.x; m[1] = v.y; m[2] = v.z; m[3] = v.w;
    m[4] = w.x; m[5] = w.y; m[6] = w.z; m[7] = w.w;
  }
}

// column of the permutation tile that register j of a lane holds (k_null's layout)
template <int R>
__device__ __forceinline__ int exc_col(int lane, int j) {
  return (R == 8) ? ((j >> 2) * 256 + lane * 4 + (j & 3)) : (lane * R + j);
}

template <int WC> struct ExcChunk;
template <> struct ExcChunk<4> { typedef u32x4 type; };
template <> struct ExcChunk<8> { typedef u32x8 type; };

// the bin of a value that reached the lowest threshold: the last of the ascending patterns that is <= v
template <typename T>
__device__ __forceinline__ int exc_bin(const T* pat, int m, T v) {
  int lo = 1, hi = m;   // (pat[0] <= v is known) first index whose pattern is above v
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pat[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

// (other waves of the block may be adding: the bin is taken with an exchange)
__device__ __forceinline__ void exc_flush(u32* bins, int n, unsigned long long* hist, int tid, int nthreads) {
  for (int i = tid; i < n; i += nthreads) {
    if (bins[i] == 0u) continue;
    const u32 v = atomicExch(&bins[i], 0u);
    if (v != 0u) atomicAdd(hist + i, (unsigned long long)v);
  }
}

// where a kernel's counts go
struct ExcBins {
  const u32* pat;             // [m] ascending
  int m;
  u32* lds;                   // the block's histogram, or nullptr: straight into hist
  unsigned long long* hist;
};

// N values per lane of which some lane's pass (the caller has voted): the passing ones go into the wave's queue in lane
// order, then the wave walks the queue.  Every lane of the wave calls it.
template <int N>
__device__ __forceinline__ void exc_emit(const u32 (&v)[N], const bool (&pass)[N], u32* queue, const ExcBins& b, int lane) {
  static_assert(64 * N <= kExceedQueue, "queue");
  u32 n = 0;
#pragma unroll
  for (int j = 0; j < N; j++) {
    const u64 bal = __ballot(pass[j]);
    const u32 pos = n + __builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u));
    if (pass[j]) queue[pos] = v[j];
    n += (u32)__popcll(bal);
  }
  __builtin_amdgcn_wave_barrier();   // (a wave's LDS accesses are served in order)
  for (u32 i = (u32)lane; i < n; i += 64u) {
    const u32 x = queue[i];
    const int bin = exc_bin(b.pat, b.m, x);
    if (b.lds) atomicAdd(&b.lds[bin], 1u);
    else atomicAdd(b.hist + bin, 1ull);
  }
  __builtin_amdgcn_wave_barrier();
}

// where a kernel's per-permutation counts go
struct ExcPerm {
  u32* pc;        // [m][stride]
  u32 stride;
  u32 base;       // absolute permutation of the tile's column 0 (window start + tile start)
};

// The same with per-permutation counts: col(lane, j) < 2048 is the column of value j inside the permutation tile.  A
// passing value is a live column of the window (the caller's `pass`): base + col < the context's permutations <= stride.
// The columns are functions of the lane alone; they are made here, on the rare road, from a lane index the optimiser
// cannot see through -- otherwise it keeps all of them in registers across the count loop (28 more VGPRs in k_exceed_ie).
template <int N, typename Col>
__device__ __forceinline__ void exc_emit_pc(const u32 (&v)[N], const bool (&pass)[N], Col col, u32* queue,
                                            unsigned short* pqueue, const ExcBins& b, const ExcPerm& pp, int lane) {
  static_assert(64 * N <= kExceedQueue, "queue");
  int lane_here = lane;
  asm volatile("" : "+v"(lane_here));
  u32 n = 0;
#pragma unroll
  for (int j = 0; j < N; j++) {
    const u64 bal = __ballot(pass[j]);
    const u32 pos = n + __builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u));
    if (pass[j]) {
      queue[pos] = v[j];
      pqueue[pos] = (unsigned short)col(lane_here, j);
    }
    n += (u32)__popcll(bal);
  }
  __builtin_amdgcn_wave_barrier();   // (a wave's LDS accesses are served in order)
  for (u32 i = (u32)lane; i < n; i += 64u) {
    const u32 x = queue[i];
    const u32 r = pp.base + (u32)pqueue[i];
    const int bin = exc_bin(b.pat, b.m, x);
    if (b.lds) atomicAdd(&b.lds[bin], 1u);
    else atomicAdd(b.hist + bin, 1ull);
    atomicAdd(pp.pc + ((size_t)bin * pp.stride + r), 1u);
  }
  __builtin_amdgcn_wave_barrier();
}

// M, R, TPW, WC, OCC as k_null; PC: per-permutation counts too
template <int M, int R, int TPW, int WC, int OCC, bool PC>
__global__ __launch_bounds__(kNullBlock, OCC) void k_exceed_dense(const ExceedArgs a) {
  typedef typename ExcChunk<WC>::type rowv;
  constexpr int NW = kNullBlock / 64;
  constexpr int PT = 64 * R;
  constexpr int TPB = NW * TPW;
  constexpr int CHUNK = WC * PT;
  constexpr int VEC = CHUNK / 4 / kNullBlock;
  static_assert(CHUNK % (4 * kNullBlock) == 0 || CHUNK < 4 * kNullBlock, "staging shape");
  static_assert(TPB * PT <= 16384, "hits per path tile and bin (flush rule)");

  __shared__ __attribute__((aligned(16))) u32 lds[2][CHUNK];
  __shared__ u32 queue_lds[NW][64 * R];
  __shared__ unsigned short pqueue_lds[PC ? NW : 1][PC ? 64 * R : 1];
  extern __shared__ u32 bins[];   // a.lds_bins words

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = blockIdx.x % a.nkt;
  const int g = blockIdx.x / a.nkt;

  const u32 GCRE_CONSTANT* P0 = as_const(a.p0);
  const u32 GCRE_CONSTANT* P1 = as_const(a.p1);
  const u32 GCRE_CONSTANT* ROW0 = as_const(a.row0);
  const u32 GCRE_CONSTANT* ROW1 = as_const(a.row1);
  const u32 GCRE_CONSTANT* TOT = as_const(a.tot);

  const int nchunks = a.W32p / WC;
  const u32* mask_tile = a.masks + (size_t)kt * PT;

  constexpr int NV = (VEC > 0) ? VEC : 1;
  u32x4 stage[NV];
  u32 voff[NV];
#pragma unroll
  for (int i = 0; i < NV; i++) {
    const int e = tid + i * kNullBlock;
    voff[i] = (u32)((e / (PT / 4)) * a.Kpad + (e % (PT / 4)) * 4) * 4u;
  }
  const size_t chunk_bytes = (size_t)WC * a.Kpad * 4;
  auto stage_load = [&](int c) {
    const char* cb = (const char*)mask_tile + (size_t)c * chunk_bytes;
#pragma unroll
    for (int i = 0; i < NV; i++)
      if (VEC > 0 || tid + i * kNullBlock < CHUNK / 4) stage[i] = *(const u32x4*)(cb + voff[i]);
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NV; i++) {
      const int e = tid + i * kNullBlock;
      if (VEC > 0 || e < CHUNK / 4) *(u32x4*)(&lds[buf][e * 4]) = stage[i];
    }
  };

  for (int i = tid; i < a.lds_bins; i += kNullBlock) bins[i] = 0u;

  // permutations K.. of the last tile are padding: they never count
  const int live_cols = a.K - kt * PT;
  const u32 pat0 = a.pat[0];

  const ExcBins eb{a.pat, a.m, a.lds_bins ? bins : nullptr, a.hist};
  u32* const queue = queue_lds[wave];
  unsigned short* const pqueue = pqueue_lds[PC ? wave : 0];
  const ExcPerm pp{a.pc, (u32)a.pc_stride, (u32)(a.k0 + kt * PT)};
  auto emit = [&](const u32 (&v)[R], const bool (&pass)[R]) {
    if constexpr (PC) {
      exc_emit_pc<R>(v, pass, [](int l, int j) { return exc_col<R>(l, j); }, queue, pqueue, eb, pp, lane);
    } else {
      exc_emit<R>(v, pass, queue, eb, lane);
    }
  };

  stage_load(0);
  stage_store(0);
  __syncthreads();
  int buf = 0;
  int tiles = 0;

  const u32 s8 = (u32)(a.S32 >> 3);
  const u32 h8 = (u32)(a.W32p >> 3);
  const i64 last = a.npaths - 1;

  for (i64 pt = g; pt < a.npt; pt += a.pgroups) {
    const i64 qbase = pt * TPB + (i64)wave * TPW;
    u32 acc[M][TPW][R];
#pragma unroll
    for (int h = 0; h < M; h++)
#pragma unroll
      for (int t = 0; t < TPW; t++)
#pragma unroll
        for (int j = 0; j < R; j++) acc[h][t][j] = 0u;

    // a path past the end reads the last path's rows (its counts are dropped): nothing beyond [0, npaths) is touched
    u32 o0[TPW], o1[TPW], o1n[TPW];
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const i64 q = qbase + t < a.npaths ? qbase + t : last;
      const u32 r0 = ROW0[q];
      const u32 r1raw = ROW1[q];
      o0[t] = r0 * s8;
      o1[t] = (r1raw & 0x7fffffffu) * s8;
      o1n[t] = o1[t];
      if constexpr (M == 2) {
        const u32 swap = r1raw >> 31;
        o1n[t] = o1[t] + (swap ? 0u : h8);
        o1[t] = o1[t] + (swap ? h8 : 0u);
      }
    }

    rowv nx[M], ny[M];
    auto fetch = [&](int c, int t) {
      const u32 GCRE_CONSTANT* b0 = P0 + (size_t)c * WC;
      const u32 GCRE_CONSTANT* b1 = P1 + (size_t)c * WC;
      nx[0] = *(const rowv GCRE_CONSTANT*)(b0 + ((size_t)o0[t] << 3));
      ny[0] = *(const rowv GCRE_CONSTANT*)(b1 + ((size_t)o1[t] << 3));
      if constexpr (M == 2) {
        nx[M - 1] = *(const rowv GCRE_CONSTANT*)(b0 + ((size_t)(o0[t] + h8) << 3));
        ny[M - 1] = *(const rowv GCRE_CONSTANT*)(b1 + ((size_t)o1n[t] << 3));
      }
    };
    fetch(0, 0);

    for (int c = 0; c < nchunks; c++) {
      const int cn = (c + 1 == nchunks) ? 0 : c + 1;
      stage_load(cn);

      u32 m[WC][R];
#pragma unroll
      for (int w = 0; w < WC; w++) exc_mask_row<R>(&lds[buf][w * PT], lane, m[w]);

#pragma unroll
      for (int t = 0; t < TPW; t++) {
        rowv jn[M];
#pragma unroll
        for (int h = 0; h < M; h++)
#pragma unroll
          for (int w = 0; w < WC; w++) jn[h][w] = __builtin_amdgcn_readfirstlane(nx[h][w] | ny[h][w]);
        if (t + 1 < TPW) fetch(c, t + 1);
        else fetch(cn, 0);
#pragma unroll
        for (int h = 0; h < M; h++)
#pragma unroll
          for (int w = 0; w < WC; w++)
#pragma unroll
            for (int j = 0; j < R; j++) acc[h][t][j] += __builtin_popcount(jn[h][w] & m[w][j]);
        __builtin_amdgcn_sched_barrier(0);
      }

      stage_store(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }

    // ---- the value k_null folds into the maxima, against the lowest threshold; the few that pass are binned ----
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      if (qbase + t < a.npaths) {   // wave-uniform
        if constexpr (M == 1) {
          const u32 total = TOT[qbase + t];
          const char* diag = (const char*)((const u32*)a.t32 + exc_diag(total));
          u32 v[R];
          bool pass[R], any = false;
#pragma unroll
          for (int j = 0; j < R; j++) v[j] = *(const u32*)(diag + (acc[0][t][j] << 2));
#pragma unroll
          for (int j = 0; j < R; j++) {
            pass[j] = v[j] >= pat0 && exc_col<R>(lane, j) < live_cols;
            any = any || pass[j];
          }
          if (__ballot(any)) emit(v, pass);
        } else {
          const u32 tp = TOT[2 * (qbase + t)];
          const u32 tn = TOT[2 * (qbase + t) + 1];
          const char* dp = (const char*)(a.d64 + exc_diag(tp));
          const char* dn = (const char*)(a.d64n + exc_diag(tn));
          u32 v[R];
          bool pass[R], any = false;
#pragma unroll
          for (int j = 0; j < R; j++) {
            const double s = *(const double*)(dp + (acc[0][t][j] << 3)) + *(const double*)(dn + (acc[M - 1][t][j] << 3));
            float f = (float)s;
            f = (f > 0.0f) ? f : 0.0f;   // NaN and negatives fold as 0, as into the join's maxima
            v[j] = __float_as_uint(f);
            pass[j] = v[j] >= pat0 && exc_col<R>(lane, j) < live_cols;
            any = any || pass[j];
          }
          if (__ballot(any)) emit(v, pass);
        }
      }
    }

    if (++tiles == kExceedFlushTiles) {   // (block-uniform: every thread of the block walks the same path tiles)
      tiles = 0;
      __syncthreads();
      exc_flush(bins, a.lds_bins, a.hist, tid, kNullBlock);
      __syncthreads();
    }
  }

  __syncthreads();
  exc_flush(bins, a.lds_bins, a.hist, tid, kNullBlock);
}

template <int M, int R, int TPW, int WC, int OCC>
hipError_t launch_exceed_t(const ExceedArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)(a.nkt * a.pgroups));
  if (a.pc)
    hipLaunchKernelGGL((k_exceed_dense<M, R, TPW, WC, OCC, true>), grid, dim3(kNullBlock), (size_t)a.lds_bins * 4, stream, a);
  else
    hipLaunchKernelGGL((k_exceed_dense<M, R, TPW, WC, OCC, false>), grid, dim3(kNullBlock), (size_t)a.lds_bins * 4, stream, a);
  return hipGetLastError();
}

// One lane per joined path.  A block adds at most its share of `count` < 2^32 paths to a bin: no flush inside the walk.
__global__ __launch_bounds__(kObsBlock) void k_exceed_observed(const ExceedObsArgs a) {
  extern __shared__ u32 obins[];
  for (int i = threadIdx.x; i < a.lds_bins; i += kObsBlock) obins[i] = 0u;
  __syncthreads();
  const u64 key0 = a.tkey[0];
  const i64 stride = (i64)gridDim.x * kObsBlock;
  for (i64 i = (i64)blockIdx.x * kObsBlock + threadIdx.x; i < a.count; i += stride) {
    const u64 key = a.key[i];
    if (key == 0 || key < key0) continue;   // (0: not a score)
    const int b = exc_bin(a.tkey, a.m, key);
    if (a.lds_bins) atomicAdd(&obins[b], 1u);
    else atomicAdd(a.hist + b, 1ull);
  }
  __syncthreads();
  exc_flush(obins, a.lds_bins, a.hist, threadIdx.x, kObsBlock);
}

// ------------------------------------------------------------------------------------------------
// k_exceed_ie: k_null_ie's counts (gcre_ie.hip), every one looked up, none kept.  L = counter planes, a multiple of 4.
// Lane l holds permutations 32 l .. 32 l + 31 of the wave's current 2048-permutation tile; value q of a lane is
// permutation 2048 kt + 32 l + q, which counts only below a.K.
// ------------------------------------------------------------------------------------------------
struct ExceedIeArgs {
  IeArgs ie;
  const u32* pat;
  unsigned long long* hist;
  int m;
  int lds_bins;
  u32* pc;          // PC: [m][pc_stride] per-permutation counts
  int pc_stride;
  int k0;           // PC: absolute permutation of the window's first
};

// PC: per-permutation counts too.  (<2, 16, PC> comes out two VGPRs above its sibling's 167 when it may take two waves'
// worth of registers, and loses the third wave; told to fit three it does, without a spill.)
template <int M, int L, bool PC>
__global__ __launch_bounds__(64 * kIeWaves) __attribute__((amdgpu_waves_per_eu(M == 1 ? 4 : (PC && L == 16) ? 3 : 2))) void k_exceed_ie(const ExceedIeArgs xa) {
  static_assert(L % 4 == 0 && L >= 8 && L <= 16, "planes come in groups of 4");
  const IeArgs& a = xa.ie;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int xcd = blockIdx.x & 7;
  const i64 wi = (i64)(blockIdx.x >> 3) * kIeWaves + wave;
  const i64 wx = a.waves_per_xcd;
  const i64 slices = 8 * wx;
  const u32 lane4 = (u32)lane * 4u;
  __shared__ u32 queue_lds[kIeWaves][kExceedQueue];
  __shared__ unsigned short pqueue_lds[PC ? kIeWaves : 1][PC ? kExceedQueue : 1];
  extern __shared__ u32 bins[];   // xa.lds_bins words
  for (int i = threadIdx.x; i < xa.lds_bins; i += 64 * kIeWaves) bins[i] = 0u;
  __syncthreads();
  const ExcBins eb{xa.pat, xa.m, xa.lds_bins ? bins : nullptr, xa.hist};
  u32* const queue = queue_lds[wave];
  unsigned short* const pqueue = pqueue_lds[PC ? wave : 0];
  ExcPerm pp{xa.pc, (u32)xa.pc_stride, 0u};   // (base: set with the tile)
  const u32 pat0 = xa.pat[0];
  int counted = 0;   // (path, tile) items since the wave's last flush

  const SparseSeg GCRE_CONSTANT* segs = (const SparseSeg GCRE_CONSTANT*)a.segs;
  const u64 GCRE_CONSTANT* loff0 = (const u64 GCRE_CONSTANT*)a.loff0;
  const u32 GCRE_CONSTANT* lidx0 = (const u32 GCRE_CONSTANT*)a.lidx0;

  int cur_kt = -1;
  int live_q = 0;   // values 0 .. live_q-1 of this lane are permutations of the window
  __amdgpu_buffer_rsrc_t mt = __builtin_amdgcn_make_buffer_rsrc((void*)a.mt, 0, 0x7fffffff, 0x00020000);

  auto to_counts = [&](const u32 (&C)[L], u32 (&R)[16]) {
#pragma unroll
    for (int l = 0; l < 16; l++) R[l] = (l < L) ? C[l] : 0u;
    transpose16(R);
  };
  // eight values of the lane, v[k] = value q0 + k
  auto emit8 = [&](const u32 (&v)[8], int q0) {
    bool pass[8], any = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      pass[k] = v[k] >= pat0 && q0 + k < live_q;
      any = any || pass[k];
    }
    if (__ballot(any)) {
      if constexpr (PC) {
        exc_emit_pc<8>(v, pass, [q0](int l, int k) { return l * 32 + q0 + k; }, queue, pqueue, eb, pp, lane);
      } else {
        exc_emit<8>(v, pass, queue, eb, lane);
      }
    }
  };
  // method 1: counts -> f32 table diagonal (methods.h:96-103), all 32 table cells of the lane in flight together
  auto finish_m1 = [&](const u32 (&C)[L], u32 total) {
    u32 R[16];
    to_counts(C, R);
    const u32* diag_g = (const u32*)a.t32 + sp_diag_offset(total);
    u32 v[32];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      v[j] = diag_g[R[j] & 0xffffu];
      v[j + 16] = diag_g[R[j] >> 16];
    }
    bool any = false;
#pragma unroll
    for (int q = 0; q < 32; q++) any = any || (v[q] >= pat0 && q < live_q);
    if (!__ballot(any)) return;   // the common case for a threshold a user cares about
#pragma unroll
    for (int q0 = 0; q0 < 32; q0 += 8) {
      u32 w[8];
#pragma unroll
      for (int k = 0; k < 8; k++) w[k] = v[q0 + k];
      emit8(w, q0);
    }
  };
  // method 2: vtmax[a][tp-a] + vtmax[tn-b][b] in f64, rounded to f32, clamped at 0 (methods.h:220-230)
  auto finish_m2 = [&](const u32 (&Cp)[L], const u32 (&Cn)[L], u32 tp, u32 tn) {
    u32 Rp[16], Rn[16];
    to_counts(Cp, Rp);
    to_counts(Cn, Rn);
    const double* dp = a.d64 + sp_diag_offset(tp);
    const double* dn = a.d64 + sp_diag_offset(tn);
#pragma unroll
    for (int g0 = 0; g0 < 16; g0 += 4) {
      double sp[8], sn[8];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        sp[k] = dp[Rp[g0 + k] & 0xffffu];
        sn[k] = dn[Rn[g0 + k] & 0xffffu];
        sp[k + 4] = dp[Rp[g0 + k] >> 16];
        sn[k + 4] = dn[Rn[g0 + k] >> 16];
      }
      u32 lo[4], hi[4];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        float f = (float)(sp[k] + sn[k]);
        f = (f > 0.0f) ? f : 0.0f;
        if (k < 4) lo[k] = __float_as_uint(f);
        else hi[k - 4] = __float_as_uint(f);
      }
      // values g0 .. g0+3 and g0+16 .. g0+19: two half rounds of the queue
      bool pass[8], any = false;
      u32 v[8];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        v[k] = lo[k];
        v[k + 4] = hi[k];
        pass[k] = lo[k] >= pat0 && g0 + k < live_q;
        pass[k + 4] = hi[k] >= pat0 && g0 + k + 16 < live_q;
        any = any || pass[k] || pass[k + 4];
      }
      if (__ballot(any)) {
        if constexpr (PC) {
          exc_emit_pc<8>(v, pass, [g0](int l, int k) { return l * 32 + g0 + (k < 4 ? k : k + 12); }, queue, pqueue, eb, pp, lane);
        } else {
          exc_emit<8>(v, pass, queue, eb, lane);
        }
      }
    }
  };

  auto load_planes = [&](u32 (&P)[L], const u32* planes, u32 unit, int groups) {
    const u32x4* src = (const u32x4*)(planes + (u64)unit * 256u) + lane;
#pragma unroll
    for (int j = 0; j < L / 4; j++) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (j < groups) v = src[j * 64];
      P[4 * j + 0] = v.x;
      P[4 * j + 1] = v.y;
      P[4 * j + 2] = v.z;
      P[4 * j + 3] = v.w;
    }
  };

  for (int step = 0; step < a.nkt; step++) {
    const i64 item = (i64)xcd * a.nkt * wx + wi + (i64)step * wx;
    const int kt = (int)(item / slices);
    const i64 sl = item % slices;
    if (kt != cur_kt) {
      cur_kt = kt;
      live_q = a.K - kt * 2048 - lane * 32;
      if constexpr (PC) pp.base = (u32)(xa.k0 + kt * 2048);
      mt = __builtin_amdgcn_make_buffer_rsrc((void*)(a.mt + (size_t)kt * a.mt_rows * 64), 0, 0x7fffffff, 0x00020000);
    }
    for (i64 sidx = a.seg_begin + sl; sidx < a.seg_end; sidx += slices) {
      const u32 row0 = segs[sidx].row0;
      const u32 first = segs[sidx].first;
      const u32 npaths = segs[sidx].n;
      const u32 qv = first + (((u32)lane < npaths) ? (u32)lane : 0u);
      u32 infov[M], lovv[M];
#pragma unroll
      for (int h = 0; h < M; h++) {
        infov[h] = a.linfo[(u64)qv * M + h];
        lovv[h] = a.lover[(u64)qv * M + h];
      }
      const u32 rzv = a.rowz[qv];
      u32 zunit[M];
#pragma unroll
      for (int h = 0; h < M; h++) {
        const u32 hz = (M == 2 && (rzv >> 31)) ? (u32)(1 - h) : (u32)h;
        zunit[h] = ((u32)kt * (u32)a.rowsz + (rzv & 0x7fffffffu) * (u32)M + hz) * (u32)a.gz;
      }
      u32 ttv[M];
#pragma unroll
      for (int h = 0; h < M; h++) ttv[h] = a.tot[(u64)qv * M + h];
      u32 lv[M][8];
#pragma unroll
      for (int h = 0; h < M; h++) {
        const u32x4* lp = (const u32x4*)(a.dlist + ((u64)qv * M + h) * 8u);
        const u32x4 e0 = lp[0], e1 = lp[1];
        lv[h][0] = e0.x; lv[h][1] = e0.y; lv[h][2] = e0.z; lv[h][3] = e0.w;
        lv[h][4] = e1.x; lv[h][5] = e1.y; lv[h][6] = e1.z; lv[h][7] = e1.w;
      }

      auto stream = [&](u32 (&P)[L], const u32 GCRE_CONSTANT* list, u64 p, u64 e) {
        u32 x[16];
        for (; p + 16 <= e; p += 16) {
          load16(x, mt, lane4, *(const u32x16 GCRE_CONSTANT*)(list + p));
          add16<L>(P, x);
        }
        for (; p < e; p += 4) {
          const u32x4 offs = *(const u32x4 GCRE_CONSTANT*)(list + p);
          u32 y4[4];
#pragma unroll
          for (int j = 0; j < 4; j++) y4[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, offs[j], 0);
          add4<L>(P, y4);
        }
      };

      // ---- base counters: the planes of paths0[row0], its recipe, or its bits streamed ----
      u32 B[M][L];
#pragma unroll
      for (int h = 0; h < M; h++) {
        const u64 r = (u64)row0 * M + h;
        if (a.planes0) {
          load_planes(B[h], a.planes0, (u32)(((u64)kt * (u64)a.rows0 + r) * (u64)a.g0), a.g0);
        } else if (a.rec_slot) {
          const u32 ra = a.rec_row0[row0], rzr = a.rec_rowz[row0], rz = rzr & 0x7fffffffu, rinfo = a.rec_linfo[r];
          const u32 hz = (M == 2 && (rzr >> 31)) ? (u32)(1 - h) : (u32)h;
          u32 ZR[L], S[L];
          load_planes(B[h], a.rec_planes_a, (u32)(((u64)kt * (u64)a.rec_rows_a + (u64)ra * M + h) * (u64)a.rec_ga), a.rec_ga);
          load_planes(ZR, a.rec_planes_z, (u32)(((u64)kt * (u64)a.rec_rows_z + (u64)rz * M + hz) * (u64)a.rec_gz), a.rec_gz);
#pragma unroll
          for (int l = 0; l < L; l++) S[l] = 0u;
          const u32 rlen = linfo_len(rinfo);
          stream(S, (const u32 GCRE_CONSTANT*)(a.rec_slot + r * 8u), 0, 8);
          if (rlen > 8u) stream(S, (const u32 GCRE_CONSTANT*)(a.rec_over + a.rec_lover[r]), 0, (u64)(rlen - 8u));
          u32 cy = 0u, bw = 0u;
#pragma unroll
          for (int l = 0; l < L; l++) {
            const u32 zl = linfo_overlap(rinfo) ? ZR[l] : S[l];   // overlap list: + Z - S; delta list: + S
            const u32 sl_ = linfo_overlap(rinfo) ? S[l] : 0u;
            const u32 s1_ = B[h][l] ^ zl ^ cy;
            cy = maj3(B[h][l], zl, cy);
            B[h][l] = s1_ ^ sl_ ^ bw;
            bw = maj3(~s1_, sl_, bw);
          }
        } else {
#pragma unroll
          for (int l = 0; l < L; l++) B[h][l] = 0u;
          stream(B[h], lidx0, loff0[r], loff0[r + 1]);
        }
      }

      for (u32 t = 0; t < npaths; t++) {
        const u32 q = first + t;
        if (q < a.score_begin || q >= a.score_end) continue;   // the path belongs to another shard
        u32 C[M][L];
#pragma unroll
        for (int h = 0; h < M; h++) {
          const u32 r0 = rdlane(infov[h], t);
          const u32 len = linfo_len(r0);
          const bool overlap = linfo_overlap(r0);
          u32 offs[8], y[8];
#pragma unroll
          for (int j = 0; j < 8; j++) offs[j] = rdlane(lv[h][j], t);
#pragma unroll
          for (int j = 0; j < 8; j++) y[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, offs[j], 0);
          u32 Z[L];
          if (overlap) {
            load_planes(Z, a.planesz, rdlane(zunit[h], t), a.gz);
          } else {
#pragma unroll
            for (int l = 0; l < L; l++) Z[l] = 0u;
          }
          u32 c0, a0, c1, a1, c2, a2, d0, b0;
          csa(c0, a0, y[0], y[1], y[2]);
          csa(c1, a1, y[3], y[4], y[5]);
          csa(c2, a2, a0, a1, y[6]);
          const u32 s0 = a2 ^ y[7], c3 = a2 & y[7];
          csa(d0, b0, c0, c1, c2);
          const u32 s1 = b0 ^ c3, d1 = b0 & c3;
          u32 S[L];
          S[0] = s0; S[1] = s1; S[2] = d0 ^ d1; S[3] = d0 & d1;
#pragma unroll
          for (int l = 4; l < L; l++) S[l] = 0u;
          if (len > 8u) stream(S, (const u32 GCRE_CONSTANT*)(a.dover + rdlane(lovv[h], t)), 0, (u64)(len - 8u));   // long list (rare)
          if (overlap) {   // C = B + Nz - S
            u32 cy = 0u, bw = 0u;
#pragma unroll
            for (int l = 0; l < L; l++) {
              const u32 s1_ = B[h][l] ^ Z[l] ^ cy;
              cy = maj3(B[h][l], Z[l], cy);
              C[h][l] = s1_ ^ S[l] ^ bw;
              bw = maj3(~s1_, S[l], bw);
            }
          } else {         // C = B + S
            u32 cy = 0u;
#pragma unroll
            for (int l = 0; l < L; l++) {
              C[h][l] = B[h][l] ^ S[l] ^ cy;
              cy = maj3(B[h][l], S[l], cy);
            }
          }
        }
        if constexpr (M == 1) {
          finish_m1(C[0], rdlane(ttv[0], t));
        } else {
          finish_m2(C[0], C[M - 1], rdlane(ttv[0], t), rdlane(ttv[M - 1], t));
        }
        if (++counted == kExceedFlushPaths) {   // (wave-uniform)
          counted = 0;
          exc_flush(bins, xa.lds_bins, xa.hist, lane, 64);
        }
      }
    }
  }
  __syncthreads();
  exc_flush(bins, xa.lds_bins, xa.hist, threadIdx.x, 64 * kIeWaves);
}

#define EXC_IE_GEN_(EXPR, PC)                    \
  if (method == 1) {                             \
    if (planes <= 8) { EXPR(1, 8, PC); }         \
    else if (planes <= 12) { EXPR(1, 12, PC); }  \
    else { EXPR(1, 16, PC); }                    \
  } else {                                       \
    if (planes <= 8) { EXPR(2, 8, PC); }         \
    else if (planes <= 12) { EXPR(2, 12, PC); }  \
    else { EXPR(2, 16, PC); }                    \
  }
#define EXC_IE_GEN(EXPR)                         \
  if (perm_counts) { EXC_IE_GEN_(EXPR, true) }   \
  else { EXC_IE_GEN_(EXPR, false) }

}  // namespace

hipError_t launch_exceed_dense(const ExceedArgs& a, int method, const NullConfig& cfg, hipStream_t stream) {
  if (a.npaths <= 0 || a.K <= 0 || a.m <= 0) return hipSuccess;
  if ((int64_t)a.nkt * a.pgroups > 0x7fffffff || a.lds_bins > kExceedLdsBinsDense || (a.lds_bins != 0 && a.lds_bins != a.m))
    return hipErrorInvalidValue;
  if (a.pc && (a.k0 < 0 || (int64_t)a.k0 + a.K > a.pc_stride)) return hipErrorInvalidValue;
  if (method == 1) {
    switch (cfg.R) {
      case 1: return launch_exceed_t<1, 1, 16, 8, 4>(a, stream);
      case 2: return launch_exceed_t<1, 2, 16, 8, 4>(a, stream);
      case 4: return launch_exceed_t<1, 4, 16, 8, 2>(a, stream);
      default: return launch_exceed_t<1, 8, 8, 4, 3>(a, stream);   // (k_null asks for 4 waves and spills 31 registers for them)
    }
  }
  switch (cfg.R) {
    case 1: return launch_exceed_t<2, 1, 16, 8, 4>(a, stream);
    case 2: return launch_exceed_t<2, 2, 16, 8, 2>(a, stream);
    case 4: return launch_exceed_t<2, 4, 8, 8, 2>(a, stream);
    default: return launch_exceed_t<2, 8, 4, 4, 3>(a, stream);
  }
}

hipError_t launch_exceed_observed(const ExceedObsArgs& a, int cus, hipStream_t stream) {
  if (a.count <= 0 || a.m <= 0) return hipSuccess;
  if (a.lds_bins > kExceedLdsBinsIe || (a.lds_bins != 0 && a.lds_bins != a.m)) return hipErrorInvalidValue;
  const i64 want = (a.count + kObsBlock - 1) / kObsBlock;
  const int grid = (int)(want < (i64)cus * kObsBlocksPerCu ? want : (i64)cus * kObsBlocksPerCu);
  trace_launch("k_exceed_observed", want, grid);
  hipLaunchKernelGGL(k_exceed_observed, dim3(grid), dim3(kObsBlock), (size_t)a.lds_bins * 4, stream, a);
  return hipGetLastError();
}

hipError_t launch_exceed_ie(const IeArgs& a, int method, int planes, const uint32_t* pat, unsigned long long* hist, int m,
                            int lds_bins, hipStream_t stream, const ExceedPerm& perm) {
  if (a.seg_end <= a.seg_begin || a.K <= 0 || m <= 0) return hipSuccess;
  if (a.waves_per_xcd < kIeWaves || lds_bins > kExceedLdsBinsIe || (lds_bins != 0 && lds_bins != m)) return hipErrorInvalidValue;
  const bool perm_counts = perm.pc != nullptr;
  if (perm_counts && (perm.k0 < 0 || (int64_t)perm.k0 + a.K > perm.stride)) return hipErrorInvalidValue;
  const ExceedIeArgs xa{a, pat, hist, m, lds_bins, perm.pc, perm.stride, perm.k0};
  const dim3 grid((unsigned)(8 * a.waves_per_xcd / kIeWaves));
  const dim3 block(64 * kIeWaves);
#define EXC_LAUNCH(MM, LL, PP) hipLaunchKernelGGL((k_exceed_ie<MM, LL, PP>), grid, block, (size_t)lds_bins * 4, stream, xa)
  EXC_IE_GEN(EXC_LAUNCH)
#undef EXC_LAUNCH
  return hipGetLastError();
}

int exceed_ie_max_waves_per_cu(int method, int planes, int lds_bins, bool perm_counts) {
  int blocks = 0;
  hipError_t e = hipSuccess;
#define EXC_OCC(MM, LL, PP) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_exceed_ie<MM, LL, PP>, 64 * kIeWaves, (size_t)lds_bins * 4)
  EXC_IE_GEN(EXC_OCC)
#undef EXC_OCC
  if (e != hipSuccess || blocks < 1) blocks = 1;
  return blocks * kIeWaves;
}

}  // namespace gcre

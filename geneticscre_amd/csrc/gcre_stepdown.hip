// gcre_stepdown.hip -- step-down max-T counts of a level's top rows (gcre_exceed_stepdown).
//   * k_stepdown_null    per (top row, permutation): the count work of k_set_null (gcre_sets.hip: one union row per set against
//                        every mask, lanes own 8 permutations, the mask tile through LDS, set words as wave-uniform scalar
//                        loads, the same table look-ups) -- a copy, so that the set kernels' code object does not move -- with
//                        another finish: the row's null value is counted into E[bin][r], bin = the largest sorted threshold it
//                        reaches that lies strictly below the row's own score
//   * k_stepdown_finish  per permutation: walks the bins from the top, cumulating pc (the join's per-permutation counts V,
//                        DESIGN.md §3.8a) and E; the successive maximum of sorted row b reaches its threshold under r exactly
//                        when V[b][r] - E[b][r] >= 1
// The finish of k_stepdown_null is k_exceed_dense's (gcre_exceed.hip) with per-permutation cells only: the value's bit pattern
// against the LOWEST threshold's pattern (one register) and a wave vote -- nothing more in the common case --; the passing
// values are compacted into the wave's LDS queue with their permutation column (ballot + mbcnt) and drained by one loop that
// locates each among the sorted patterns (the same binary search, the same "largest threshold it reaches" rule).  The queue
// is drained once per set, so the set -- and with it the cap of the bin, the last sorted index below the row's f64 tie
// group -- is wave-uniform and rides in a scalar instead of a third queue.  Every global write is a 32-bit vector atomic.
#include "gcre_kernels.h"

namespace gcre {
namespace {

typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;
typedef u32 __attribute__((ext_vector_type(4))) u32x4;

// wave-uniform read-only inputs through the constant address space: scalar loads
#define SD_CONSTANT __attribute__((address_space(4)))
template <typename T>
__device__ __forceinline__ const T SD_CONSTANT* sd_const(const T* p) {
  return (const T SD_CONSTANT*)p;
}

__device__ __forceinline__ u64 sd_diag(u64 t) { return (t * (t + 1)) >> 1; }

constexpr int kSdBlock = 256;               // threads per block
constexpr int kSdR = 8;                     // permutations per lane
constexpr int kSdPT = 64 * kSdR;            // permutations per tile
constexpr int kSdWC = 4;                    // mask dwords per staged chunk
constexpr int kSdFinishBlock = 256;
constexpr int kSdFinishBatch = 8;          // bins whose cells k_stepdown_finish loads before it walks them
static_assert(kSdPT == kSetPermTile, "k_set_null's tile");

// column of the permutation tile that register j of a lane holds (k_set_null's layout)
__device__ __forceinline__ int sd_col(int lane, int j) { return (j >> 2) * 256 + lane * 4 + (j & 3); }

// the bin of a value that reached the lowest threshold: the last of the ascending patterns that is <= v
__device__ __forceinline__ int sd_bin(const u32* pat, int m, u32 v) {
  int lo = 1, hi = m;   // (pat[0] <= v is known) first index whose pattern is above v
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pat[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

}  // namespace

// M method, TPW sets per wave and set tile, OCC waves per SIMD the register allocation must admit
template <int M, int TPW, int OCC>
__global__ __launch_bounds__(kSdBlock, OCC) void k_stepdown_null(const StepdownArgs a) {
  constexpr int R = kSdR, WC = kSdWC, PT = kSdPT;
  constexpr int NW = kSdBlock / 64;
  constexpr int TPB = NW * TPW;
  constexpr int CHUNK = WC * PT;                // dwords per staged mask chunk
  constexpr int VEC = CHUNK / 4 / kSdBlock;     // uint4 per thread per chunk
  static_assert(VEC >= 1 && CHUNK % (4 * kSdBlock) == 0, "staging shape");

  __shared__ __attribute__((aligned(16))) u32 lds[2][CHUNK];
  __shared__ u32 queue_lds[NW][PT];             // a round holds at most 8 values per lane
  __shared__ unsigned short cqueue_lds[NW][PT];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = blockIdx.x % a.nkt;
  const int g = blockIdx.x / a.nkt;

  const u32 SD_CONSTANT* ROWS = sd_const(a.rows);
  const u32 SD_CONSTANT* TOT = sd_const(a.tot);
  const int32_t SD_CONSTANT* CAP = sd_const(a.cap);

  const int nchunks = a.W32p / WC;
  const u32* mask_tile = a.masks + (size_t)kt * PT;   // column offset of this permutation tile

  // ---- mask staging: chunk c = rows [c*WC, c*WC+WC) x PT columns, row-major in LDS ----
  u32x4 stage[VEC];
  u32 voff[VEC];
#pragma unroll
  for (int i = 0; i < VEC; i++) {
    const int e = tid + i * kSdBlock;
    voff[i] = (u32)((e / (PT / 4)) * a.Kpad + (e % (PT / 4)) * 4) * 4u;
  }
  const size_t chunk_bytes = (size_t)WC * a.Kpad * 4;
  auto stage_load = [&](int c) {
    const char* cb = (const char*)mask_tile + (size_t)c * chunk_bytes;
#pragma unroll
    for (int i = 0; i < VEC; i++) stage[i] = *(const u32x4*)(cb + voff[i]);
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < VEC; i++) *(u32x4*)(&lds[buf][(tid + i * kSdBlock) * 4]) = stage[i];
  };

  // permutations K.. of the last tile are padding: they never count
  const int live_cols = a.K - kt * PT;
  const u32 pat0 = a.pat[0];
  const u32 base = (u32)(kt * PT);   // absolute permutation of the tile's column 0
  u32* const queue = queue_lds[wave];
  unsigned short* const cqueue = cqueue_lds[wave];

  // The passing ones of a set's R values per lane (the caller has voted) go into the wave's queue in lane order with their
  // columns, then the wave walks the queue.  Every lane of the wave calls it; cap >= 0 is wave-uniform.  A passing value is
  // a live column: base + col < K <= stride; 0 <= bin <= cap < m.
  auto emit = [&](const u32 (&v)[R], const bool (&pass)[R], int cap) {
    int lane_here = lane;   // (as exc_emit_pc: the columns are made here, not kept in registers across the count loop)
    asm volatile("" : "+v"(lane_here));
    u32 n = 0;
#pragma unroll
    for (int j = 0; j < R; j++) {
      const u64 bal = __ballot(pass[j]);
      const u32 pos = n + __builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u));
      if (pass[j]) {
        queue[pos] = v[j];
        cqueue[pos] = (unsigned short)sd_col(lane_here, j);
      }
      n += (u32)__popcll(bal);
    }
    __builtin_amdgcn_wave_barrier();   // (a wave's LDS accesses are served in order)
    for (u32 i = (u32)lane; i < n; i += 64u) {
      const u32 x = queue[i];
      const u32 r = base + (u32)cqueue[i];
      int bin = sd_bin(a.pat, a.m, x);
      bin = bin < cap ? bin : cap;
      atomicAdd(a.E + ((size_t)bin * a.stride + r), 1u);
    }
    __builtin_amdgcn_wave_barrier();
  };

  stage_load(0);
  stage_store(0);
  __syncthreads();
  int buf = 0;

  const size_t rs = (size_t)M * a.W32p;   // dwords per set: (+) half, then (-) half (method 2)

  for (i64 pt = g; pt < a.npt; pt += a.pgroups) {
    const i64 qbase = pt * TPB + (i64)wave * TPW;
    u32 acc[M][TPW][R];
#pragma unroll
    for (int h = 0; h < M; h++)
#pragma unroll
      for (int t = 0; t < TPW; t++)
#pragma unroll
        for (int j = 0; j < R; j++) acc[h][t][j] = 0u;

    // row offsets of this wave's sets, wave-uniform; a set past the end reads the last set's row (its result is dropped)
    size_t o[TPW];
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const i64 q = qbase + t < a.nsets ? qbase + t : a.nsets - 1;
      o[t] = (size_t)q * rs;
    }

    // software pipeline over the flattened (chunk, set) sequence, as k_set_null
    u32x4 nx[M];
    auto fetch = [&](int c, int t) {
      const u32 SD_CONSTANT* b = ROWS + o[t] + (size_t)c * WC;
      nx[0] = *(const u32x4 SD_CONSTANT*)b;
      if constexpr (M == 2) nx[1] = *(const u32x4 SD_CONSTANT*)(b + a.W32p);
    };
    fetch(0, 0);

    for (int c = 0; c < nchunks; c++) {
      const int cn = (c + 1 == nchunks) ? 0 : c + 1;
      stage_load(cn);   // the next chunk of this block's (periodic) mask stream

      u32 m[WC][R];
#pragma unroll
      for (int w = 0; w < WC; w++) {
        const u32* row = &lds[buf][w * PT];
        const u32x4 v0 = *(const u32x4*)(row + lane * 4);
        const u32x4 v1 = *(const u32x4*)(row + 256 + lane * 4);
        m[w][0] = v0.x; m[w][1] = v0.y; m[w][2] = v0.z; m[w][3] = v0.w;
        m[w][4] = v1.x; m[w][5] = v1.y; m[w][6] = v1.z; m[w][7] = v1.w;
      }

#pragma unroll
      for (int t = 0; t < TPW; t++) {
        u32 jn[M][WC];
#pragma unroll
        for (int h = 0; h < M; h++)
#pragma unroll
          for (int w = 0; w < WC; w++) jn[h][w] = __builtin_amdgcn_readfirstlane(nx[h][w]);
        if (t + 1 < TPW) fetch(c, t + 1);
        else fetch(cn, 0);
#pragma unroll
        for (int h = 0; h < M; h++)
#pragma unroll
          for (int w = 0; w < WC; w++)
#pragma unroll
            for (int j = 0; j < R; j++) acc[h][t][j] += __builtin_popcount(jn[h][w] & m[w][j]);
        __builtin_amdgcn_sched_barrier(0);   // keep each set's scalar loads in its own region
      }

      stage_store(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }

    // ---- null scores on each set's table diagonal, against the lowest threshold; the few that pass are binned ----
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const i64 q = qbase + t;
      if (q >= a.nsets) continue;   // wave-uniform
      const int cap = CAP[q];
      if (cap < 0) continue;        // a best row (nothing is strictly below its tie group's start): it is excluded nowhere
      u32 v[R];
      if constexpr (M == 1) {
        // the sanitised f32 table: non-negative floats, ordered as their bit patterns
        const u32* diag = (const u32*)a.t32 + sd_diag(TOT[q]);
#pragma unroll
        for (int j = 0; j < R; j++) v[j] = diag[acc[0][t][j]];
      } else {
        // vtmax[pp][|P| - pp] + vtmax[|N| - pn][pn] (d64n: d64, or its mirror image where vtmax is not symmetric), folded as
        // k_null folds it
        const double* dp = a.d64 + sd_diag(TOT[2 * q]);
        const double* dn = a.d64n + sd_diag(TOT[2 * q + 1]);
#pragma unroll
        for (int j = 0; j < R; j++) {
          float f = (float)(dp[acc[0][t][j]] + dn[acc[M - 1][t][j]]);
          f = (f > 0.0f) ? f : 0.0f;   // NaN and negatives fold as 0, as into the join's maxima
          v[j] = __float_as_uint(f);
        }
      }
      bool pass[R], any = false;
#pragma unroll
      for (int j = 0; j < R; j++) {
        pass[j] = v[j] >= pat0 && sd_col(lane, j) < live_cols;
        any = any || pass[j];
      }
      if (__ballot(any)) emit(v, pass, cap);
    }
  }
}

// Lane = permutation.  Bin b of the ascending thresholds, from the top: cumV = V[b][r] = joined paths whose null value of r
// reaches threshold b, cumE = E[b][r] = the strictly better top rows among them.  A permutation's cells of pc sum to the
// joined paths counted (< 2^32, gcre_exceed_keep_perm_counts), and E <= m.
__global__ __launch_bounds__(kSdFinishBlock) void k_stepdown_finish(const StepdownFinishArgs a) {
  const int r = blockIdx.x * kSdFinishBlock + threadIdx.x;
  const bool live = r < a.K;
  const size_t col = live ? (size_t)r : 0;   // (a lane past the end reads column 0 and never counts)
  const int lane = threadIdx.x & 63;
  u32 cumV = 0u, cumE = 0u;
  bool bad = false;
  // the walk is serial in the bin; the loads are not: kSdFinishBatch bins' cells are in flight together
  for (int b0 = a.m - 1; b0 >= 0; b0 -= kSdFinishBatch) {
    u32 v[kSdFinishBatch], e[kSdFinishBatch];
#pragma unroll
    for (int i = 0; i < kSdFinishBatch; i++) {
      const int b = b0 - i;   // (wave-uniform)
      v[i] = b >= 0 ? a.pc[(size_t)b * a.stride + col] : 0u;
      e[i] = b >= 0 ? a.E[(size_t)b * a.stride + col] : 0u;
    }
#pragma unroll
    for (int i = 0; i < kSdFinishBatch; i++) {
      const int b = b0 - i;
      if (b < 0) break;
      cumV += v[i];
      cumE += e[i];
      const u64 hit = __ballot(live && cumV > cumE);
      bad = bad || (live && cumE > cumV);
      if (lane == 0 && hit != 0) atomicAdd(a.n_ge + b, (u32)__popcll(hit));
    }
  }
  const u64 anybad = __ballot(bad);
  if (lane == 0 && anybad != 0) atomicAdd(a.bad, (u32)__popcll(anybad));
}

hipError_t launch_stepdown_null(const StepdownArgs& a, int method, hipStream_t stream) {
  if (a.nsets <= 0 || a.K <= 0 || a.m <= 0) return hipSuccess;
  if ((int64_t)a.nkt * a.pgroups > 0x7fffffff || a.W32p % kSdWC != 0 || a.K > a.stride || a.K > a.Kpad ||
      (int64_t)a.nkt * kSdPT < a.K || a.nsets > a.m)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.nkt * a.pgroups));
  if (g_launch_trace)   // a block walks `per` set tiles
    fprintf(stderr, "launch k_stepdown_null npt=%lld pgroups=%d per=%lld\n", (long long)a.npt, a.pgroups,
            (long long)((a.npt + a.pgroups - 1) / a.pgroups));
  if (method == 1) hipLaunchKernelGGL((k_stepdown_null<1, 4, 4>), grid, dim3(kSdBlock), 0, stream, a);
  else hipLaunchKernelGGL((k_stepdown_null<2, 2, 4>), grid, dim3(kSdBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_stepdown_finish(const StepdownFinishArgs& a, hipStream_t stream) {
  if (a.K <= 0 || a.m <= 0) return hipSuccess;
  if (a.K > a.stride) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.K + kSdFinishBlock - 1) / kSdFinishBlock));
  hipLaunchKernelGGL(k_stepdown_finish, grid, dim3(kSdFinishBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

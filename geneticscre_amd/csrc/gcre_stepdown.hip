// gcre_stepdown.hip -- step-down max-T counts of a level's top rows (gcre_exceed_stepdown).
//   * k_stepdown_null    per (top row, permutation): k_set_null's counts and null scores (count_tile and null_scores of
//                        gcre_count_tile.h; row = top row) with another finish: the row's null value is counted into
//                        E[bin][r], bin = the largest sorted threshold it reaches that lies strictly below the row's own score
//   * k_stepdown_finish  per permutation: walks the bins from the top, cumulating pc (the join's per-permutation counts V,
//                        DESIGN.md §3.8a) and E; the successive maximum of sorted row b reaches its threshold under r exactly
//                        when V[b][r] - E[b][r] >= 1
// The finish of k_stepdown_null is k_exceed_dense's (gcre_exceed.hip) with per-permutation cells only: the value's bit pattern
// against the LOWEST threshold's pattern (one register) and a wave vote -- nothing more in the common case --; the passing
// values are compacted into the wave's LDS queue with their permutation column (ballot + mbcnt) and drained by one loop that
// locates each among the sorted patterns (the same binary search, the same "largest threshold it reaches" rule).  The queue
// is drained once per set, so the set -- and with it the cap of the bin, the last sorted index below the row's f64 tie
// group -- is wave-uniform and rides in a scalar instead of a third queue.  Every global write is a 32-bit vector atomic.
#include "gcre_count_tile.h"

namespace gcre {
namespace {

constexpr int kSdFinishBlock = 256;
constexpr int kSdFinishBatch = 8;          // bins whose cells k_stepdown_finish loads before it walks them

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
__global__ __launch_bounds__(kCtBlock, OCC) void k_stepdown_null(const StepdownArgs a) {
  constexpr int R = kCtR, PT = kCtPT, NW = kCtWaves;
  constexpr int TPB = NW * TPW;

  __shared__ __attribute__((aligned(16))) u32 lds[2][kCtChunk];
  __shared__ u32 queue_lds[NW][PT];             // a round holds at most 8 values per lane
  __shared__ unsigned short cqueue_lds[NW][PT];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = blockIdx.x % a.nkt;
  const int g = blockIdx.x / a.nkt;

  const u32 GCRE_CONSTANT* ROWS = as_const(a.rows);
  const u32 GCRE_CONSTANT* TOT = as_const(a.tot);
  const int32_t GCRE_CONSTANT* CAP = as_const(a.cap);

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
        cqueue[pos] = (unsigned short)ct_col(lane_here, j);
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

  MaskStream ms(lds, a.masks + (size_t)kt * PT, a.Kpad);   // column offset of this permutation tile

  const size_t rs = (size_t)M * a.W32p;   // dwords per set: (+) half, then (-) half (method 2)

  for (i64 pt = g; pt < a.npt; pt += a.pgroups) {
    const i64 qbase = pt * TPB + (i64)wave * TPW;
    // row offsets of this wave's sets, wave-uniform; a set past the end reads the last set's row (its result is dropped)
    size_t o[TPW];
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const i64 q = qbase + t < a.nsets ? qbase + t : a.nsets - 1;
      o[t] = (size_t)q * rs;
    }

    const TileCounts<M, TPW> acc = count_tile<M, TPW>(ms, ROWS, o, a.W32p);

    // ---- null scores on each set's table diagonal, against the lowest threshold; the few that pass are binned ----
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const i64 q = qbase + t;
      if (q >= a.nsets) continue;   // wave-uniform
      const int cap = CAP[q];
      if (cap < 0) continue;        // a best row (nothing is strictly below its tie group's start): it is excluded nowhere
      u32 v[R];
      null_scores<M>(a.t32, a.d64, a.d64n, TOT, q, acc.v[0][t], acc.v[M - 1][t], v);
      bool pass[R], any = false;
#pragma unroll
      for (int j = 0; j < R; j++) {
        pass[j] = v[j] >= pat0 && ct_col(lane, j) < live_cols;
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
  if ((int64_t)a.nkt * a.pgroups > 0x7fffffff || a.W32p % kCtWC != 0 || a.K > a.stride || a.K > a.Kpad ||
      (int64_t)a.nkt * kCtPT < a.K || a.nsets > a.m)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.nkt * a.pgroups));
  if (g_launch_trace)   // a block walks `per` set tiles
    fprintf(stderr, "launch k_stepdown_null npt=%lld pgroups=%d per=%lld\n", (long long)a.npt, a.pgroups,
            (long long)((a.npt + a.pgroups - 1) / a.pgroups));
  if (method == 1) hipLaunchKernelGGL((k_stepdown_null<1, 4, 4>), grid, dim3(kCtBlock), 0, stream, a);
  else hipLaunchKernelGGL((k_stepdown_null<2, 2, 4>), grid, dim3(kCtBlock), 0, stream, a);
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

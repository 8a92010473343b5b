// gcre_family.hip -- step-down, k-FWER and FDR over a family of caller-given sets (gcre_score_sets_family).
// All of them are functions of one matrix: N[i][r], the f32 null score of valid set i under permutation r.
//   * k_family_null   per (set, permutation): k_set_null's counts and null scores (count_tile and null_scores of
//                     gcre_count_tile.h; row = set) with another finish: a lane stores its eight values as two 16-byte vector
//                     stores into N[row][perm], row = the set's rank in ascending observed order
//   * k_family_scan   lane = permutation: walks the rows in that order with a running maximum; at the end of each tie group
//                     the lanes whose maximum reaches the group's threshold are counted (a ballot; the counts of 64 rows
//                     leave a wave as one atomic instruction); in the same walk a sorted insertion keeps the column's
//                     kFamilyKmax largest values
//   * k_family_hist   every live value is located among the ascending distinct threshold patterns (sd_bin's rule: the largest
//                     threshold it reaches) and counted into a block's LDS histogram of kFamilyHistBins bins, flushed with
//                     64-bit atomics; a family with more thresholds is walked in passes over ranges of bins (blockIdx.y)
// N is kept for a slab of whole 512-permutation tiles at a time; its row stride is the slab's permutation count.  Padded
// columns (permutations >= K) hold whatever the padded masks give: k_family_scan and k_family_hist never count them.
// Every global write is a plain vector store or a vector atomic.
#include "gcre_count_tile.h"

namespace gcre {
namespace {

constexpr int kFamScanBlock = 64;            // one wave per block: K / 64 waves is all the scan has, spread over the CUs
constexpr int kFamScanBatch = 32;            // rows whose loads k_family_scan has in flight before it walks them
constexpr int kFamHistBlock = 256;
constexpr int kFamHistRound = 1 << 20;       // vectors per thread between two flushes; with the row that follows, at most
                                             // 2^21: a block counts at most 2^31 values into its LDS counters
}  // namespace

// M method, TPW sets per wave and set tile, OCC waves per SIMD the register allocation must admit
template <int M, int TPW, int OCC>
__global__ __launch_bounds__(kCtBlock, OCC) void k_family_null(const FamilyNullArgs a) {
  constexpr int R = kCtR, PT = kCtPT;
  constexpr int TPB = kCtWaves * TPW;

  __shared__ __attribute__((aligned(16))) u32 lds[2][kCtChunk];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = blockIdx.x % a.nkt;            // tile of the slab
  const int g = blockIdx.x / a.nkt;

  const u32 GCRE_CONSTANT* ROWS = as_const(a.rows);
  const u32 GCRE_CONSTANT* TOT = as_const(a.tot);
  const u32 GCRE_CONSTANT* RANK = as_const(a.rank);

  MaskStream ms(lds, a.masks + (size_t)(a.kt0 + kt) * PT, a.Kpad);   // column offset of this permutation tile

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

    // ---- null scores on each set's table diagonal, stored as they are: registers 0..3 are columns 4 lane .. 4 lane + 3 of
    // the tile, registers 4..7 the same columns of its second half (ct_col) ----
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const i64 q = qbase + t;
      if (q >= a.nsets) continue;   // wave-uniform
      u32 v[R];
      null_scores<M>(a.t32, a.d64, a.d64n, TOT, q, acc.v[0][t], acc.v[M - 1][t], v);
      // rank < nsets and (kt + 1) * PT <= stride: inside N [nsets][stride]
      u32* dst = a.N + ((size_t)RANK[q] * (size_t)a.stride + (size_t)kt * PT + (size_t)lane * 4);
      u32x4 lo, hi;
      lo.x = v[0]; lo.y = v[1]; lo.z = v[2]; lo.w = v[3];
      hi.x = v[4]; hi.y = v[5]; hi.z = v[6]; hi.w = v[7];
      *(u32x4*)dst = lo;
      *(u32x4*)(dst + 256) = hi;
    }
  }
}

// Lane = column of the slab.  meta[row] = the row's f32 threshold pattern (at most 0x7f800001: bit 31 is free), bit 31 set
// on the last row of a tie group; zeros behind the last row, up to a multiple of 64.  A group's rows share one threshold
// (they tie as doubles), so the group's count is one ballot at its last row; the host hands it to the group's other rows.
// The counts of 64 consecutive rows wait in the wave's lanes, lane l that of row r0 + l, and leave as one atomic instruction
// on 64 consecutive words.  The walk is serial in the row; the loads are not: kFamScanBatch rows' cells and thresholds are in
// flight together.  top[] and the batch are indexed by unrolled loops only: registers.
__global__ __launch_bounds__(kFamScanBlock) void k_family_scan(const FamilyScanArgs a) {
  constexpr int KM = kFamilyKmax, B = kFamScanBatch;
  static_assert(64 % B == 0, "whole batches per 64 rows");
  const int col = blockIdx.x * kFamScanBlock + threadIdx.x;
  const bool live = col < a.live;
  const size_t c = live ? (size_t)col : 0;   // (a lane past the end reads column 0 and never counts or stores)
  const int lane = threadIdx.x & 63;
  const u32 GCRE_CONSTANT* META = as_const(a.meta);
  u32 run = 0u;
  u32 top[KM];
#pragma unroll
  for (int k = 0; k < KM; k++) top[k] = 0u;
  for (i64 r0 = 0; r0 < a.nsets; r0 += 64) {
    u32 mine = 0u;   // the count of row r0 + lane, 0 unless that row ends a group
#pragma unroll
    for (int h = 0; h < 64 / B; h++) {
      const i64 rb = r0 + h * B;   // (wave-uniform)
      if (rb < a.nsets) {
        u32 v[B], mt[B];
#pragma unroll
        for (int i = 0; i < B; i++) v[i] = rb + i < a.nsets ? a.N[(size_t)(rb + i) * (size_t)a.stride + c] : 0u;
#pragma unroll
        for (int i = 0; i < B; i++) mt[i] = META[rb + i];   // (padded: a row past the end is a 0 that ends no group)
#pragma unroll
        for (int i = 0; i < B; i++) {
          u32 x = v[i];   // (a row past the end is a 0 that changes nothing)
          run = x > run ? x : run;
          if (a.kmax && __ballot(x > top[KM - 1])) {
            // sorted insertion, descending: x sinks to its place, every smaller value moves down one
#pragma unroll
            for (int k = 0; k < KM; k++) {
              const u32 hi = x > top[k] ? x : top[k];
              x = x > top[k] ? top[k] : x;
              top[k] = hi;
            }
          }
          const u64 hit = __ballot(live && (mt[i] >> 31) != 0u && run >= (mt[i] & 0x7fffffffu));
          if (lane == h * B + i) mine = (u32)__popcll(hit);
        }
      }
    }
    if (mine != 0u) atomicAdd(a.n_ge + r0 + lane, mine);   // (mine != 0: a real row)
  }
  if (a.kmax && live) {
#pragma unroll
    for (int k = 0; k < KM; k++) a.kmax[(size_t)k * (size_t)a.kstride + (size_t)a.k0 + c] = top[k];
  }
}

// A block walks whole rows, a thread reads 16 bytes at a time.  Pass p = blockIdx.y owns the bins [p * kFamilyHistBins, ...):
// its patterns are staged in LDS and searched there; a value below the pass's first pattern, or at or above the next pass's
// first one, is dropped after one compare each.  A block's LDS counters are flushed before they can overflow.
__global__ __launch_bounds__(kFamHistBlock) void k_family_hist(const FamilyHistArgs a) {
  constexpr int NB = kFamilyHistBins;
  __shared__ u32 pat[NB];
  __shared__ u32 cnt[NB];
  const int tid = threadIdx.x;
  const int b0 = blockIdx.y * NB;
  const int nb = a.m - b0 < NB ? a.m - b0 : NB;               // bins of this pass, >= 1
  const u32 above = b0 + nb < a.m ? a.pat[b0 + nb] : 0xffffffffu;   // the next pass's first pattern (no value reaches ~0)
  for (int i = tid; i < nb; i += kFamHistBlock) pat[i] = a.pat[b0 + i];
  for (int i = tid; i < NB; i += kFamHistBlock) cnt[i] = 0u;
  __syncthreads();
  const u32 first = pat[0];
  auto flush = [&]() {   // every thread of the block calls it
    __syncthreads();
    for (int i = tid; i < nb; i += kFamHistBlock) {
      const u32 n = cnt[i];
      if (n != 0u) atomicAdd(a.hist + b0 + i, (unsigned long long)n);
      cnt[i] = 0u;
    }
    __syncthreads();
  };
  // a block takes whole rows; a row costs a thread `per_row` vectors (block-uniform), at most 2^21: live < 2^31
  const int live4 = (a.live + 3) / 4;            // vectors of a row with a live column
  const int per_row = (live4 + kFamHistBlock - 1) / kFamHistBlock;
  int done = 0;                                  // vectors per thread since the last flush
  for (i64 row = blockIdx.x; row < a.nsets; row += gridDim.x) {
    if (done + per_row > kFamHistRound && done > 0) {
      flush();
      done = 0;
    }
    done += per_row;
    const u32* nrow = a.N + (size_t)row * (size_t)a.stride;
    for (int v4 = tid; v4 < live4; v4 += kFamHistBlock) {
      const int c4 = v4 * 4;                     // c4 + 3 < stride: stride is a multiple of 4 and >= live
      const u32x4 q = *(const u32x4*)(nrow + c4);
      const u32 x[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (c4 + k >= a.live || x[k] < first || x[k] >= above) continue;   // a padded column, or another pass's value
        int lo = 1, hi = nb;   // (pat[0] <= x is known) first index whose pattern is above x
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (pat[mid] <= x[k]) lo = mid + 1;
          else hi = mid;
        }
        atomicAdd(&cnt[lo - 1], 1u);
      }
    }
  }
  flush();
}

hipError_t launch_family_null(const FamilyNullArgs& a, int method, hipStream_t stream) {
  if (a.nsets <= 0 || a.nkt <= 0) return hipSuccess;
  if ((int64_t)a.nkt * a.pgroups > 0x7fffffff || a.pgroups < 1 || a.W32p % kCtWC != 0 || a.kt0 < 0 ||
      (int64_t)(a.kt0 + a.nkt) * kCtPT > a.Kpad || a.stride != (int64_t)a.nkt * kCtPT)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.nkt * a.pgroups));
  if (g_launch_trace)   // a block walks `per` set tiles
    fprintf(stderr, "launch k_family_null npt=%lld pgroups=%d per=%lld\n", (long long)a.npt, a.pgroups,
            (long long)((a.npt + a.pgroups - 1) / a.pgroups));
  if (method == 1) hipLaunchKernelGGL((k_family_null<1, 4, 4>), grid, dim3(kCtBlock), 0, stream, a);
  else hipLaunchKernelGGL((k_family_null<2, 2, 4>), grid, dim3(kCtBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_family_scan(const FamilyScanArgs& a, hipStream_t stream) {
  if (a.nsets <= 0 || a.live <= 0) return hipSuccess;
  if (a.live > a.stride || (a.kmax && a.k0 + a.live > a.kstride)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.live + kFamScanBlock - 1) / kFamScanBlock));
  hipLaunchKernelGGL(k_family_scan, grid, dim3(kFamScanBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_family_hist(const FamilyHistArgs& a, int cus, hipStream_t stream) {
  if (a.nsets <= 0 || a.live <= 0 || a.m <= 0) return hipSuccess;
  if (a.live > a.stride || a.stride % 4 != 0) return hipErrorInvalidValue;
  const int64_t passes = ((int64_t)a.m + kFamilyHistBins - 1) / kFamilyHistBins;
  if (passes > 65535) return hipErrorInvalidValue;
  // whole rows per block, a few blocks per CU at the most: the flush of a block is up to kFamilyHistBins atomics
  const int64_t blocks = std::min<int64_t>(a.nsets, (int64_t)std::max(cus, 1) * 8);
  const dim3 grid((unsigned)blocks, (unsigned)passes);
  hipLaunchKernelGGL(k_family_hist, grid, dim3(kFamHistBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

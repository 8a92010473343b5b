// gcre_minp.hip -- Westfall-Young min-P over a family of caller-given sets (gcre_score_sets_minp).
// Everything is a function of N[i][r], the f32 null score of valid set i under permutation r (k_family_null, gcre_family.hip),
// taken row by row: R[i][r] = #{r' < K : N[i][r'] >= N[i][r]}, K times the nominal p-value permutation r's data would have
// got for set i from the set's own null distribution.
//   * k_minp_gather   copies the union rows and carrier totals the set stage left on the device into the walk order (NaN
//                     scores first, then the count c descending), so that a slab of the walk is a contiguous run of rows
//   * k_minp_rank     one block per row of N.  The row is taken in chunks of kMinpChunk values; a chunk is sorted in LDS
//                     (bitonic: strides of 16 and more through LDS, the strides below inside a thread's 16 registers), then
//                     every live value of the row searches the sorted chunk and adds "values >= mine" to its cell of R.  The
//                     padding of the last chunk is 0xffffffff: above every score, so it sorts behind the live values and the
//                     count "live values of the chunk - values below mine" never sees it.  Padded columns of R get
//                     0xffffffff.  Counts are integers: exact, whatever the chunking.
//   * k_minp_scan     lane = permutation: walks the slab's rows of R with a running minimum that is loaded at the start of
//                     the slab and stored at its end; at the last row of a tie group the lanes whose minimum is <= the
//                     group's c are counted (a ballot; the counts of 64 rows leave a wave as one atomic instruction)
// Every global write is a plain vector store or a vector atomic.
#include "gcre_count_tile.h"   // GCRE_CONSTANT

namespace gcre {
namespace {

constexpr int kRankBlock = 1024;                  // 16 waves sort one chunk: 16 values per thread
constexpr int kRankE = kMinpChunk / kRankBlock;   // values of a chunk per thread: the strides below it stay in registers
constexpr int kRankU = 4;                         // searches a thread has in flight
constexpr int kScanBlock = 64;                    // one wave per block, as k_family_scan
constexpr int kScanBatch = 32;                    // rows in flight before the walk
constexpr int kGatherBlock = 256;
static_assert(kRankE == 16, "the register stages are written for 16 values per thread");
static_assert((kMinpChunk & (kMinpChunk - 1)) == 0, "a bitonic network");

// ascending order where `asc`, descending where not
__device__ __forceinline__ void cswap(u32& x, u32& y, bool asc) {
  const u32 lo = x < y ? x : y, hi = x < y ? y : x;
  x = asc ? lo : hi;
  y = asc ? hi : lo;
}

// the strides 8, 4, 2, 1 of one merge on a thread's 16 consecutive values
__device__ __forceinline__ void merge16(u32 (&v)[kRankE], bool asc) {
#pragma unroll
  for (int j = kRankE / 2; j >= 1; j >>= 1)
#pragma unroll
    for (int e = 0; e < kRankE; e++)
      if ((e & j) == 0) cswap(v[e], v[e + j], asc);
}

}  // namespace

__global__ __launch_bounds__(kGatherBlock) void k_minp_gather(const MinpGatherArgs a) {
  const i64 i = (i64)blockIdx.x * kGatherBlock + threadIdx.x;
  if (i < a.nsets * a.rw) {
    const i64 row = i / a.rw, w = i % a.rw;
    a.rows_out[i] = a.rows[(size_t)a.order[row] * (size_t)a.rw + (size_t)w];   // order[row] < nsets
  }
  if (i < a.nsets * a.m) {
    const i64 row = i / a.m, h = i % a.m;
    a.tot_out[i] = a.tot[(size_t)a.order[row] * (size_t)a.m + (size_t)h];
  }
}

__global__ __launch_bounds__(kRankBlock) void k_minp_rank(const MinpRankArgs a) {
  constexpr int C = kMinpChunk, T = kRankBlock, E = kRankE, U = kRankU;
  __shared__ __attribute__((aligned(16))) u32 s[C];
  const int tid = threadIdx.x;
  const u32* nrow = a.N + (size_t)blockIdx.x * (size_t)a.stride;   // blockIdx.x < nsets
  u32* rrow = a.R + (size_t)blockIdx.x * (size_t)a.stride;
  const int stride = (int)a.stride;                                // < 2^31: a multiple of 512 at or above K

  for (int c0 = 0; c0 < a.K; c0 += C) {
    const int nl = a.K - c0 < C ? a.K - c0 : C;   // live values of this chunk
    // ---- a thread's 16 consecutive values; whole vectors lie inside the row (stride % 16 == 0) or behind it ----
    u32 v[E];
    const int base = tid * E;
    if (c0 + base < stride) {
#pragma unroll
      for (int q = 0; q < E / 4; q++) {
        const u32x4 x = *(const u32x4*)(nrow + c0 + base + q * 4);
        v[q * 4 + 0] = x.x; v[q * 4 + 1] = x.y; v[q * 4 + 2] = x.z; v[q * 4 + 3] = x.w;
      }
    }
#pragma unroll
    for (int e = 0; e < E; e++)
      if (base + e >= nl) v[e] = 0xffffffffu;     // the padding: above every score
    // ---- merges of 2, 4, 8 and 16 in registers ----
#pragma unroll
    for (int k = 2; k <= E; k <<= 1)
#pragma unroll
      for (int j = k >> 1; j >= 1; j >>= 1)
#pragma unroll
        for (int e = 0; e < E; e++)
          if ((e & j) == 0) cswap(v[e], v[e + j], ((base + e) & k) == 0);
#pragma unroll
    for (int q = 0; q < E / 4; q++) {
      u32x4 x;
      x.x = v[q * 4 + 0]; x.y = v[q * 4 + 1]; x.z = v[q * 4 + 2]; x.w = v[q * 4 + 3];
      *(u32x4*)(&s[base + q * 4]) = x;
    }
    __syncthreads();
    // ---- merges of 32 .. C: the strides >= 16 through LDS, then 8 .. 1 in registers ----
    for (int k = 2 * E; k <= C; k <<= 1) {
      for (int j = k >> 1; j >= E; j >>= 1) {
#pragma unroll
        for (int p = 0; p < E / 2; p++) {
          const int t = tid + p * T;                              // pair of the stage, 0 .. C/2 - 1
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));    // i + j < C
          u32 x = s[i], y = s[i + j];
          cswap(x, y, (i & k) == 0);
          s[i] = x;
          s[i + j] = y;
        }
        __syncthreads();
      }
#pragma unroll
      for (int q = 0; q < E / 4; q++) {
        const u32x4 x = *(const u32x4*)(&s[base + q * 4]);
        v[q * 4 + 0] = x.x; v[q * 4 + 1] = x.y; v[q * 4 + 2] = x.z; v[q * 4 + 3] = x.w;
      }
      merge16(v, (base & k) == 0);
#pragma unroll
      for (int q = 0; q < E / 4; q++) {
        u32x4 x;
        x.x = v[q * 4 + 0]; x.y = v[q * 4 + 1]; x.z = v[q * 4 + 2]; x.w = v[q * 4 + 3];
        *(u32x4*)(&s[base + q * 4]) = x;
      }
      __syncthreads();
    }
    // ---- every column of the row against the sorted chunk: U searches in flight per thread ----
    for (int col0 = tid; col0 < stride; col0 += T * U) {
      u32 x[U];
      int pos[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int col = col0 + u * T;
        x[u] = col < a.K ? nrow[col] : 0u;   // col < stride where it is read
        pos[u] = 0;
      }
      // values below x: s[0 .. pos) are, after the last step also decided for s[pos]
#pragma unroll 1
      for (int step = C >> 1; step >= 1; step >>= 1) {
#pragma unroll
        for (int u = 0; u < U; u++)
          if (s[pos[u] + step - 1] < x[u]) pos[u] += step;       // pos + step - 1 <= C - 2
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int col = col0 + u * T;
        if (col >= stride) continue;
        if (col >= a.K) {
          if (c0 == 0) rrow[col] = 0xffffffffu;                  // a padded column
          continue;
        }
        if (s[pos[u]] < x[u]) pos[u]++;                          // pos <= C - 1; x is live, so pos <= nl afterwards
        const u32 ge = (u32)(nl - pos[u]);
        rrow[col] = c0 == 0 ? ge : rrow[col] + ge;
      }
    }
    __syncthreads();   // the next chunk overwrites s
  }
}

// meta[row] = the row's count c (< 2^31), bit 31 set on the last row of a tie group that is counted (a NaN score ends none).
__global__ __launch_bounds__(kScanBlock) void k_minp_scan(const MinpScanArgs a) {
  constexpr int B = kScanBatch;
  static_assert(64 % B == 0, "whole batches per 64 rows");
  const int col = blockIdx.x * kScanBlock + threadIdx.x;
  const bool live = col < a.K;
  const size_t c = live ? (size_t)col : 0;   // (a lane past the end reads column 0 and never counts or stores)
  const int lane = threadIdx.x & 63;
  const u32 GCRE_CONSTANT* META = (const u32 GCRE_CONSTANT*)a.meta;
  u32 run = a.q[c];
  for (i64 r0 = 0; r0 < a.nsets; r0 += 64) {
    u32 mine = 0u;   // the count of row r0 + lane, 0 unless that row ends a group
#pragma unroll
    for (int h = 0; h < 64 / B; h++) {
      const i64 rb = r0 + h * B;   // (wave-uniform)
      if (rb < a.nsets) {
        u32 v[B], mt[B];
#pragma unroll
        for (int i = 0; i < B; i++) v[i] = rb + i < a.nsets ? a.R[(size_t)(rb + i) * (size_t)a.stride + c] : 0xffffffffu;
#pragma unroll
        for (int i = 0; i < B; i++) mt[i] = rb + i < a.nsets ? META[rb + i] : 0u;   // (a row past the slab ends no group)
#pragma unroll
        for (int i = 0; i < B; i++) {
          run = v[i] < run ? v[i] : run;
          const u64 hit = __ballot(live && (mt[i] >> 31) != 0u && run <= (mt[i] & 0x7fffffffu));
          if (lane == h * B + i) mine = (u32)__popcll(hit);
        }
      }
    }
    if (mine != 0u) atomicAdd(a.n_le + r0 + lane, mine);   // (mine != 0: a real row of the slab)
  }
  if (live) a.q[c] = run;
}

hipError_t launch_minp_gather(const MinpGatherArgs& a, hipStream_t stream) {
  if (a.nsets <= 0) return hipSuccess;
  if (a.rw < 1 || a.m < 1 || a.m > a.rw) return hipErrorInvalidValue;
  const int64_t blocks = (a.nsets * a.rw + kGatherBlock - 1) / kGatherBlock;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_minp_gather, dim3((unsigned)blocks), dim3(kGatherBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_minp_rank(const MinpRankArgs& a, hipStream_t stream) {
  if (a.nsets <= 0 || a.K <= 0) return hipSuccess;
  if (a.nsets > 0x7fffffff || a.stride > 0x7fffffff - kRankBlock * kRankU || a.stride % 16 != 0 || a.K > a.stride)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_minp_rank, dim3((unsigned)a.nsets), dim3(kRankBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_minp_scan(const MinpScanArgs& a, hipStream_t stream) {
  if (a.nsets <= 0 || a.K <= 0) return hipSuccess;
  if (a.K > a.stride) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.K + kScanBlock - 1) / kScanBlock));
  hipLaunchKernelGGL(k_minp_scan, grid, dim3(kScanBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

// gcre_sequential.hip -- sequential permutation p-values of caller-given sets (gcre_score_sets_sequential):
// every set is permuted until its null score has reached its observed score h times, in batches of permutations that are
// never resident as a whole.
//   * k_seq_masks   the masks of permutations [r0, r0 + nb) by the rule of gcre_sequential.h (k_generate_masks' rule, caller
//                   strata, a 64-bit permutation index), one permutation per lane, in k_set_null's mask layout
//                   [W32p][stride] (permutation-minor; padding rows and padding columns zero)
//   * k_seq_null    count_tile (gcre_count_tile.h) over the sets of an active list; the finish compares every null
//                   score with the set's threshold and writes one ballot word per (active slot, 64 consecutive permutations)
//   * k_seq_retire  one wave per active slot: the slot's exceedances in the batch, by a wave prefix sum over the words of its
//                   bit row; a set whose h-th exceedance lies in the batch gets its position and leaves, the others go on
//                   the next active list
// Row = the set of an active slot; the mask rows have stride `stride`, not Kpad.  Every global write is a vector store or a
// vector atomic.  The context-side entry is in gcre_host_sequential.hip.
#include "gcre_count_tile.h"
#include "gcre_sequential.h"

namespace gcre {
namespace {

constexpr int kSeqTW = kCtPT / 64;           // ballot words per tile
constexpr int kSeqRetireBlock = 256;         // threads per block of k_seq_retire: one wave per active slot
static_assert(kCtPT == gcre_sequential::kSeqTile, "tile");

}  // namespace

// One permutation per lane.  Patients are walked in order; the stratum of a patient is wave-uniform (a scalar load), so with
// up to NS strata need / rem stay in registers and the stratum picks them by a uniform branch; NS == 0: any number of strata,
// need / rem of a column in `work`, stratum-major, so that a wave reads and writes 256 contiguous bytes.  A finished dword goes
// to row c >> 5 of the permutation's column: 256 contiguous bytes a wave.  Columns at and beyond nb (up to stride) are zero.
template <int NS>
__global__ __launch_bounds__(64) void k_seq_masks(const SeqMaskArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.stride) return;
  const size_t S = (size_t)a.stride;
  const int n = a.n;
  const int words = (n + 31) >> 5;            // <= W32p (launch_seq_masks)
  if (r >= a.nb) {
    for (int k = 0; k < a.W32p; k++) a.masks[(size_t)k * S + r] = 0u;
    return;
  }
  const int32_t GCRE_CONSTANT* STR = as_const(a.stratum);
  const u32 GCRE_CONSTANT* CASES = as_const(a.cases_in);
  const u32 GCRE_CONSTANT* SIZE = as_const(a.size_of);
  const u64 base = gcre_sequential::seq_base(a.seed, a.r0 + (u64)r);
  u32 word = 0;
  if constexpr (NS > 0) {
    u32 need[NS], rem[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) {
      need[k] = k < a.n_strata ? CASES[k] : 0u;
      rem[k] = k < a.n_strata ? SIZE[k] : 0u;
    }
    for (int c = 0; c < n; c++) {
      const int s = (NS > 1 && a.stratum) ? STR[c] : 0;   // wave-uniform
      bool take = false;
#pragma unroll
      for (int k = 0; k < NS; k++)
        if (s == k) take = gcre_sequential::seq_step(base, (u32)c, rem[k], need[k]);
      if (take) word |= 1u << (c & 31);
      if ((c & 31) == 31 || c == n - 1) {
        a.masks[(size_t)(c >> 5) * S + r] = word;
        word = 0;
      }
    }
  } else {
    u32* need = a.work + r;
    u32* rem = a.work + (size_t)a.n_strata * S + r;
    for (int k = 0; k < a.n_strata; k++) {
      need[(size_t)k * S] = CASES[k];
      rem[(size_t)k * S] = SIZE[k];
    }
    for (int c = 0; c < n; c++) {
      const size_t s = (size_t)(a.stratum ? STR[c] : 0) * S;
      u32 nd = need[s], rm = rem[s];
      if (gcre_sequential::seq_step(base, (u32)c, rm, nd)) word |= 1u << (c & 31);
      need[s] = nd;
      rem[s] = rm;
      if ((c & 31) == 31 || c == n - 1) {
        a.masks[(size_t)(c >> 5) * S + r] = word;
        word = 0;
      }
    }
  }
  for (int k = words; k < a.W32p; k++) a.masks[(size_t)k * S + r] = 0u;
}

// M method, TPW sets per wave and set tile, OCC waves per SIMD the register allocation must admit
template <int M, int TPW, int OCC>
__global__ __launch_bounds__(kCtBlock, OCC) void k_seq_null(const SeqNullArgs a) {
  constexpr int R = kCtR, PT = kCtPT;
  constexpr int TPB = kCtWaves * TPW;

  __shared__ __attribute__((aligned(16))) u32 lds[2][kCtChunk];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = blockIdx.x % a.nkt;
  const int g = blockIdx.x / a.nkt;

  const u32 GCRE_CONSTANT* ROWS = as_const(a.rows);
  const u32 GCRE_CONSTANT* TOT = as_const(a.tot);
  const u32 GCRE_CONSTANT* THR = as_const(a.thr);
  const u32 GCRE_CONSTANT* ACT = as_const(a.active);

  // whether the permutation of each register is one of the batch (the padding of the last tile never counts)
  bool live[R];
#pragma unroll
  for (int j = 0; j < R; j++) live[j] = kt * PT + ct_col(lane, j) < a.K;

  MaskStream ms(lds, a.masks + (size_t)kt * PT, a.stride);   // column offset of this permutation tile

  const size_t rs = (size_t)M * a.W32p;   // dwords per set: (+) half, then (-) half (method 2)

  for (i64 pt = g; pt < a.npt; pt += a.pgroups) {
    const i64 sbase = pt * TPB + (i64)wave * TPW;   // the wave's first slot of the active list
    // the sets of this wave's slots and their row offsets, wave-uniform; a slot past the end reads the last slot's set (its
    // result is dropped)
    size_t o[TPW];
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const i64 sl = sbase + t < a.nactive ? sbase + t : a.nactive - 1;
      o[t] = (size_t)ACT[sl] * rs;
    }

    const TileCounts<M, TPW> acc = count_tile<M, TPW>(ms, ROWS, o, a.W32p);

    // ---- null scores on each set's table diagonal (null_scores); the compares by ballot; the tile's eight words ----
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      if (sbase + t >= a.nactive) continue;   // wave-uniform
      const i64 q = (i64)ACT[sbase + t];   // (read again: nothing of it is kept across the count loop)
      const u32 thr = THR[q];
      u32 v[R];
      null_scores<M>(a.t32, a.d64, a.d64n, TOT, q, acc.v[0][t], acc.v[M - 1][t], v);
      // Column 64 w + i of the tile is register (w >> 2) * 4 + (i & 3) of lane (w & 3) * 16 + (i >> 2): lane i looks its bit
      // of word w up in that register's ballot, and the ballot of these bits is word w in permutation order.
      u64 mine = 0;
#pragma unroll
      for (int j0 = 0; j0 < R; j0 += 4) {
        u64 ball[4];
#pragma unroll
        for (int j = 0; j < 4; j++) ball[j] = __ballot(live[j0 + j] && v[j0 + j] >= thr);
        const u64 lo = (lane & 1) ? ball[1] : ball[0], hi = (lane & 1) ? ball[3] : ball[2];
        const u64 sel = (lane & 2) ? hi : lo;
#pragma unroll
        for (int w = 0; w < 4; w++) {
          const u64 word = __ballot(((sel >> (w * 16 + (lane >> 2))) & 1ull) != 0ull);
          if (lane == j0 + w) mine = word;
        }
      }
      const size_t wstride = (size_t)a.stride / 64;   // words per slot of the bit rows
      if (lane < kSeqTW) a.bits[(size_t)(sbase + t) * wstride + (size_t)kt * kSeqTW + lane] = mine;
    }
  }
}

// One wave per active slot.  The words of the slot's bit row are walked 64 at a time: a lane's popcount, the wave's inclusive
// prefix sum, and where the running count first reaches h the lane that holds the crossing word selects the bit.  A block
// reserves the places of its surviving slots with one atomic.
__global__ __launch_bounds__(kSeqRetireBlock) void k_seq_retire(const SeqRetireArgs a) {
  constexpr int NW = kSeqRetireBlock / 64;
  __shared__ u32 keep[NW];
  __shared__ u32 base_s;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const i64 slot = (i64)blockIdx.x * NW + wave;
  const u32 GCRE_CONSTANT* ACT = as_const(a.active);
  bool survive = false;
  u32 q = 0;
  if (slot < a.nactive) {   // wave-uniform
    q = ACT[slot];
    const unsigned long long* w = a.bits + (size_t)slot * (size_t)a.wstride;
    u64 running = a.prior[q];   // < h
    bool found = false;
    for (int kb = 0; kb < a.nw; kb += 64) {
      const u64 word = kb + lane < a.nw ? w[kb + lane] : 0ull;
      const u32 c = (u32)__popcll(word);
      u32 incl = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const u32 up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
      }
      const u32 total = __shfl(incl, 63);
      if (running + total >= (u64)a.h) {
        const u32 target = (u32)((u64)a.h - running);   // >= 1: which exceedance of these 64 words
        const int L = (int)__builtin_ctzll(__ballot(incl >= target));
        if (lane == L) {
          const i64 pos = (i64)(kb + lane) * 64 + gcre_sequential::seq_select64(word, (int)(target - (incl - c) - 1u));
          a.n_perm[q] = (long long)(a.r0 + (u64)pos + 1ull);
        }
        found = true;
        break;
      }
      running += total;
    }
    if (!found) {
      if (lane == 0) a.prior[q] = (u32)running;
      survive = true;
    }
  }
  if (lane == 0) keep[wave] = survive ? 1u : 0u;
  __syncthreads();
  if (tid == 0) {
    u32 n = 0;
#pragma unroll
    for (int k = 0; k < NW; k++) n += keep[k];
    base_s = n ? atomicAdd(a.n_next, n) : 0u;
  }
  __syncthreads();
  if (survive && lane == 0) {
    u32 rank = 0;
    for (int k = 0; k < wave; k++) rank += keep[k];
    a.next[(size_t)base_s + rank] = q;
  }
}

hipError_t launch_seq_masks(const SeqMaskArgs& a, hipStream_t stream) {
  if (a.stride == 0) return hipSuccess;
  if (a.stride % 64 != 0 || a.nb < 0 || a.nb > a.stride || a.n < 1 || (a.n + 31) / 32 > a.W32p || a.n_strata < 1 || !a.cases_in ||
      !a.size_of || !a.masks || (a.n_strata > 1 && !a.stratum) || (a.n_strata > kSeqRegStrata && !a.work))
    return hipErrorInvalidValue;
  if (g_launch_trace) fprintf(stderr, "launch k_seq_masks perms=%d of %d strata=%d\n", a.nb, a.stride, a.n_strata);
  const dim3 grid((unsigned)(a.stride / 64)), block(64);
  if (a.n_strata == 1) hipLaunchKernelGGL((k_seq_masks<1>), grid, block, 0, stream, a);
  else if (a.n_strata <= kSeqRegStrata) hipLaunchKernelGGL((k_seq_masks<kSeqRegStrata>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((k_seq_masks<0>), grid, block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_seq_null(const SeqNullArgs& a, int method, hipStream_t stream) {
  if (a.nactive == 0 || a.K == 0) return hipSuccess;
  if ((int64_t)a.nkt * a.pgroups > 0x7fffffff || a.nkt < 1 || a.pgroups < 1 || a.W32p % kCtWC != 0 || a.W32p < kCtWC ||
      a.stride % kCtPT != 0 || (int64_t)a.nkt * kCtPT > a.stride || a.K > a.nkt * kCtPT || (int64_t)a.W32p * a.stride > 0x40000000 ||
      !a.active || !a.bits)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.nkt * a.pgroups));
  if (g_launch_trace)
    fprintf(stderr, "launch k_seq_null active=%lld npt=%lld pgroups=%d perms=%d\n", (long long)a.nactive, (long long)a.npt, a.pgroups, a.K);
  if (method == 1) hipLaunchKernelGGL((k_seq_null<1, 4, 4>), grid, dim3(kCtBlock), 0, stream, a);
  else hipLaunchKernelGGL((k_seq_null<2, 2, 4>), grid, dim3(kCtBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_seq_retire(const SeqRetireArgs& a, hipStream_t stream) {
  if (a.nactive == 0) return hipSuccess;
  constexpr int NW = kSeqRetireBlock / 64;
  const int64_t blocks = (a.nactive + NW - 1) / NW;
  if (blocks > 0x7fffffff || a.nw < 1 || a.nw > a.wstride || a.h < 1u || !a.bits || !a.active || !a.next || !a.n_next || !a.prior ||
      !a.n_perm)
    return hipErrorInvalidValue;
  if (g_launch_trace) fprintf(stderr, "launch k_seq_retire active=%lld words=%d\n", (long long)a.nactive, a.nw);
  hipLaunchKernelGGL(k_seq_retire, dim3((unsigned)blocks), dim3(kSeqRetireBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

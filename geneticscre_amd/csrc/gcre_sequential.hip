// gcre_sequential.hip -- sequential permutation p-values of caller-given sets (gcre_score_sets_sequential):
// every set is permuted until its null score has reached its observed score h times, in batches of permutations that are
// never resident as a whole.
//   * k_seq_masks   the masks of permutations [r0, r0 + nb) by the rule of gcre_sequential.h (k_generate_masks' rule, caller
//                   strata, a 64-bit permutation index), one permutation per lane, in k_set_null's mask layout
//                   [W32p][stride] (permutation-minor; padding rows and padding columns zero)
//   * k_seq_null    k_set_null's count loop (gcre_sets.hip) over the sets of an active list; the finish compares every null
//                   score with the set's threshold and writes one ballot word per (active slot, 64 consecutive permutations)
//   * k_seq_retire  one wave per active slot: the slot's exceedances in the batch, by a wave prefix sum over the words of its
//                   bit row; a set whose h-th exceedance lies in the batch gets its position and leaves, the others go on
//                   the next active list
// k_seq_null keeps k_set_null's mapping: lanes own permutations (8 per lane), a set's words are wave-uniform (scalar loads),
// the mask tile goes through LDS and is shared by the block's four waves.  Every global write is a vector store or a vector
// atomic.  The context-side entry is in gcre_host_sequential.hip.
#include "gcre_kernels.h"
#include "gcre_sequential.h"

namespace gcre {
namespace {

typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;
typedef u32 __attribute__((ext_vector_type(4))) u32x4;

// wave-uniform read-only inputs through the constant address space: scalar loads
#define SEQ_CONSTANT __attribute__((address_space(4)))
template <typename T>
__device__ __forceinline__ const T SEQ_CONSTANT* seq_const(const T* p) {
  return (const T SEQ_CONSTANT*)p;
}

__device__ __forceinline__ u64 seq_diag(u64 t) { return (t * (t + 1)) >> 1; }

constexpr int kSeqBlock = 256;                // threads per block
constexpr int kSeqR = 8;                      // permutations per lane
constexpr int kSeqPT = 64 * kSeqR;            // permutations per tile
constexpr int kSeqWC = 4;                     // mask dwords per staged chunk (one s_load_dwordx4 per set and half)
constexpr int kSeqTW = kSeqPT / 64;           // ballot words per tile
static_assert(kSeqPT == kSetPermTile && kSeqPT == gcre_sequential::kSeqTile, "k_set_null's tile");

// column of the permutation tile that register j of a lane holds (k_set_null's layout)
__device__ __forceinline__ int seq_col(int lane, int j) { return (j >> 2) * 256 + lane * 4 + (j & 3); }

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
  const int32_t SEQ_CONSTANT* STR = seq_const(a.stratum);
  const u32 SEQ_CONSTANT* CASES = seq_const(a.cases_in);
  const u32 SEQ_CONSTANT* SIZE = seq_const(a.size_of);
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
__global__ __launch_bounds__(kSeqBlock, OCC) void k_seq_null(const SeqNullArgs a) {
  constexpr int R = kSeqR, WC = kSeqWC, PT = kSeqPT;
  constexpr int NW = kSeqBlock / 64;
  constexpr int TPB = NW * TPW;
  constexpr int CHUNK = WC * PT;                // dwords per staged mask chunk
  constexpr int VEC = CHUNK / 4 / kSeqBlock;    // uint4 per thread per chunk
  static_assert(VEC >= 1 && CHUNK % (4 * kSeqBlock) == 0, "staging shape");

  __shared__ __attribute__((aligned(16))) u32 lds[2][CHUNK];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = blockIdx.x % a.nkt;
  const int g = blockIdx.x / a.nkt;

  const u32 SEQ_CONSTANT* ROWS = seq_const(a.rows);
  const u32 SEQ_CONSTANT* TOT = seq_const(a.tot);
  const u32 SEQ_CONSTANT* THR = seq_const(a.thr);
  const u32 SEQ_CONSTANT* ACT = seq_const(a.active);

  const int nchunks = a.W32p / WC;
  const u32* mask_tile = a.masks + (size_t)kt * PT;   // column offset of this permutation tile

  // ---- mask staging: chunk c = rows [c*WC, c*WC+WC) x PT columns, row-major in LDS (as k_set_null) ----
  u32x4 stage[VEC];
  u32 voff[VEC];
#pragma unroll
  for (int i = 0; i < VEC; i++) {
    const int e = tid + i * kSeqBlock;
    voff[i] = (u32)((e / (PT / 4)) * a.stride + (e % (PT / 4)) * 4) * 4u;
  }
  const size_t chunk_bytes = (size_t)WC * a.stride * 4;
  auto stage_load = [&](int c) {
    const char* cb = (const char*)mask_tile + (size_t)c * chunk_bytes;
#pragma unroll
    for (int i = 0; i < VEC; i++) stage[i] = *(const u32x4*)(cb + voff[i]);
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < VEC; i++) *(u32x4*)(&lds[buf][(tid + i * kSeqBlock) * 4]) = stage[i];
  };

  // whether the permutation of each register is one of the batch (the padding of the last tile never counts)
  bool live[R];
#pragma unroll
  for (int j = 0; j < R; j++) live[j] = kt * PT + seq_col(lane, j) < a.K;

  stage_load(0);
  stage_store(0);
  __syncthreads();
  int buf = 0;

  const size_t rs = (size_t)M * a.W32p;   // dwords per set: (+) half, then (-) half (method 2)

  for (i64 pt = g; pt < a.npt; pt += a.pgroups) {
    const i64 sbase = pt * TPB + (i64)wave * TPW;   // the wave's first slot of the active list
    u32 acc[M][TPW][R];
#pragma unroll
    for (int h = 0; h < M; h++)
#pragma unroll
      for (int t = 0; t < TPW; t++)
#pragma unroll
        for (int j = 0; j < R; j++) acc[h][t][j] = 0u;

    // the sets of this wave's slots and their row offsets, wave-uniform; a slot past the end reads the last slot's set (its
    // result is dropped)
    size_t o[TPW];
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const i64 sl = sbase + t < a.nactive ? sbase + t : a.nactive - 1;
      o[t] = (size_t)ACT[sl] * rs;
    }

    // software pipeline over the flattened (chunk, set) sequence, as k_set_null
    u32x4 nx[M];
    auto fetch = [&](int c, int t) {
      const u32 SEQ_CONSTANT* b = ROWS + o[t] + (size_t)c * WC;
      nx[0] = *(const u32x4 SEQ_CONSTANT*)b;
      if constexpr (M == 2) nx[1] = *(const u32x4 SEQ_CONSTANT*)(b + a.W32p);
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

    // ---- null scores on each set's table diagonal (as k_set_null); the compares by ballot; the tile's eight words ----
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      if (sbase + t >= a.nactive) continue;   // wave-uniform
      const i64 q = (i64)ACT[sbase + t];   // (read again: nothing of it is kept across the count loop)
      const u32 thr = THR[q];
      u32 v[R];
      if constexpr (M == 1) {
        const u32* diag = (const u32*)a.t32 + seq_diag(TOT[q]);
#pragma unroll
        for (int j = 0; j < R; j++) v[j] = diag[acc[0][t][j]];
      } else {
        const double* dp = a.d64 + seq_diag(TOT[2 * q]);
        const double* dn = a.d64n + seq_diag(TOT[2 * q + 1]);
#pragma unroll
        for (int j = 0; j < R; j++) {
          float f = (float)(dp[acc[0][t][j]] + dn[acc[M - 1][t][j]]);
          f = (f > 0.0f) ? f : 0.0f;   // NaN and negatives fold as 0, as into the join's maxima
          v[j] = __float_as_uint(f);
        }
      }
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
__global__ __launch_bounds__(kSeqBlock) void k_seq_retire(const SeqRetireArgs a) {
  constexpr int NW = kSeqBlock / 64;
  __shared__ u32 keep[NW];
  __shared__ u32 base_s;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const i64 slot = (i64)blockIdx.x * NW + wave;
  const u32 SEQ_CONSTANT* ACT = seq_const(a.active);
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
  if ((int64_t)a.nkt * a.pgroups > 0x7fffffff || a.nkt < 1 || a.pgroups < 1 || a.W32p % kSeqWC != 0 || a.W32p < kSeqWC ||
      a.stride % kSeqPT != 0 || (int64_t)a.nkt * kSeqPT > a.stride || a.K > a.nkt * kSeqPT || (int64_t)a.W32p * a.stride > 0x40000000 ||
      !a.active || !a.bits)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.nkt * a.pgroups));
  if (g_launch_trace)
    fprintf(stderr, "launch k_seq_null active=%lld npt=%lld pgroups=%d perms=%d\n", (long long)a.nactive, (long long)a.npt, a.pgroups, a.K);
  if (method == 1) hipLaunchKernelGGL((k_seq_null<1, 4, 4>), grid, dim3(kSeqBlock), 0, stream, a);
  else hipLaunchKernelGGL((k_seq_null<2, 2, 4>), grid, dim3(kSeqBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_seq_retire(const SeqRetireArgs& a, hipStream_t stream) {
  if (a.nactive == 0) return hipSuccess;
  constexpr int NW = kSeqBlock / 64;
  const int64_t blocks = (a.nactive + NW - 1) / NW;
  if (blocks > 0x7fffffff || a.nw < 1 || a.nw > a.wstride || a.h < 1u || !a.bits || !a.active || !a.next || !a.n_next || !a.prior ||
      !a.n_perm)
    return hipErrorInvalidValue;
  if (g_launch_trace) fprintf(stderr, "launch k_seq_retire active=%lld words=%d\n", (long long)a.nactive, a.nw);
  hipLaunchKernelGGL(k_seq_retire, dim3((unsigned)blocks), dim3(kSeqBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

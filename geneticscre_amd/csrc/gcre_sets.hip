// gcre_sets.hip -- permutation tests of caller-given sets of carrier rows: named paths, gene sets (gcre_score_sets).
//   * k_set_observed  the observed score of every set, read from the device's value table (methods.h:90, :255)
//   * k_set_null      per (set, permutation): the AND+popcount of the set's union row(s) with the permutation's case
//                     mask, the null score the join's kernels fold into their maxima (methods.h:96-103, :220-230), the
//                     count of permutations whose null score reaches the set's observed score, and the per-permutation
//                     maximum over the sets of the launch
// The context-side entry, gcre_score_sets, is in gcre_host_sets.hip.  DESIGN.md §3.6.
//
// k_set_null is k_null's mapping (gcre_kernels.hip) with one operand row instead of two: lanes own permutations (8 per
// lane), a set's words are wave-uniform (scalar loads), the mask tile goes through LDS and is shared by the block's four
// waves, and a block stays on one permutation tile.  Every global write is a vector atomic.
#include "gcre_kernels.h"

namespace gcre {
namespace {

typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;
typedef u32 __attribute__((ext_vector_type(4))) u32x4;

// wave-uniform read-only inputs through the constant address space: scalar loads
#define SETS_CONSTANT __attribute__((address_space(4)))
template <typename T>
__device__ __forceinline__ const T SETS_CONSTANT* sets_const(const T* p) {
  return (const T SETS_CONSTANT*)p;
}

__device__ __forceinline__ u64 sets_diag(u64 t) { return (t * (t + 1)) >> 1; }

constexpr int kSetBlock = 256;                // threads per block
constexpr int kSetR = 8;                      // permutations per lane
constexpr int kSetPT = 64 * kSetR;            // permutations per tile (= kSetPermTile)
constexpr int kSetWC = 4;                     // mask dwords per staged chunk (one s_load_dwordx4 per set and half)
static_assert(kSetPT == kSetPermTile, "tile");

// column of the permutation tile that register j of a lane holds: permutations {4 lane .. 4 lane + 3} and
// {256 + 4 lane ..}, so that both ds_read_b128 of a mask row have a 16-byte lane stride (k_null's R = 8 layout)
__device__ __forceinline__ int set_col(int lane, int j) { return (j >> 2) * 256 + lane * 4 + (j & 3); }

}  // namespace

__global__ __launch_bounds__(256) void k_set_observed(const int32_t* __restrict__ cnt, int64_t S, int method,
                                                      const double* __restrict__ dvt, double* __restrict__ obs) {
  const i64 s = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int32_t* c = cnt + 4 * s;   // cases_pos, ctrls_pos, cases_neg, ctrls_neg
  const u64 tp = (u64)c[0] + (u64)c[1];
  double v = dvt[sets_diag(tp) + (u64)c[0]];
  if (method == 2) {
    const u64 tn = (u64)c[2] + (u64)c[3];
    v = v + dvt[sets_diag(tn) + (u64)c[2]];
  }
  obs[s] = v;
}

// M method, TPW sets per wave and set tile, OCC waves per SIMD the register allocation must admit
template <int M, int TPW, int OCC>
__global__ __launch_bounds__(kSetBlock, OCC) void k_set_null(const SetNullArgs a) {
  constexpr int R = kSetR, WC = kSetWC, PT = kSetPT;
  constexpr int NW = kSetBlock / 64;
  constexpr int TPB = NW * TPW;
  constexpr int CHUNK = WC * PT;                // dwords per staged mask chunk
  constexpr int VEC = CHUNK / 4 / kSetBlock;    // uint4 per thread per chunk
  static_assert(VEC >= 1 && CHUNK % (4 * kSetBlock) == 0, "staging shape");

  __shared__ __attribute__((aligned(16))) u32 lds[2][CHUNK];
  __shared__ u32 red[NW][PT];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = blockIdx.x % a.nkt;
  const int g = blockIdx.x / a.nkt;

  const u32 SETS_CONSTANT* ROWS = sets_const(a.rows);
  const u32 SETS_CONSTANT* TOT = sets_const(a.tot);
  const u32 SETS_CONSTANT* THR = sets_const(a.thr);

  const int nchunks = a.W32p / WC;
  const u32* mask_tile = a.masks + (size_t)kt * PT;   // column offset of this permutation tile

  // ---- mask staging: chunk c = rows [c*WC, c*WC+WC) x PT columns, row-major in LDS ----
  u32x4 stage[VEC];
  u32 voff[VEC];
#pragma unroll
  for (int i = 0; i < VEC; i++) {
    const int e = tid + i * kSetBlock;
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
    for (int i = 0; i < VEC; i++) *(u32x4*)(&lds[buf][(tid + i * kSetBlock) * 4]) = stage[i];
  };

  // whether the permutation of each register is one of the K (the padding up to Kpad never counts)
  bool live[R];
#pragma unroll
  for (int j = 0; j < R; j++) live[j] = kt * PT + set_col(lane, j) < a.K;

  u32 nmax[R];
#pragma unroll
  for (int j = 0; j < R; j++) nmax[j] = 0u;

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

    // software pipeline over the flattened (chunk, set) sequence: the scalar loads of the next set's words are in flight
    // while the VALU works on the current one
    u32x4 nx[M];
    auto fetch = [&](int c, int t) {
      const u32 SETS_CONSTANT* b = ROWS + o[t] + (size_t)c * WC;
      nx[0] = *(const u32x4 SETS_CONSTANT*)b;
      if constexpr (M == 2) nx[1] = *(const u32x4 SETS_CONSTANT*)(b + a.W32p);
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

    // ---- null scores on each set's table diagonal; n_ge by ballot; running maxima ----
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const i64 q = qbase + t;
      if (q >= a.nsets) continue;   // wave-uniform
      const u32 thr = THR[q];
      u32 v[R];
      if constexpr (M == 1) {
        // the sanitised f32 table: non-negative floats, ordered as their bit patterns
        const u32* diag = (const u32*)a.t32 + sets_diag(TOT[q]);
#pragma unroll
        for (int j = 0; j < R; j++) v[j] = diag[acc[0][t][j]];
      } else {
        // vtmax[pp][|P| - pp] + vtmax[|N| - pn][pn] (d64n: d64, or its mirror image where vtmax is not symmetric), folded as
        // k_null folds it
        const double* dp = a.d64 + sets_diag(TOT[2 * q]);
        const double* dn = a.d64n + sets_diag(TOT[2 * q + 1]);
#pragma unroll
        for (int j = 0; j < R; j++) {
          float f = (float)(dp[acc[0][t][j]] + dn[acc[M - 1][t][j]]);
          f = (f > 0.0f) ? f : 0.0f;   // NaN and negatives fold as 0, as into the join's maxima
          v[j] = __float_as_uint(f);
        }
      }
      u32 ge = 0;
#pragma unroll
      for (int j = 0; j < R; j++) {
        ge += (u32)__popcll(__ballot(live[j] && v[j] >= thr));
        const u32 x = live[j] ? v[j] : 0u;
        nmax[j] = (x > nmax[j]) ? x : nmax[j];
      }
      if (lane == 0 && ge != 0u) atomicAdd(a.n_ge + q, (unsigned long long)ge);
    }
  }

  if (!a.fam_bits) return;   // uniform over the grid
  // ---- block reduction, then one atomic per permutation ----
#pragma unroll
  for (int j = 0; j < R; j++) red[wave][set_col(lane, j)] = nmax[j];
  __syncthreads();
  for (int i = tid; i < PT; i += kSetBlock) {
    u32 v = red[0][i];
#pragma unroll
    for (int w = 1; w < NW; w++) v = (red[w][i] > v) ? red[w][i] : v;
    if (v != 0u) atomicMax(a.fam_bits + (size_t)kt * PT + i, v);
  }
}

int set_null_tile_sets(int method) { return (kSetBlock / 64) * (method == 1 ? 4 : 2); }

hipError_t launch_set_observed(const int32_t* cnt, int64_t S, int method, const double* dvt, double* obs,
                               hipStream_t stream) {
  if (S == 0) return hipSuccess;
  hipLaunchKernelGGL(k_set_observed, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, stream, cnt, S, method, dvt, obs);
  return hipGetLastError();
}

hipError_t launch_set_null(const SetNullArgs& a, int method, hipStream_t stream) {
  if (a.nsets == 0 || a.K == 0) return hipSuccess;
  if ((int64_t)a.nkt * a.pgroups > 0x7fffffff || a.W32p % kSetWC != 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.nkt * a.pgroups));
  if (g_launch_trace)   // a block walks `per` set tiles
    fprintf(stderr, "launch k_set_null npt=%lld pgroups=%d per=%lld\n", (long long)a.npt, a.pgroups,
            (long long)((a.npt + a.pgroups - 1) / a.pgroups));
  if (method == 1) hipLaunchKernelGGL((k_set_null<1, 4, 4>), grid, dim3(kSetBlock), 0, stream, a);
  else hipLaunchKernelGGL((k_set_null<2, 2, 4>), grid, dim3(kSetBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

// gcre_sets.hip -- permutation tests of caller-given sets of carrier rows: named paths, gene sets (gcre_score_sets).
//   * k_set_observed  the observed score of every set, read from the device's value table (methods.h:90, :255)
//   * k_set_null      per (set, permutation): the AND+popcount of the set's union row(s) with the permutation's case
//                     mask, the null score the join's kernels fold into their maxima (methods.h:96-103, :220-230), the
//                     count of permutations whose null score reaches the set's observed score, and the per-permutation
//                     maximum over the sets of the launch
// The context-side entry, gcre_score_sets, is in gcre_host_sets.hip.  DESIGN.md §3.6.
//
// k_set_null counts with count_tile (gcre_count_tile.h: the mask stream through LDS, the count loop and the look-up, shared
// with the other kernels that test given rows); row = set.  Every global write is a vector atomic.
#include "gcre_count_tile.h"

namespace gcre {

__global__ __launch_bounds__(256) void k_set_observed(const int32_t* __restrict__ cnt, int64_t S, int method,
                                                      const double* __restrict__ dvt, double* __restrict__ obs) {
  const i64 s = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int32_t* c = cnt + 4 * s;   // cases_pos, ctrls_pos, cases_neg, ctrls_neg
  const u64 tp = (u64)c[0] + (u64)c[1];
  double v = dvt[tri_index(tp) + (u64)c[0]];
  if (method == 2) {
    const u64 tn = (u64)c[2] + (u64)c[3];
    v = v + dvt[tri_index(tn) + (u64)c[2]];
  }
  obs[s] = v;
}

// M method, TPW sets per wave and set tile, OCC waves per SIMD the register allocation must admit
template <int M, int TPW, int OCC>
__global__ __launch_bounds__(kCtBlock, OCC) void k_set_null(const SetNullArgs a) {
  constexpr int R = kCtR, PT = kCtPT, NW = kCtWaves;
  constexpr int TPB = NW * TPW;

  __shared__ __attribute__((aligned(16))) u32 lds[2][kCtChunk];
  __shared__ u32 red[NW][PT];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = blockIdx.x % a.nkt;
  const int g = blockIdx.x / a.nkt;

  const u32 GCRE_CONSTANT* ROWS = as_const(a.rows);
  const u32 GCRE_CONSTANT* TOT = as_const(a.tot);
  const u32 GCRE_CONSTANT* THR = as_const(a.thr);

  // whether the permutation of each register is one of the K (the padding up to Kpad never counts)
  bool live[R];
#pragma unroll
  for (int j = 0; j < R; j++) live[j] = kt * PT + ct_col(lane, j) < a.K;

  u32 nmax[R];
#pragma unroll
  for (int j = 0; j < R; j++) nmax[j] = 0u;

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

    // ---- null scores on each set's table diagonal; n_ge by ballot; running maxima ----
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const i64 q = qbase + t;
      if (q >= a.nsets) continue;   // wave-uniform
      const u32 thr = THR[q];
      u32 v[R];
      null_scores<M>(a.t32, a.d64, a.d64n, TOT, q, acc.v[0][t], acc.v[M - 1][t], v);
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
  for (int j = 0; j < R; j++) red[wave][ct_col(lane, j)] = nmax[j];
  __syncthreads();
  for (int i = tid; i < PT; i += kCtBlock) {
    u32 v = red[0][i];
#pragma unroll
    for (int w = 1; w < NW; w++) v = (red[w][i] > v) ? red[w][i] : v;
    if (v != 0u) atomicMax(a.fam_bits + (size_t)kt * PT + i, v);
  }
}

int set_null_tile_sets(int method) { return kCtWaves * (method == 1 ? 4 : 2); }

hipError_t launch_set_observed(const int32_t* cnt, int64_t S, int method, const double* dvt, double* obs,
                               hipStream_t stream) {
  if (S == 0) return hipSuccess;
  hipLaunchKernelGGL(k_set_observed, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, stream, cnt, S, method, dvt, obs);
  return hipGetLastError();
}

hipError_t launch_set_null(const SetNullArgs& a, int method, hipStream_t stream) {
  if (a.nsets == 0 || a.K == 0) return hipSuccess;
  if ((int64_t)a.nkt * a.pgroups > 0x7fffffff || a.W32p % kCtWC != 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.nkt * a.pgroups));
  if (g_launch_trace)   // a block walks `per` set tiles
    fprintf(stderr, "launch k_set_null npt=%lld pgroups=%d per=%lld\n", (long long)a.npt, a.pgroups,
            (long long)((a.npt + a.pgroups - 1) / a.pgroups));
  if (method == 1) hipLaunchKernelGGL((k_set_null<1, 4, 4>), grid, dim3(kCtBlock), 0, stream, a);
  else hipLaunchKernelGGL((k_set_null<2, 2, 4>), grid, dim3(kCtBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

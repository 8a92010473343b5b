// gcre_strata.hip -- stratified scores of caller-given sets: every stratum scored on its own counts against its own table,
// the terms summed, the same sum under every permutation (gcre_score_sets_strata).
//   * k_strata_masks     the stratum ids as S indicator rows Z_s, cut by wave ballots
//   * k_strata_check     every resident mask counted against every Z_s: the pairs that do not hold the stratum's cases
//   * k_strata_rows      per set: the S rows "union & Z_s" in k_set_null's row layout, and the counts SetUnion::build
//                        (gcre_setlists.h) gives such rows
//   * k_strata_observed  per set: the carrier totals k_strata_null reads, the S observed terms and their sum
//   * k_strata_null      per (set, permutation): the sum over the strata of the f64 look-up in stratum s's table, the count of
//                        permutations whose sum reaches the set's observed sum, and the per-permutation maximum over the
//                        sets of the launch
// The context-side entry is in gcre_host_strata.hip, the host plan (checks, table offsets, slabs) in gcre_strata.h.
//
// k_strata_rows is k_prefix_rows' mapping (gcre_prefix.hip): one wave per set and 64-dword stretch of the row, lanes over the
// dwords, a wave reduction and one 32-bit vector atomic per non-zero count.
// k_strata_null is k_prefix_null's shape: the rows of a wave's tile are consecutive strata of ONE set, counted with count_tile
// (gcre_count_tile.h); the running f64 sum stays in registers.  S is the same for every set, so the last, narrower tiles are
// count_tile instances of their own width: a set's S rows are counted and no clamped copy of one.  The tables are the raw ones
// in diagonal-major form (k_table_to_diag), one behind the other; the (-) half reads its diagonal at tot - count, so no mirror
// table is needed.
// Every global write is a vector store or a vector atomic.
#include "gcre_count_tile.h"

#include <type_traits>

namespace gcre {
namespace {

constexpr int kStrRowsBlock = 256;            // threads per block of k_strata_rows: four waves
constexpr int kStrCheckRows = 4;              // indicator rows per wave of k_strata_check: 4 waves x 4 = the most strata

}  // namespace

// One wave per 64 patients: bit p & 31 of dword p >> 5 of row s says whether patient p is of stratum s.  Patients at and
// beyond n_patients vote for no stratum, so the padding up to W32p is zero.
__global__ __launch_bounds__(64) void k_strata_masks(const StrataArgs a) {
  const int lane = threadIdx.x;
  const int p = blockIdx.x * 64 + lane;
  const int id = p < a.n_patients ? a.stratum[p] : -1;
  const int w = blockIdx.x * 2 + lane;   // lanes 0 and 1 store the wave's two dwords
  for (int s = 0; s < a.S; s++) {
    const u64 b = __ballot(id == s);
    if (lane < 2 && w < a.W32p) a.zrows[(size_t)s * a.W32p + w] = (u32)(b >> (32 * lane));
  }
}

// One block per permutation tile; wave w counts the indicator rows [4 w, 4 w + 4) against the tile's masks.
__global__ __launch_bounds__(kCtBlock, 4) void k_strata_check(const StrataArgs a) {
  constexpr int R = kCtR, PT = kCtPT, TPW = kStrCheckRows;

  __shared__ __attribute__((aligned(16))) u32 lds[2][kCtChunk];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kt = blockIdx.x;

  MaskStream ms(lds, a.masks + (size_t)kt * PT, a.Kpad);

  // a row past the last stratum reads the last stratum's row (its result is dropped)
  size_t o[TPW];
#pragma unroll
  for (int t = 0; t < TPW; t++) {
    const int s = wave * TPW + t < a.S ? wave * TPW + t : a.S - 1;
    o[t] = (size_t)s * a.W32p;
  }
  const TileCounts<1, TPW> acc = count_tile<1, TPW>(ms, as_const((const u32*)a.zrows), o, a.W32p);

  u32 bad = 0;
#pragma unroll
  for (int t = 0; t < TPW; t++) {
    const int s = wave * TPW + t;
    if (s >= a.S) continue;   // wave-uniform
    const u32 want = as_const(a.cases_in)[s];
#pragma unroll
    for (int j = 0; j < R; j++) {
      const bool live = kt * PT + ct_col(lane, j) < a.K;   // the padding up to Kpad never counts
      bad += (u32)__popcll(__ballot(live && acc.v[0][t][j] != want));
    }
  }
  if (lane == 0 && bad != 0u) atomicAdd(a.violations, bad);
}

template <int M>
__global__ __launch_bounds__(kStrRowsBlock) void k_strata_rows(const StrataArgs a) {
  const int nch = (a.W32p + 63) / 64;   // 64-dword stretches of a row: one wave each
  const i64 wv = (i64)blockIdx.x * (kStrRowsBlock / 64) + (threadIdx.x >> 6);
  const i64 e = wv / nch;
  const int lane = threadIdx.x & 63;
  if (e >= a.nslots) return;   // the whole wave
  const int split = a.n_cases >> 5;
  const u32 split_mask = (1u << (a.n_cases & 31)) - 1u;
  const size_t rs = (size_t)M * a.W32p;
  const int w = (int)(wv % nch) * 64 + lane;
  const bool in_row = w < a.W32p;
  const u32 cm = w < split ? 0xffffffffu : w == split ? split_mask : 0u;
  // the wave's 64 dwords of the set's union, cut by every stratum in turn
  const u32 UP = in_row ? a.urows[(size_t)e * rs + w] : 0u;
  const u32 UN = (M == 2 && in_row) ? a.urows[(size_t)e * rs + a.W32p + w] : 0u;
  for (int s = 0; s < a.S; s++) {
    const u32 z = in_row ? a.zrows[(size_t)s * a.W32p + w] : 0u;
    const u32 P = UP & z, N = UN & z;
    const size_t row = (size_t)e * a.S + s;
    if (in_row) {
      u32* out = a.rows + row * rs;
      out[w] = P;
      if (M == 2) out[a.W32p + w] = N;
    }
    u32 k0 = __popc(P & cm);    // cases_pos
    u32 k1 = __popc(P & ~cm);   // ctrls_pos
    u32 k2 = __popc(N & ~cm);   // cases_neg: the (-) half counts the other way round (SetUnion::build)
    u32 k3 = __popc(N & cm);    // ctrls_neg
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      k0 += __shfl_down(k0, d, 64);
      k1 += __shfl_down(k1, d, 64);
      if (M == 2) {
        k2 += __shfl_down(k2, d, 64);
        k3 += __shfl_down(k3, d, 64);
      }
    }
    if (lane == 0) {
      int32_t* c = a.cnt + row * 4;
      if (k0) atomicAdd(c + 0, (int32_t)k0);
      if (k1) atomicAdd(c + 1, (int32_t)k1);
      if (M == 2) {
        if (k2) atomicAdd(c + 2, (int32_t)k2);
        if (k3) atomicAdd(c + 3, (int32_t)k3);
      }
    }
  }
}

// One thread per slot: term_s = T_s[cases_pos][ctrls_pos] (+ T_s[cases_neg][ctrls_neg], in this order), summed from +0.0 in
// ascending s.  A stratum row holds patients of Z_s only, so its total is a diagonal the table has.
template <int M>
__global__ __launch_bounds__(256) void k_strata_observed(const StrataArgs a) {
  const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.nslots) return;
  double sum = 0.0;
  for (int s = 0; s < a.S; s++) {
    const size_t r = (size_t)e * a.S + s;
    const int32_t* c = a.cnt + 4 * r;
    const double* T = a.dvt + a.doff[s];
    const u64 tp = (u64)c[0] + (u64)c[1];
    a.tot[r * M] = (u32)tp;
    double term = T[tri_index(tp) + (u64)c[0]];
    if (M == 2) {
      const u64 tn = (u64)c[2] + (u64)c[3];
      a.tot[r * M + 1] = (u32)tn;
      term = term + T[tri_index(tn) + (u64)c[2]];
    }
    if (a.terms) a.terms[r] = term;
    sum = sum + term;
  }
  a.obs[e] = sum;
}

// M method, TPW strata per wave and full step tile, OCC waves per SIMD the register allocation must admit
template <int M, int TPW, int OCC>
__global__ __launch_bounds__(kCtBlock, OCC) void k_strata_null(const StrataArgs a) {
  constexpr int R = kCtR, PT = kCtPT, NW = kCtWaves;

  __shared__ __attribute__((aligned(16))) u32 lds[2][kCtChunk];
  __shared__ u64 red[NW][PT];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = blockIdx.x % a.nkt;
  const int g = blockIdx.x / a.nkt;

  const u32 GCRE_CONSTANT* ROWS = as_const((const u32*)a.rows);
  const u32 GCRE_CONSTANT* TOT = as_const((const u32*)a.tot);
  const i64 GCRE_CONSTANT* DOFF = as_const(a.doff);
  const PrefixWaveDev GCRE_CONSTANT* WV = as_const(a.waves) + (size_t)g * NW;

  // this wave's set; every set has S rows, so every wave of the block walks the same step tiles
  const int slot = WV[wave].slot;
  const bool idle = WV[wave].steps == 0;   // a wave without a set counts the slab's first row (its results are dropped)
  const i64 row0 = WV[wave].row0;

  // the running sum over this wave's strata, per permutation of the lane
  double sum[R];
#pragma unroll
  for (int j = 0; j < R; j++) sum[j] = 0.0;

  MaskStream ms(lds, a.masks + (size_t)kt * PT, a.Kpad);   // column offset of this permutation tile

  const size_t rs = (size_t)M * a.W32p;   // dwords per stratum row: (+) half, then (-) half (method 2)

  // One step tile: the T strata from kbase on (all below S, so no row is counted for nothing), one pass over the mask stream.
  auto tile = [&](auto width, int kbase) {
    constexpr int T = decltype(width)::value;
    i64 q[T];
    size_t o[T];
#pragma unroll
    for (int t = 0; t < T; t++) {
      q[t] = idle ? 0 : row0 + kbase + t;   // wave-uniform
      o[t] = (size_t)q[t] * rs;
    }

    const TileCounts<M, T> acc = count_tile<M, T>(ms, ROWS, o, a.W32p);

    // ---- per stratum one f64 look-up on the row's diagonal of the stratum's table, added in ascending s ----
    if (idle) return;   // wave-uniform
#pragma unroll
    for (int t = 0; t < T; t++) {
      const double* Tb = a.dvt + DOFF[kbase + t];
      const u32 tp = TOT[q[t] * M];
      const double* dp = Tb + tri_index(tp);
      if constexpr (M == 1) {
#pragma unroll
        for (int j = 0; j < R; j++) sum[j] = sum[j] + dp[acc.v[0][t][j]];
      } else {
        // T_s[|N & Z_s \ m|][|N & Z_s & m|]: the row index is the total minus the count
        const u32 tn = TOT[q[t] * M + 1];
        const double* dn = Tb + tri_index(tn);
#pragma unroll
        for (int j = 0; j < R; j++) sum[j] = sum[j] + (dp[acc.v[0][t][j]] + dn[tn - acc.v[1][t][j]]);
      }
    }
  };
  // full tiles of TPW strata, then the rest in tiles of half the width down to one: S rows are counted, never more
  // (uniform over the grid, so every thread of a block constructs and walks the stream the same number of times)
  int k = 0;
  for (; k + TPW <= a.S; k += TPW) tile(std::integral_constant<int, TPW>{}, k);
  if constexpr (TPW >= 4) {
    if (a.S - k >= 2) {
      tile(std::integral_constant<int, 2>{}, k);
      k += 2;
    }
  }
  if constexpr (TPW >= 2) {
    if (a.S - k >= 1) tile(std::integral_constant<int, 1>{}, k);
  }

  // ---- the set's end: n_ge by ballot over the live permutations, the sums into the null_scores slab ----
  bool live[R];
#pragma unroll
  for (int j = 0; j < R; j++) live[j] = kt * PT + ct_col(lane, j) < a.K;   // the padding up to Kpad never counts
  if (slot >= 0) {   // wave-uniform
    const double sc = as_const((const double*)a.obs)[slot];
    u32 ge = 0;
#pragma unroll
    for (int j = 0; j < R; j++) ge += (u32)__popcll(__ballot(live[j] && sum[j] >= sc));   // a NaN on either side never counts
    if (lane == 0 && ge != 0u) atomicAdd(a.n_ge + slot, (unsigned long long)ge);
    if (a.null_scores) {
      double* row = a.null_scores + (size_t)slot * a.Kpad + (size_t)kt * PT;
#pragma unroll
      for (int j = 0; j < R; j++) row[ct_col(lane, j)] = sum[j];
    }
  }

  if (!a.fam_bits) return;   // uniform over the grid
  // ---- block reduction, then one atomic per permutation: non-negative doubles order as their bit patterns ----
#pragma unroll
  for (int j = 0; j < R; j++)
    red[wave][ct_col(lane, j)] = (slot >= 0 && live[j] && sum[j] > 0.0) ? (u64)__double_as_longlong(sum[j]) : 0ull;   // NaN and negatives fold as +0
  __syncthreads();
  for (int i = tid; i < PT; i += kCtBlock) {
    u64 v = red[0][i];
#pragma unroll
    for (int w = 1; w < NW; w++) v = (red[w][i] > v) ? red[w][i] : v;
    if (v != 0ull) atomicMax(a.fam_bits + (size_t)kt * PT + i, (unsigned long long)v);
  }
}

hipError_t launch_strata_masks(const StrataArgs& a, hipStream_t stream) {
  if (a.S < 1 || a.S > 16 || a.W32p < 1 || (a.n_patients + 31) / 32 > a.W32p || !a.stratum || !a.zrows) return hipErrorInvalidValue;
  if (g_launch_trace) fprintf(stderr, "launch k_strata_masks strata=%d\n", a.S);
  hipLaunchKernelGGL(k_strata_masks, dim3((unsigned)((a.W32p + 1) / 2)), dim3(64), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_strata_check(const StrataArgs& a, hipStream_t stream) {
  if (a.K == 0) return hipSuccess;
  if (a.S < 1 || a.S > kCtWaves * kStrCheckRows || a.W32p % kCtWC != 0 || a.W32p < kCtWC || a.nkt < 1 ||
      (int64_t)a.nkt * kCtPT > a.Kpad || a.K > a.Kpad || !a.cases_in || !a.violations)
    return hipErrorInvalidValue;
  if (g_launch_trace) fprintf(stderr, "launch k_strata_check strata=%d nkt=%d\n", a.S, a.nkt);
  hipLaunchKernelGGL(k_strata_check, dim3((unsigned)a.nkt), dim3(kCtBlock), 0, stream, a);
  return hipGetLastError();
}

// one wave per slot and 64-dword stretch of a row; a grid that does not fit is refused, never clamped
hipError_t launch_strata_rows(const StrataArgs& a, int method, hipStream_t stream) {
  if (a.nslots == 0) return hipSuccess;
  if (a.nslots < 0 || a.S < 1 || a.S > 16 || a.nslots * a.S > 0x7fffffff || a.W32p < 1 || (method != 1 && method != 2))
    return hipErrorInvalidValue;
  const i64 waves = a.nslots * ((a.W32p + 63) / 64);
  const i64 blocks = (waves + kStrRowsBlock / 64 - 1) / (kStrRowsBlock / 64);
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  if (g_launch_trace) fprintf(stderr, "launch k_strata_rows slots=%lld strata=%d\n", (long long)a.nslots, a.S);
  if (method == 1) hipLaunchKernelGGL(k_strata_rows<1>, dim3((unsigned)blocks), dim3(kStrRowsBlock), 0, stream, a);
  else hipLaunchKernelGGL(k_strata_rows<2>, dim3((unsigned)blocks), dim3(kStrRowsBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_strata_observed(const StrataArgs& a, int method, hipStream_t stream) {
  if (a.nslots == 0) return hipSuccess;
  const i64 blocks = (a.nslots + 255) / 256;
  if (a.nslots < 0 || blocks > 0x7fffffff || a.S < 1 || a.S > 16 || (method != 1 && method != 2)) return hipErrorInvalidValue;
  if (method == 1) hipLaunchKernelGGL(k_strata_observed<1>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(k_strata_observed<2>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_strata_null(const StrataArgs& a, int method, hipStream_t stream) {
  if (a.nslots == 0 || a.K == 0) return hipSuccess;
  if (a.nblocks < 1 || (int64_t)a.nkt * a.nblocks > 0x7fffffff || a.W32p % kCtWC != 0 || a.W32p < kCtWC || a.nkt < 1 ||
      (int64_t)a.nkt * kCtPT > a.Kpad || a.K > a.Kpad || a.S < 1 || a.S > 16 || (int64_t)a.nblocks * kCtWaves < a.nslots ||
      (method != 1 && method != 2))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((int64_t)a.nkt * a.nblocks));
  if (g_launch_trace)
    fprintf(stderr, "launch k_strata_null slots=%lld strata=%d blocks=%d nkt=%d\n", (long long)a.nslots, a.S, a.nblocks, a.nkt);
  if (method == 1) hipLaunchKernelGGL((k_strata_null<1, 4, 4>), grid, dim3(kCtBlock), 0, stream, a);
  else hipLaunchKernelGGL((k_strata_null<2, 2, 4>), grid, dim3(kCtBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

// gcre_prefix.hip -- variable-threshold tests of caller-given sets: the best prefix of a set's member list, with the same
// maximum taken under every permutation (gcre_score_sets_prefix).
//   * k_prefix_rows  per set: the union rows of every step (a prefix of the member list that ends at a cut member), written
//                    in k_set_null's row layout, and the counts SetUnion::build (gcre_setlists.h) gives such rows
//   * k_prefix_pick  per set: the best observed step score, the smallest step that attains it, its counts, the f32 threshold
//                    pattern of that score; per step row the carrier totals k_prefix_null reads
//   * k_prefix_null  per (set, permutation): the maximum over the set's steps of the null score k_set_null gives a step row,
//                    the count of permutations whose maximum reaches the set's best observed score, and the
//                    per-permutation maximum over the sets of the launch
// The step rows are scored by k_set_observed (gcre_sets.hip) between the first two.  The context-side entry is in
// gcre_host_steps.hip, the host plan (steps, slabs, block table) in gcre_prefix.h.
//
// k_prefix_rows is k_set_residual's mapping (gcre_given.hip), lanes over the dwords of a row, with one wave per set and
// 64-dword stretch of the row: a wave's walk over the members is a chain of dependent loads, so the stretches of a row go to
// waves of their own.
// k_prefix_null counts with count_tile (gcre_count_tile.h), the rows of a wave's tile being consecutive steps of ONE set;
// the running maximum over the steps stays in registers.  Every global write is a vector store or a vector atomic.
#include "gcre_count_tile.h"

namespace gcre {
namespace {

constexpr int kPfxRowsBlock = 256;            // threads per block of k_prefix_rows: four waves

}  // namespace

template <int M>
__global__ __launch_bounds__(kPfxRowsBlock) void k_prefix_rows(const PrefixArgs a) {
  const int nch = (a.W32p + 63) / 64;   // 64-dword stretches of a row: one wave each
  const i64 wv = (i64)blockIdx.x * (kPfxRowsBlock / 64) + (threadIdx.x >> 6);
  const i64 e = wv / nch;
  const int lane = threadIdx.x & 63;
  if (e >= a.nslots) return;   // the whole wave
  const i64 s = a.which[e];
  const i64 sb = a.set_off[s], se = a.set_off[s + 1];
  const i64 r0 = a.row0[e];
  const int split = a.n_cases >> 5;
  const u32 split_mask = (1u << (a.n_cases & 31)) - 1u;
  const size_t rs = (size_t)M * a.W32p;
  // the wave's 64 dwords of the set's rows: it walks the members in order with running unions and, at every cut, stores
  // its dword of the step row and adds the step's counts (a wave reduction, then one 32-bit vector atomic per count, which
  // the waves of the row's other stretches add to as well)
  {
    const int w = (int)(wv % nch) * 64 + lane;
    const bool in_row = w < a.W32p;
    const bool has = in_row && w < a.W2 && w * 32 < a.n_patients;
    const int left = a.n_patients - w * 32;   // patients from this dword on
    const u32 keep = has ? (left < 32 ? (1u << left) - 1u : 0xffffffffu) : 0u;
    const u32 cm = w < split ? 0xffffffffu : w == split ? split_mask : 0u;
    u32 P = 0, N = 0;
    i64 row = r0;
    for (i64 i = sb; i < se; i++) {
      if (has) {
        const u32 x = a.gene_rows[(i64)a.members[i] * a.W2 + w] & keep;
        if (M == 2 && a.signs && a.signs[i] == -1) N |= x;
        else P |= x;
      }
      if (a.cut && a.cut[i] == 0 && i + 1 != se) continue;   // wave-uniform
      if (in_row) {
        u32* out = a.rows + (size_t)row * rs;
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
        int32_t* c = a.cnt + (size_t)row * 4;
        if (k0) atomicAdd(c + 0, (int32_t)k0);
        if (k1) atomicAdd(c + 1, (int32_t)k1);
        if (M == 2) {
          if (k2) atomicAdd(c + 2, (int32_t)k2);
          if (k3) atomicAdd(c + 3, (int32_t)k3);
        }
      }
      row++;
    }
  }
}

// The bit pattern of the smallest float x with (double)x >= score among the non-negative floats: f32_threshold of the host
// side (gcre_threshold.h)
__device__ __forceinline__ u32 pfx_threshold(double score) {
  if (score != score) return 0x7f800001u;
  if (score <= 0) return 0u;
  const float f = (float)score;
  u32 b = __float_as_uint(f);
  if ((double)f < score) b += 1u;   // f is finite and not negative: the next float up
  return b;
}

template <int M>
__global__ __launch_bounds__(256) void k_prefix_pick(const PrefixArgs a) {
  const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.nslots) return;
  const i64 r0 = a.row0[e], r1 = a.row0[e + 1];
  double best = 0;
  i64 at = -1;
  for (i64 r = r0; r < r1; r++) {
    const int32_t* c = a.cnt + 4 * r;
    a.tot[r * M] = (u32)c[0] + (u32)c[1];
    if (M == 2) a.tot[r * M + 1] = (u32)c[2] + (u32)c[3];
    const double v = a.obs[r];
    if (v != v) continue;                          // a NaN step is skipped
    if (at < 0 || v > best) { best = v; at = r; }  // the smallest step that attains the maximum
  }
  PrefixPick p;
  p.score = at < 0 ? __longlong_as_double(0x7ff8000000000000ll) : best;
  p.best_step = at < 0 ? -1 : (int32_t)(at - r0);
#pragma unroll
  for (int i = 0; i < 4; i++) p.cnt[i] = at < 0 ? 0 : a.cnt[4 * at + i];
  p.pad = 0;
  a.pick[e] = p;
  a.thr[e] = pfx_threshold(p.score);
}

// M method, TPW steps per wave and step tile, OCC waves per SIMD the register allocation must admit
template <int M, int TPW, int OCC>
__global__ __launch_bounds__(kCtBlock, OCC) void k_prefix_null(const PrefixArgs a) {
  constexpr int R = kCtR, PT = kCtPT, NW = kCtWaves;

  __shared__ __attribute__((aligned(16))) u32 lds[2][kCtChunk];
  __shared__ u32 red[NW][PT];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = blockIdx.x % a.nkt;
  const int g = blockIdx.x / a.nkt;

  const u32 GCRE_CONSTANT* ROWS = as_const(a.rows);
  const u32 GCRE_CONSTANT* TOT = as_const(a.tot);
  const PrefixWaveDev GCRE_CONSTANT* WV = as_const(a.waves) + (size_t)g * NW;

  // this wave's set, and the step tiles the block walks: those of its first wave, the longest of the four (gcre_prefix.h)
  const int slot = WV[wave].slot;
  const int nsteps = WV[wave].steps;
  const i64 row0 = WV[wave].row0;
  const int ntiles = (WV[0].steps + TPW - 1) / TPW;

  // the running maximum over this wave's steps, per permutation of the lane
  u32 tmax[R];
#pragma unroll
  for (int j = 0; j < R; j++) tmax[j] = 0u;

  MaskStream ms(lds, a.masks + (size_t)kt * PT, a.Kpad);   // column offset of this permutation tile

  const size_t rs = (size_t)M * a.W32p;   // dwords per step row: (+) half, then (-) half (method 2)

  for (int st = 0; st < ntiles; st++) {
    const int kbase = st * TPW;
    // rows of this wave's steps, wave-uniform; a step past the set's end reads the set's last row and a wave without a
    // set the slab's first row (their results are dropped)
    i64 q[TPW];
    size_t o[TPW];
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const int k = kbase + t < nsteps ? kbase + t : (nsteps > 0 ? nsteps - 1 : 0);
      q[t] = row0 + k;
      o[t] = (size_t)q[t] * rs;
    }

    const TileCounts<M, TPW> acc = count_tile<M, TPW>(ms, ROWS, o, a.W32p);

    // ---- null scores on each step's table diagonal, folded into the running maximum ----
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      if (kbase + t >= nsteps) continue;   // wave-uniform
      u32 v[R];
      null_scores<M>(a.t32, a.d64, a.d64n, TOT, q[t], acc.v[0][t], acc.v[M - 1][t], v);
#pragma unroll
      for (int j = 0; j < R; j++) tmax[j] = (v[j] > tmax[j]) ? v[j] : tmax[j];
    }
  }

  // ---- the set's end: n_ge by ballot over the live permutations, T into the null_max slab ----
  bool live[R];
#pragma unroll
  for (int j = 0; j < R; j++) live[j] = kt * PT + ct_col(lane, j) < a.K;   // the padding up to Kpad never counts
  if (slot >= 0) {   // wave-uniform
    const u32 thr = as_const(a.thr)[slot];
    u32 ge = 0;
#pragma unroll
    for (int j = 0; j < R; j++) ge += (u32)__popcll(__ballot(live[j] && tmax[j] >= thr));
    if (lane == 0 && ge != 0u) atomicAdd(a.n_ge + slot, (unsigned long long)ge);
    if (a.null_max) {
      u32* row = a.null_max + (size_t)slot * a.Kpad + (size_t)kt * PT;
      u32x4 v0, v1;
      v0.x = tmax[0]; v0.y = tmax[1]; v0.z = tmax[2]; v0.w = tmax[3];
      v1.x = tmax[4]; v1.y = tmax[5]; v1.z = tmax[6]; v1.w = tmax[7];
      *(u32x4*)(row + lane * 4) = v0;
      *(u32x4*)(row + 256 + lane * 4) = v1;
    }
  }

  if (!a.fam_bits) return;   // uniform over the grid
  // ---- block reduction, then one atomic per permutation ----
#pragma unroll
  for (int j = 0; j < R; j++) red[wave][ct_col(lane, j)] = (slot >= 0 && live[j]) ? tmax[j] : 0u;
  __syncthreads();
  for (int i = tid; i < PT; i += kCtBlock) {
    u32 v = red[0][i];
#pragma unroll
    for (int w = 1; w < NW; w++) v = (red[w][i] > v) ? red[w][i] : v;
    if (v != 0u) atomicMax(a.fam_bits + (size_t)kt * PT + i, v);
  }
}

// one wave per slot and 64-dword stretch of a row; a grid that does not fit is refused, never clamped
hipError_t launch_prefix_rows(const PrefixArgs& a, int method, hipStream_t stream) {
  if (a.nslots == 0) return hipSuccess;
  if (a.nslots < 0 || a.W2 < 1 || a.W32p < a.W2 || (method != 1 && method != 2)) return hipErrorInvalidValue;
  const i64 waves = a.nslots * ((a.W32p + 63) / 64);
  const i64 blocks = (waves + kPfxRowsBlock / 64 - 1) / (kPfxRowsBlock / 64);
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  if (g_launch_trace) fprintf(stderr, "launch k_prefix_rows slots=%lld rows=%lld\n", (long long)a.nslots, (long long)a.nrows);
  if (method == 1) hipLaunchKernelGGL(k_prefix_rows<1>, dim3((unsigned)blocks), dim3(kPfxRowsBlock), 0, stream, a);
  else hipLaunchKernelGGL(k_prefix_rows<2>, dim3((unsigned)blocks), dim3(kPfxRowsBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_prefix_pick(const PrefixArgs& a, int method, hipStream_t stream) {
  if (a.nslots == 0) return hipSuccess;
  const i64 blocks = (a.nslots + 255) / 256;
  if (a.nslots < 0 || blocks > 0x7fffffff || (method != 1 && method != 2)) return hipErrorInvalidValue;
  if (method == 1) hipLaunchKernelGGL(k_prefix_pick<1>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(k_prefix_pick<2>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_prefix_null(const PrefixArgs& a, int method, hipStream_t stream) {
  if (a.nslots == 0 || a.K == 0) return hipSuccess;
  if (a.nblocks < 1 || (int64_t)a.nkt * a.nblocks > 0x7fffffff || a.W32p % kCtWC != 0 || a.nkt < 1 ||
      (int64_t)a.nkt * kCtPT > a.Kpad || (method != 1 && method != 2))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((int64_t)a.nkt * a.nblocks));
  if (g_launch_trace)
    fprintf(stderr, "launch k_prefix_null slots=%lld rows=%lld blocks=%d nkt=%d\n", (long long)a.nslots, (long long)a.nrows, a.nblocks, a.nkt);
  if (method == 1) hipLaunchKernelGGL((k_prefix_null<1, 4, 4>), grid, dim3(kCtBlock), 0, stream, a);
  else hipLaunchKernelGGL((k_prefix_null<2, 2, 4>), grid, dim3(kCtBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

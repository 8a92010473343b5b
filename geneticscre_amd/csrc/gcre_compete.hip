// gcre_compete.hip -- competitive tests of caller-given sets (gcre_score_sets_compete): every set against
// random sets of the same size drawn bin by bin from the caller's gene pool, scored on the OBSERVED labels.
//   * k_compete_null  one wave per (valid set, run of draws).  Phase 1: the picks of a draw in member order, by the rule of
//                     gcre_compete.h -- the candidate is wave-uniform, the earlier picks sit one per lane in NC registers
//                     and a candidate is held against all of them by NC compares and one ballot.  Phase 2: the OR of the
//                     picked gene rows over the patients, 16 bytes a lane so that a wave-load is a contiguous 1 KB of one
//                     row, eight rows' loads in flight; AND with the case / control bits (computed, not loaded), popcount,
//                     wave reduction, the look-up in the f64 table k_set_observed reads, in its order of the addition.
// No LDS; every global write is a vector store or a vector atomic.  The context-side entry is in gcre_host_compete.hip.
#include "gcre_count_tile.h"   // GCRE_CONSTANT, as_const, tri_index
#include "gcre_compete.h"

namespace gcre {
namespace {

// the low x bits set (x <= 0: none, x >= 32: all)
__device__ __forceinline__ u32 compete_below(int x) { return x <= 0 ? 0u : (x >= 32 ? 0xffffffffu : ((1u << x) - 1u)); }

__device__ __forceinline__ int compete_wave_sum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// GCRE_COMPETE_U / GCRE_COMPETE_WAVES: tools/build_variant.py, for A/B runs of tools/compete_time.py
#ifndef GCRE_COMPETE_U
#define GCRE_COMPETE_U 8
#endif
#ifdef GCRE_COMPETE_WAVES
#define COMPETE_WAVES __attribute__((amdgpu_waves_per_eu(GCRE_COMPETE_WAVES)))
#else
#define COMPETE_WAVES
#endif
constexpr int kCompeteBlock = 256;
constexpr int kCompeteU = GCRE_COMPETE_U;     // rows whose loads are in flight per lane

}  // namespace

// M method, NC picks per lane: sets of up to 64 NC members
template <int M, int NC>
__global__ __launch_bounds__(kCompeteBlock) COMPETE_WAVES void k_compete_null(const CompeteArgs a) {
  constexpr int U = kCompeteU;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 w = (i64)blockIdx.x * (kCompeteBlock / 64) + wave;
  if (w >= (i64)a.V * a.groups) return;   // wave-uniform; the kernel has no barrier
  const int v = (int)(w / a.groups);
  const int grp = (int)(w % a.groups);

  const CompeteSet GCRE_CONSTANT* SETS = as_const(a.sets);
  const int32_t GCRE_CONSTANT* POOL = as_const(a.pool_rows);
  const i64 set = SETS[v].set;
  const int moff = SETS[v].moff;
  const int k = SETS[v].k;
  const double obs = a.obs[v];

  // this lane's members: j = 64 c + lane.  Which of them are (-) is a wave-uniform 64-bit word per c.
  CompeteMemberDev mem[NC];
  u64 neg[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) {
    const int j = 64 * c + lane;
    mem[c] = j < k ? a.mem[moff + j] : CompeteMemberDev{-1, -1};
    const bool minus = M == 2 && a.signs && j < k && a.signs[moff + j] == -1;
    neg[c] = __ballot(minus);
  }

  const int ncc = (a.Wd + 255) / 256;          // column chunks of 256 dwords
  u32 ge = 0;
  const int b_lo = grp * a.dpw;
  const int b_hi = b_lo + a.dpw < a.nb ? b_lo + a.dpw : a.nb;
  for (int bi = b_lo; bi < b_hi; bi++) {
    // ---- phase 1: the picks ----
    const u64 base = gcre_compete::compete_base(a.seed, set, a.b0 + bi);
    int32_t pick[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) pick[c] = -1;   // never a candidate
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const int kc = k - 64 * c < 64 ? k - 64 * c : 64;
      for (int jj = 0; jj < kc; jj++) {
        const int off = __builtin_amdgcn_readlane(mem[c].off, jj);
        const int n = __builtin_amdgcn_readlane(mem[c].n, jj);
        int32_t got = n;                        // a fixed member stays itself
        if (off >= 0)
          got = gcre_compete::compete_pick(base, 64 * c + jj, POOL + off, n, a.attempts, [&](int32_t row) {
            bool hit = false;
#pragma unroll
            for (int q = 0; q < NC; q++) hit = hit || pick[q] == row;
            return __ballot(hit) != 0ull;
          });
        pick[c] = lane == jj ? got : pick[c];
      }
    }
    if (a.picks_out) {
      int32_t* out = a.picks_out + (size_t)bi * (size_t)a.tm + (size_t)moff;
#pragma unroll
      for (int c = 0; c < NC; c++)
        if (64 * c + lane < k) out[64 * c + lane] = pick[c];
    }

    // ---- phase 2: the unions over the patients, and their counts ----
    int cnt[2 * M];
#pragma unroll
    for (int h = 0; h < 2 * M; h++) cnt[h] = 0;
    for (int cc = 0; cc < ncc; cc++) {
      const int d0 = cc * 256 + lane * 4;       // this lane's four dwords of every row
      const bool live = d0 < a.Wd;
      const u32* col = a.rows + (live ? d0 : 0);
      u32x4 acc[M];
#pragma unroll
      for (int h = 0; h < M; h++) acc[h] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int c = 0; c < NC; c++) {
        const int kc = k - 64 * c < 64 ? k - 64 * c : 64;
        for (int jj = 0; jj < kc; jj += U) {
          u32x4 x[U];
#pragma unroll
          for (int u = 0; u < U; u++) {
            x[u] = u32x4{0u, 0u, 0u, 0u};
            if (jj + u < kc) {                  // wave-uniform
              const int row = __builtin_amdgcn_readlane(pick[c], jj + u);
              if (live && row >= 0) x[u] = *(const u32x4*)(col + (size_t)row * (size_t)a.Wd);   // (a pick is never negative: 2k <= N)
            }
          }
#pragma unroll
          for (int u = 0; u < U; u++) {
            if constexpr (M == 1) {
              acc[0] |= x[u];
            } else {
              const bool minus = (neg[c] >> ((jj + u) & 63)) & 1ull;   // wave-uniform; beyond kc x is zero
              if (minus) acc[1] |= x[u];
              else acc[0] |= x[u];
            }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int p0 = 32 * (d0 + i);           // the first patient of the dword
        const u32 cases = compete_below(a.n_cases - p0), all = compete_below(a.n - p0);
#pragma unroll
        for (int h = 0; h < M; h++) {
          cnt[2 * h] += __builtin_popcount(acc[h][i] & cases);
          cnt[2 * h + 1] += __builtin_popcount(acc[h][i] & all & ~cases);
        }
      }
    }
#pragma unroll
    for (int h = 0; h < 2 * M; h++) cnt[h] = compete_wave_sum(cnt[h]);

    // ---- the null score: k_set_observed's expression on (cases, controls) of P and (controls, cases) of N ----
    double score = a.dvt[tri_index((u64)cnt[0] + (u64)cnt[1]) + (u64)cnt[0]];
    if constexpr (M == 2) score = score + a.dvt[tri_index((u64)cnt[3] + (u64)cnt[2]) + (u64)cnt[3]];
    ge += score >= obs ? 1u : 0u;               // a NaN on either side never counts
    if (a.null_out && lane == 0) a.null_out[(size_t)v * (size_t)a.stride + (size_t)bi] = score;
  }
  if (lane == 0 && ge != 0u) atomicAdd(a.n_ge + v, (unsigned long long)ge);
}

hipError_t launch_compete_null(const CompeteArgs& a, int method, hipStream_t stream) {
  if (a.V == 0 || a.nb == 0) return hipSuccess;
  const int64_t waves = (int64_t)a.V * a.groups;
  const int64_t blocks = (waves + kCompeteBlock / 64 - 1) / (kCompeteBlock / 64);
  if (blocks > 0x7fffffff || a.Wd % 4 != 0 || a.maxk > 1024 || a.dpw < 1 || (int64_t)a.groups * a.dpw < a.nb) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(kCompeteBlock);
  if (g_launch_trace) fprintf(stderr, "launch k_compete_null sets=%d draws=%d dpw=%d maxk=%d\n", a.V, a.nb, a.dpw, a.maxk);
#define COMPETE_LAUNCH(M, NC) hipLaunchKernelGGL((k_compete_null<M, NC>), grid, block, 0, stream, a)
  if (method == 1) {
    if (a.maxk <= 64) COMPETE_LAUNCH(1, 1);
    else if (a.maxk <= 256) COMPETE_LAUNCH(1, 4);
    else COMPETE_LAUNCH(1, 16);
  } else {
    if (a.maxk <= 64) COMPETE_LAUNCH(2, 1);
    else if (a.maxk <= 256) COMPETE_LAUNCH(2, 4);
    else COMPETE_LAUNCH(2, 16);
  }
#undef COMPETE_LAUNCH
  return hipGetLastError();
}

}  // namespace gcre

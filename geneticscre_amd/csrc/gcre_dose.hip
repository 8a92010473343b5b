// gcre_dose.hip -- multi-hit tests of caller-given sets: the patients who carry at least m of a set's members, for the
// caller's levels m, with the maximum over the levels taken under every permutation (gcre_score_sets_dose).
//   * k_dose_rows  per set: a bit-sliced count, per patient, of the set's members the patient carries; per level m the row
//                  "count >= m", written in k_set_null's row layout, and the counts SetUnion::build (gcre_setlists.h) gives
//                  such a row
// The level rows are scored by k_set_observed (gcre_sets.hip) and walked by k_prefix_pick and k_prefix_null
// (gcre_prefix.hip), which do not care how the rows of a slot were made.  The context-side entry is in gcre_host_steps.hip,
// the argument checks in gcre_dose.h.
//
// k_dose_rows is k_prefix_rows' mapping: one wave per (slot, 64-dword stretch of the row), one lane per dword, 32 patients
// per lane.  Per half a lane holds four count planes and a sticky plane: bit q of plane b is bit b of patient q's count, and
// a carry out of plane 3 sets the patient's sticky bit, so a patient with 16 or more carried members stays at or above every
// level.  The member loads do not depend on the counter: kDoseFly of them are issued before the first is added.  Every global
// write is a vector store or a vector atomic.
#include "gcre_count_tile.h"   // GCRE_CONSTANT, as_const

namespace gcre {
namespace {

constexpr int kDoseBlock = 256;   // threads per block: four waves
constexpr int kDoseFly = 8;       // member rows whose loads are in flight per lane

// One half's count of 32 patients: planes c[0] (ones) .. c[3] (eights), and the patients that passed 15
struct DoseCounter {
  u32 c[4];
  u32 sticky;
  __device__ __forceinline__ void clear() {
    c[0] = c[1] = c[2] = c[3] = 0u;
    sticky = 0u;
  }
  // count += 1 for the patients of x: a ripple through the planes
  __device__ __forceinline__ void add(u32 x) {
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const u32 t = c[b] & x;
      c[b] ^= x;
      x = t;
    }
    sticky |= x;
  }
  // the patients with count >= m, 1 <= m <= 15 (wave-uniform): greater / equal so far from the top plane down
  __device__ __forceinline__ u32 at_least(int m) const {
    u32 gt = 0u, eq = 0xffffffffu;
#pragma unroll
    for (int b = 3; b >= 0; b--) {
      const u32 mb = 0u - (u32)((m >> b) & 1);   // all ones where bit b of m is set
      gt |= eq & c[b] & ~mb;                     // equal above, 1 against 0 here
      eq &= ~(c[b] ^ mb);                        // still equal
    }
    return sticky | gt | eq;
  }
};

}  // namespace

template <int M>
__global__ __launch_bounds__(kDoseBlock) void k_dose_rows(const DoseArgs a) {
  constexpr int U = kDoseFly;
  const int nch = (a.W32p + 63) / 64;   // 64-dword stretches of a row: one wave each
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 wv = (i64)blockIdx.x * (kDoseBlock / 64) + wave;
  const i64 e = wv / nch;
  const int lane = threadIdx.x & 63;
  if (e >= a.nslots) return;   // the whole wave; the kernel has no barrier
  const i64 s = as_const(a.which)[e];
  const i64 sb = as_const(a.set_off)[s], se = as_const(a.set_off)[s + 1];
  const int32_t GCRE_CONSTANT* MEM = as_const(a.members);
  const int32_t GCRE_CONSTANT* SGN = as_const(a.signs);
  const int split = a.n_cases >> 5;
  const u32 split_mask = (1u << (a.n_cases & 31)) - 1u;
  const size_t rs = (size_t)M * a.W32p;

  const int w = (int)(wv % nch) * 64 + lane;
  const bool in_row = w < a.W32p;
  const bool has = in_row && w < a.W2 && w * 32 < a.n_patients;
  const int left = a.n_patients - w * 32;   // patients from this dword on
  const u32 keep = has ? (left < 32 ? (1u << left) - 1u : 0xffffffffu) : 0u;
  const u32 cm = w < split ? 0xffffffffu : w == split ? split_mask : 0u;
  const u32* col = a.gene_rows + (has ? w : 0);

  DoseCounter cp, cn;
  cp.clear();
  cn.clear();
  for (i64 i = sb; i < se; i += U) {
    // the loads of up to U members first, the tail of the set masked (wave-uniform), then the adds
    u32 x[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      x[u] = 0u;
      if (i + u < se) {
        const i64 row = MEM[i + u];
        if (has) x[u] = col[row * a.W2];
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      if (i + u >= se) continue;   // wave-uniform
      const u32 v = x[u] & keep;
      if constexpr (M == 2) {
        const bool minus = a.signs && SGN[i + u] == -1;   // wave-uniform
        if (minus) cn.add(v);
        else cp.add(v);
      } else {
        cp.add(v);
      }
    }
  }

  // per level its dword of the level row and the row's counts: a wave reduction, then one 32-bit vector atomic per count,
  // which the waves of the row's other stretches add to as well
  const i64 r0 = e * a.n_levels;
  for (int l = 0; l < a.n_levels; l++) {
    const int m = (int)((a.levels >> (4 * l)) & 15u);   // wave-uniform
    const u32 P = cp.at_least(m);
    const u32 N = M == 2 ? cn.at_least(m) : 0u;
    const i64 row = r0 + l;
    if (in_row) {
      u32* out = a.rows + (size_t)row * rs;
      out[w] = P;   // lanes without patients hold empty counters: the pad dwords are written as zero
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
  }
}

// one wave per slot and 64-dword stretch of a row; a grid that does not fit is refused, never clamped
hipError_t launch_dose_rows(const DoseArgs& a, int method, hipStream_t stream) {
  if (a.nslots == 0) return hipSuccess;
  if (a.nslots < 0 || a.W2 < 1 || a.W32p < a.W2 || a.n_levels < 1 || a.n_levels > 15 || (method != 1 && method != 2))
    return hipErrorInvalidValue;
  if (a.nslots > 0x7fffffffffffll / ((a.W32p + 63) / 64)) return hipErrorInvalidValue;
  const i64 waves = a.nslots * ((a.W32p + 63) / 64);
  const i64 blocks = (waves + kDoseBlock / 64 - 1) / (kDoseBlock / 64);
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  if (g_launch_trace)
    fprintf(stderr, "launch k_dose_rows slots=%lld levels=%d\n", (long long)a.nslots, a.n_levels);
  if (method == 1) hipLaunchKernelGGL(k_dose_rows<1>, dim3((unsigned)blocks), dim3(kDoseBlock), 0, stream, a);
  else hipLaunchKernelGGL(k_dose_rows<2>, dim3((unsigned)blocks), dim3(kDoseBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

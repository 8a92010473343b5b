// gcre_given.hip -- residual union rows for conditional set scores (gcre_score_sets_given).
//   * k_set_residual  per (set, given set) pair: the set's (+) and (-) unions with every carrier of the given set taken
//                     out, written in k_set_null's row layout, and the counts SetUnion::build (gcre_setlists.h) gives
// The rows are scored by the kernels of gcre_sets.hip in later launches on the same stream; the context-side entry is in
// gcre_host_sets.hip.
//
// k_clump_union's mapping (gcre_clump.hip): one wave per entry, lanes stride over the dwords of a row, every member's
// dword is one coalesced vector load.  The set list is read as the caller gave it (CSR), so a lane walks the members of
// both sets once per dword it owns.  Vector loads and stores only; no LDS, no atomics.
#include "gcre_kernels.h"

namespace gcre {
namespace {

typedef uint32_t u32;
typedef int64_t i64;

constexpr int kResBlock = 256;   // four waves, one entry each

}  // namespace

template <int M>
__global__ __launch_bounds__(kResBlock) void k_set_residual(const SetResidualArgs a) {
  const i64 e = (i64)blockIdx.x * (kResBlock / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (e >= a.n) return;   // the whole wave
  const i64 s = a.which[e], g = a.given[e];
  const i64 sb = a.set_off[s], se = a.set_off[s + 1];
  const i64 gb = g >= 0 ? a.set_off[g] : 0, ge = g >= 0 ? a.set_off[g + 1] : 0;
  const int split = a.n_cases >> 5;
  const u32 split_mask = (1u << (a.n_cases & 31)) - 1u;
  u32* out = a.out + e * (i64)(M * a.W32p);
  u32 k0 = 0, k1 = 0, k2 = 0, k3 = 0;
  for (int w = lane; w < a.W32p; w += 64) {
    u32 P = 0, N = 0;
    if (w < a.W2 && w * 32 < a.n_patients) {
      for (i64 i = sb; i < se; i++) {
        const u32 x = a.rows[(i64)a.members[i] * a.W2 + w];
        if (M == 2 && a.signs && a.signs[i] == -1) N |= x;
        else P |= x;
      }
      u32 C = 0;   // the given set's carriers: all its members, whatever their signs
      for (i64 i = gb; i < ge; i++) C |= a.rows[(i64)a.members[i] * a.W2 + w];
      const int left = a.n_patients - w * 32;   // patients from this dword on
      const u32 keep = ~C & (left < 32 ? (1u << left) - 1u : 0xffffffffu);
      P &= keep;
      N &= keep;
    }
    out[w] = P;
    if (M == 2) out[a.W32p + w] = N;
    const u32 cm = w < split ? 0xffffffffu : w == split ? split_mask : 0u;
    k0 += __popc(P & cm);    // cases_pos
    k1 += __popc(P & ~cm);   // ctrls_pos
    k2 += __popc(N & ~cm);   // cases_neg: the (-) half counts the other way round (SetUnion::build)
    k3 += __popc(N & cm);    // ctrls_neg
  }
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
    int4 k;
    k.x = (int)k0;
    k.y = (int)k1;
    k.z = (int)k2;
    k.w = (int)k3;
    *(int4*)(a.cnt + e * 4) = k;
    a.tot[e * M] = k0 + k1;
    if (M == 2) a.tot[e * M + 1] = k2 + k3;
  }
}

// one wave per entry; a grid that does not fit is refused, never clamped
hipError_t launch_set_residual(const SetResidualArgs& a, int method, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  const i64 blocks = (a.n + kResBlock / 64 - 1) / (kResBlock / 64);
  if (a.n < 0 || blocks > 0x7fffffff || a.W2 < 1 || a.W32p < a.W2 || (method != 1 && method != 2)) return hipErrorInvalidValue;
  if (g_launch_trace) fprintf(stderr, "launch k_set_residual entries=%lld blocks=%lld\n", (long long)a.n, (long long)blocks);
  if (method == 1) hipLaunchKernelGGL(k_set_residual<1>, dim3((unsigned)blocks), dim3(kResBlock), 0, stream, a);
  else hipLaunchKernelGGL(k_set_residual<2>, dim3((unsigned)blocks), dim3(kResBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

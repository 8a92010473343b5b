// gcre_seq_weighted.hip -- one batch of covariate-adjusted masks for the sequential p-values
// (gcre_score_sets_sequential_weighted): permutations [r0, r0 + nb) of gcre_generate_weighted_masks' rule in
// the layout k_seq_null reads, never resident beyond the batch.  The law, the thresholds and the draw are gcre_weighted.h's
// (wt_*), which batch columns are written is gcre_seq_weighted.h's; here are the two phases of gcre_weighted.hip again, for a
// batch column i with the permutation r = r0 + i as 64 bits.
//   * k_seq_weighted_search   one wave per (batch column i, stratum s): k_weighted_search's pass -- lanes stride over the
//                             stratum's patient list, kWeightedBatch attempts per pass in registers, four wt_mix64 per patient,
//                             a wave reduction, the first exact hit in attempt order.  a*(r, s) leaves as one dword of the
//                             batch-local att[s][i]; a pair that meets the cap leaves kWeightedNone there and takes part in a
//                             32-bit atomicMin on the batch's first left-over column.  No mask bit is written.
//   * k_seq_weighted_write    a lane per batch column, k_weighted_write's walk: the hash key of the accepted attempt of every
//                             stratum in the lane's own LDS column, the patients in column order, a dword every 32 patients
//                             into masks[word * stride + i]; rows up to W32p and columns nb .. stride-1 zero, as k_seq_masks
//                             leaves them.  Launched on the columns in front of the first left-over one only: every attempt
//                             it reads was accepted.
// Every global write is a vector store or a 32-bit vector atomic in plain C++.
#include "gcre_kernels.h"
#include "gcre_seq_weighted.h"

namespace gcre {

using namespace gcre_weighted;

namespace {
constexpr int kSwSearchBlock = 256;   // four waves: four (i, s) pairs of one stratum, but for the block on a stratum's edge
}  // namespace

__global__ __launch_bounds__(kSwSearchBlock) void k_seq_weighted_search(const SeqWeightedArgs a) {
  constexpr int B = kWeightedBatch;
  static_assert(B == 8, "four hashes, two attempts each");
  const uint32_t lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * (kSwSearchBlock / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= (long long)a.nb * a.S) return;   // (the whole wave)
  const uint32_t s = (uint32_t)(w / a.nb), i = (uint32_t)(w % a.nb);
  const uint32_t off = a.soff[s], size = a.soff[s + 1] - off, need = a.cases_in[s];
  const int32_t* cols = a.cols + off;
  const uint32_t* cthr = a.cthr + off;
  const uint64_t base = wt_base(wt_key(a.seed1, a.r0 + (uint64_t)i), s);

  uint32_t found = kWeightedNone;
  for (uint32_t a0 = 0; a0 < a.cap; a0 += B) {   // cap <= 2^31: a0 + B does not wrap
    uint64_t pair[B / 2];
#pragma unroll
    for (int j = 0; j < B / 2; j++) pair[j] = wt_pair(base, (a0 >> 1) + (uint32_t)j);
    uint32_t cnt[B];
#pragma unroll
    for (int k = 0; k < B; k++) cnt[k] = 0;
    for (uint32_t p = lane; p < size; p += 64) {
      const uint32_t c = (uint32_t)cols[p], t = cthr[p];
#pragma unroll
      for (int j = 0; j < B / 2; j++) {
        const uint64_t u = wt_draw(pair[j], c);
        cnt[2 * j] += (uint32_t)(u >> 32) < t ? 1u : 0u;
        cnt[2 * j + 1] += (uint32_t)u < t ? 1u : 0u;
      }
    }
#pragma unroll
    for (int k = 0; k < B; k++) {
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) cnt[k] += (uint32_t)__shfl_xor((int)cnt[k], m, 64);
    }
    // every lane holds the eight totals: the first exact hit in attempt order, below the cap
#pragma unroll
    for (int k = B - 1; k >= 0; k--)
      if (cnt[k] == need && a0 + (uint32_t)k < a.cap) found = a0 + (uint32_t)k;
    if (found != kWeightedNone) break;
  }
  if (lane == 0) {
    a.att[(size_t)s * (size_t)a.att_stride + i] = found;
    if (found == kWeightedNone) atomicMin(a.first, i);
  }
}

__global__ __launch_bounds__(64) void k_seq_weighted_write(const SeqWeightedArgs a) {
  __shared__ uint64_t pair_of[kWeightedStrataMax][64];
  __shared__ uint32_t shift_of[kWeightedStrataMax][64];
  const int lane = threadIdx.x;
  const int i = blockIdx.x * 64 + lane;
  if (i >= a.stride) return;
  const size_t S = (size_t)a.stride;
  if (i >= a.nb) {
    for (int k = 0; k < a.W32p; k++) a.masks[(size_t)k * S + i] = 0u;
    return;
  }
  const uint64_t key = wt_key(a.seed1, a.r0 + (uint64_t)i);
  // (a lane reads back only what it wrote itself: no barrier)
  for (int s = 0; s < a.S; s++) {
    const uint32_t at = a.att[(size_t)s * (size_t)a.att_stride + i];
    pair_of[s][lane] = wt_pair(wt_base(key, (uint32_t)s), at >> 1);
    shift_of[s][lane] = (at & 1u) ? 0u : 32u;   // odd attempt: the low half
  }
  uint32_t word = 0;
  for (int c = 0; c < a.n; c++) {
    const int s = a.stratum ? a.stratum[c] : 0;
    const uint32_t t = a.thr[c];
    const uint64_t u = wt_draw(pair_of[s][lane], (uint32_t)c);
    if ((uint32_t)(u >> shift_of[s][lane]) < t) word |= 1u << (c & 31);
    if ((c & 31) == 31 || c == a.n - 1) {
      a.masks[(size_t)(c >> 5) * S + i] = word;
      word = 0;
    }
  }
  for (int k = (a.n + 31) >> 5; k < a.W32p; k++) a.masks[(size_t)k * S + i] = 0u;
}

hipError_t launch_seq_weighted_search(const SeqWeightedArgs& a, hipStream_t stream) {
  const long long waves = (long long)a.nb * a.S;
  if (waves == 0) return hipSuccess;
  const long long blocks = (waves + kSwSearchBlock / 64 - 1) / (kSwSearchBlock / 64);
  if (blocks > 0x7fffffffll || a.nb < 0 || a.nb > a.att_stride || a.S < 1 || a.S > kWeightedStrataMax || a.cap < 1u || !a.cols || !a.cthr ||
      !a.soff || !a.cases_in || !a.att || !a.first)
    return hipErrorInvalidValue;
  if (g_launch_trace) fprintf(stderr, "launch k_seq_weighted_search perms=%d strata=%d\n", a.nb, a.S);
  hipLaunchKernelGGL(k_seq_weighted_search, dim3((unsigned)blocks), dim3(kSwSearchBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_seq_weighted_write(const SeqWeightedArgs& a, hipStream_t stream) {
  if (a.stride == 0) return hipSuccess;
  if (a.stride % 64 != 0 || a.nb < 0 || a.nb > a.stride || a.nb > a.att_stride || a.n < 1 || (a.n + 31) / 32 > a.W32p || a.S < 1 ||
      a.S > kWeightedStrataMax || !a.att || !a.thr || !a.masks || (a.S > 1 && !a.stratum))
    return hipErrorInvalidValue;
  if (g_launch_trace) fprintf(stderr, "launch k_seq_weighted_write perms=%d of %d strata=%d\n", a.nb, a.stride, a.S);
  hipLaunchKernelGGL(k_seq_weighted_write, dim3((unsigned)(a.stride / 64)), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

// gcre_weighted.hip -- covariate-adjusted permutation masks: case labels drawn with per-patient odds, conditional on the
// number of cases of every stratum (gcre_generate_weighted_masks).  The law, the thresholds and the draw rule
// are gcre_weighted.h's; here are the two phases, because the search wants a wave per mask and the stores want a lane per mask.
//   * k_weighted_search   one wave per (permutation r, stratum s): lanes stride over the stratum's patient list (columns and
//                         thresholds contiguous per stratum; the hash reads the patient's COLUMN, so the layout cannot leak
//                         into the result), kWeightedBatch attempts per pass in registers -- one threshold load and four
//                         gcre_mix64 per patient feed eight counters per lane -- then a wave reduction and the first exact hit
//                         in attempt order.  a*(r, s) leaves as one dword; a pair that meets the cap leaves kWeightedNone and
//                         adds one to the failure counter.  No mask bit is written.
//   * k_weighted_write    k_generate_masks' shape, a lane per permutation: the lane keeps the hash key of its accepted attempt
//                         of every stratum in LDS (its own column of a [16][64] array: no dynamic register index, no
//                         barrier), walks the patients in column order, recomputes the bit and stores a dword every 32
//                         patients into masks[word * Kpad + r]; zeros up to W32p.
// Every global write is a vector store or a 32-bit vector atomic in plain C++.
#include "gcre_kernels.h"
#include "gcre_weighted.h"

namespace gcre {

using namespace gcre_weighted;

namespace {
constexpr int kWtSearchBlock = 256;   // four waves: four (r, s) pairs of one stratum
}  // namespace

__global__ __launch_bounds__(kWtSearchBlock) void k_weighted_search(const WeightedArgs a) {
  constexpr int B = kWeightedBatch;
  static_assert(B == 8, "four hashes, two attempts each");
  const uint32_t lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * (kWtSearchBlock / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= (long long)a.K * a.S) return;   // (the whole wave)
  const uint32_t s = (uint32_t)(w / a.K), r = (uint32_t)(w % a.K);
  const uint32_t off = a.soff[s], size = a.soff[s + 1] - off, need = a.cases_in[s];
  const int32_t* cols = a.cols + off;
  const uint32_t* cthr = a.cthr + off;
  const uint64_t base = wt_base(wt_key(a.seed1, r), s);

  uint32_t found = kWeightedNone;
  for (uint32_t a0 = 0; a0 < a.cap; a0 += B) {   // cap <= 2^31: a0 + B does not wrap
    uint64_t pair[B / 2];
#pragma unroll
    for (int j = 0; j < B / 2; j++) pair[j] = wt_pair(base, (a0 >> 1) + (uint32_t)j);
    uint32_t cnt[B];
#pragma unroll
    for (int k = 0; k < B; k++) cnt[k] = 0;
    for (uint32_t i = lane; i < size; i += 64) {
      const uint32_t c = (uint32_t)cols[i], t = cthr[i];
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
    a.att[(size_t)s * a.K + r] = found;
    if (found == kWeightedNone) atomicAdd(a.left, 1u);
  }
}

__global__ __launch_bounds__(64) void k_weighted_write(const WeightedArgs a) {
  __shared__ uint64_t pair_of[kWeightedStrataMax][64];
  __shared__ uint32_t shift_of[kWeightedStrataMax][64];
  const int lane = threadIdx.x;
  const int r = blockIdx.x * 64 + lane;
  if (r >= a.K) return;
  const uint64_t key = wt_key(a.seed1, (uint64_t)r);
  // (a lane reads back only what it wrote itself: no barrier)
  for (int s = 0; s < a.S; s++) {
    const uint32_t at = a.att[(size_t)s * a.K + r];
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
      a.masks[(size_t)(c >> 5) * a.Kpad + r] = word;
      word = 0;
    }
  }
  for (int k = (a.n + 31) >> 5; k < a.W32p; k++) a.masks[(size_t)k * a.Kpad + r] = 0;
}

hipError_t launch_weighted_search(const WeightedArgs& a, hipStream_t stream) {
  const long long waves = (long long)a.K * a.S;
  if (waves == 0) return hipSuccess;
  const long long blocks = (waves + kWtSearchBlock / 64 - 1) / (kWtSearchBlock / 64);
  if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_weighted_search, dim3((unsigned)blocks), dim3(kWtSearchBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_weighted_write(const WeightedArgs& a, hipStream_t stream) {
  if (a.K == 0) return hipSuccess;
  hipLaunchKernelGGL(k_weighted_write, dim3((a.K + 63) / 64), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

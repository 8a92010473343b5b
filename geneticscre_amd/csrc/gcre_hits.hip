// gcre_hits.hip -- hit lists (gcre_hits): every joined path of a join whose observed score reaches a
// cut-off, not only the top K.  Like the gene tally and k_exceed_observed it reads what a chunk's inspector left on the
// device -- score key, operand rows, cases, controls of every joined path -- before the next chunk overwrites it.
//   * k_hits_collect   a stream compaction over a chunk's scored paths: the records of the paths whose key is at or above
//                      the threshold key are appended to the list's struct-of-arrays, 32 B per record
// Keys are compared, never doubles: score_key (gcre_kernels.hip) is monotone in the score, 0 = not a score (-inf, NaN);
// the host makes the threshold key so that a cut-off of either zero admits both zeros (the key of -0.0) and -inf admits
// every score (key 1).  The record keeps the path's OWN key: -0.0 reads back with its sign.
//
// A wave walks whole groups of 64 consecutive paths.  A group in which no lane passes -- at a family-wise cut-off almost
// every group -- costs its key load and one vote.  Otherwise ONE lane of the wave reserves room for all the passing lanes
// (the popcount of the vote added to the list's 64-bit cursor, relaxed, agent scope) and broadcasts the base; a passing
// lane's slot is the base plus its rank among the passing lanes, and it writes its record when the slot is inside the
// capacity.  The cursor keeps counting past the capacity: the number found is exact even when the list overflows.  The
// order of the records in the list depends on which wave reserved first; the host sorts them (gcre_hits_read).
// Every global write is a vector store or a vector atomic.
#include "gcre_kernels.h"

namespace gcre {
namespace {

typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;

constexpr int kHitsBlock = 256;
constexpr int kHitsBlocksPerCu = 8;

__global__ __launch_bounds__(kHitsBlock) void k_hits_collect(const HitsArgs a) {
  const int lane = threadIdx.x & 63;
  const i64 stride = (i64)gridDim.x * kHitsBlock;
  // whole groups of 64 consecutive paths: the trip count is the same for all lanes of a wave (the votes need them all)
  for (i64 base = (i64)blockIdx.x * kHitsBlock + (threadIdx.x & ~63); base < a.count; base += stride) {
    const i64 i = base + lane;
    const u64 key = i < a.count ? a.key[i] : 0;
    const bool pass = key != 0 && key >= a.tkey;   // (0: not a score)
    const u64 vote = __ballot(pass);
    if (vote == 0) continue;   // (wave-uniform)
    const int leader = __ffsll((unsigned long long)vote) - 1;
    u64 slot = 0;
    if (lane == leader)
      slot = __hip_atomic_fetch_add(a.cursor, (unsigned long long)__popcll(vote), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    slot = __shfl(slot, leader, 64);
    slot += __builtin_amdgcn_mbcnt_hi((u32)(vote >> 32), __builtin_amdgcn_mbcnt_lo((u32)vote, 0u));
    if (pass && slot < (u64)a.cap) {
      a.ord[slot] = a.first + i;
      a.hkey[slot] = key;
      a.src[slot] = (int32_t)a.row0[i];
      a.trg[slot] = (int32_t)(a.row1[i] & 0x7fffffffu);   // (bit 31: the signed method's half swap)
      a.hcases[slot] = (int32_t)a.cases[i];
      a.hctrls[slot] = (int32_t)a.ctrls[i];
    }
  }
}

}  // namespace

hipError_t launch_hits_collect(const HitsArgs& a, int cus, hipStream_t stream) {
  if (a.count <= 0) return hipSuccess;
  if (a.cap < 1 || !a.cursor) return hipErrorInvalidValue;
  const i64 want = (a.count + kHitsBlock - 1) / kHitsBlock;
  const int grid = (int)(want < (i64)cus * kHitsBlocksPerCu ? want : (i64)cus * kHitsBlocksPerCu);
  trace_launch("k_hits_collect", want, grid);
  hipLaunchKernelGGL(k_hits_collect, dim3(grid), dim3(kHitsBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

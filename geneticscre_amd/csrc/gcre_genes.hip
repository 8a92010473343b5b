// gcre_genes.hip -- the per-gene best-path tally (gcre_gene_tally): for every gene slot the joined path
// through it with the largest observed score, ties to the smallest joined-path ordinal.  It reads what a chunk's
// inspector left on the device -- score key, operand rows, cases, controls of every joined path -- and nothing else.
//   * k_gene_fold   per joined path: the chunk's largest key of every slot the path touches (chunk-local table)
//   * k_gene_index  per joined path: the smallest in-chunk index among the paths whose key IS the slot's chunk best
//   * k_gene_merge  per slot: the chunk's entry into the join's table under "(key greater) or (key equal and ordinal
//                   smaller)", and the chunk-local tables back to empty
// Keys are compared, never doubles: score_key (gcre_kernels.hip) is monotone in the score, 0 = not a score (-inf, NaN).
// The one pair of equal scores under two keys, -0.0 and +0.0, is compared as the key of +0.0 (tie_key); the tables' entry
// of a slot is the winning path's OWN key, so the score read back has its sign.
// The merge rule is a total order on (key, ordinal), so the table does not depend on how the join was cut into chunks,
// on the order they arrive in, or on a chunk being folded twice.
//
// Contention (20,000 slots, hubs on millions of paths): an atomic is issued only by a path whose key beats what a plain
// look at the slot shows, and then a second look past the CU's cache -- after the first wave front almost none does -- and
// the lanes of a wave that pass for the same slot (the genes a path has from its paths0 row are wave-uniform for long
// runs: ordinals walk the paths1 rows of one paths0 row) are reduced in the wave first: one atomic per slot and wave.  A
// path whose key is below the slot's entry in the JOIN's table cannot win either and is dropped by the same look.  Every
// global write is a vector store or a vector atomic.
#include "gcre_kernels.h"

namespace gcre {
namespace {

typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;

constexpr int kGeneBlock = 256;
constexpr int kGeneBlocksPerCu = 8;
constexpr u32 kNoIndex = 0xffffffffu;

// a look at a slot that other waves are writing: past the CU's vector cache, or a stale line would keep every path of
// the CU passing the test
__device__ __forceinline__ u64 peek(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u32 peek(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ u64 tie_key(u64 k) { return k == kKeyMinusZero ? kKeyPlusZero : k; }

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// One slot column of a wave's 64 paths.  Every lane of the wave calls it (pass false: nothing to fold for this lane).
__device__ __forceinline__ void fold_slot(const GeneFoldArgs& a, int slot, u64 key, bool pass, int lane) {
  // the look that let the lane pass may have been at a stale line of the CU's cache: look again, past it
  if (pass) pass = key > peek(a.ck + slot);
  u64 todo = __ballot(pass);
  while (todo) {   // (wave-uniform: one round per distinct slot among the passing lanes)
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const int s = __shfl(slot, leader, 64);
    const bool same = pass && slot == s;
    const u64 m = wave_max(same ? key : 0);
    if (lane == leader) atomicMax((unsigned long long*)(a.ck + s), (unsigned long long)m);
    todo &= ~__ballot(same);
  }
}

// PRIOR: the join's table holds entries of earlier chunks (a path below a slot's entry there cannot win it)
template <bool PRIOR>
__global__ __launch_bounds__(kGeneBlock) void k_gene_fold(const GeneFoldArgs a) {
  const int lane = threadIdx.x & 63;
  const i64 stride = (i64)gridDim.x * kGeneBlock;
  // a wave walks whole groups of 64 consecutive paths: the trip count is the same for all of its lanes
  for (i64 base = (i64)blockIdx.x * kGeneBlock + (threadIdx.x & ~63); base < a.count; base += stride) {
    const i64 i = base + lane;
    bool valid = i < a.count;
    const u64 key = valid ? tie_key(a.key[i]) : 0;     // (the chunk-local table holds tie keys)
    valid = valid && key != 0;
    const i64 r0 = valid ? (i64)a.row0[i] : 0;
    const i64 r1 = valid ? (i64)(a.row1[i] & 0x7fffffffu) : 0;   // (bit 31: the signed method's half swap)
    // every slot of the path, then every slot's current best, as loads that do not wait for one another (the wave-wide
    // votes below would otherwise put a round trip to the L2 between any two of them); a lane without a slot reads slot 0
    int slot[2 * kGeneWidthMax];
    bool pass[2 * kGeneWidthMax];
#pragma unroll
    for (int s = 0; s < kGeneWidthMax; s++) {
      slot[s] = (s < a.w0 && valid) ? a.genes0[r0 * a.w0 + s] : -1;
      slot[kGeneWidthMax + s] = (s < a.w1 && valid) ? a.genes1[r1 * a.w1 + s] : -1;
    }
    u64 seen[2 * kGeneWidthMax];
#pragma unroll
    for (int s = 0; s < 2 * kGeneWidthMax; s++) {
      const int g = slot[s] < 0 ? 0 : slot[s];
      u64 v = a.ck[g];
      if (PRIOR) {
        const u64 b = tie_key(a.bkey[g]);
        v = (b > v && b > key) ? ~0ull : v;   // (an equal key may still win on the ordinal)
      }
      seen[s] = v;
    }
#pragma unroll
    for (int s = 0; s < 2 * kGeneWidthMax; s++) pass[s] = slot[s] >= 0 && key > seen[s];
    u64 any = 0;
#pragma unroll
    for (int s = 0; s < 2 * kGeneWidthMax; s++) any |= __ballot(pass[s]) ? (1ull << s) : 0;
#pragma unroll
    for (int s = 0; s < 2 * kGeneWidthMax; s++)
      if (any & (1ull << s)) fold_slot(a, slot[s], key, pass[s], lane);
  }
}

// the in-chunk index of a slot's best path: only paths whose key equals the chunk best (final: k_gene_fold is done) ask
__device__ __forceinline__ void index_slot(const GeneFoldArgs& a, int slot, u64 key, u32 i) {
  if (slot < 0 || key != a.ck[slot]) return;
  if (i < peek(a.cidx + slot)) atomicMin(a.cidx + slot, i);
}

__global__ __launch_bounds__(kGeneBlock) void k_gene_index(const GeneFoldArgs a) {
  const i64 stride = (i64)gridDim.x * kGeneBlock;
  for (i64 i = (i64)blockIdx.x * kGeneBlock + threadIdx.x; i < a.count; i += stride) {
    const u64 key = tie_key(a.key[i]);
    if (key == 0) continue;
    const i64 r0 = (i64)a.row0[i];
    const i64 r1 = (i64)(a.row1[i] & 0x7fffffffu);
#pragma unroll
    for (int s = 0; s < kGeneWidthMax; s++)
      if (s < a.w0) index_slot(a, a.genes0[r0 * a.w0 + s], key, (u32)i);
#pragma unroll
    for (int s = 0; s < kGeneWidthMax; s++)
      if (s < a.w1) index_slot(a, a.genes1[r1 * a.w1 + s], key, (u32)i);
  }
}

__global__ __launch_bounds__(kGeneBlock) void k_gene_merge(const GeneFoldArgs a) {
  const int g = blockIdx.x * kGeneBlock + threadIdx.x;
  if (g >= a.n_slots) return;
  const u64 k = a.ck[g];
  if (k == 0) return;   // (no path of the chunk could win the slot: cidx was not touched either)
  const u32 i = a.cidx[g];
  a.ck[g] = 0;
  a.cidx[g] = kNoIndex;
  const i64 ord = a.first + (i64)i;
  const u64 bk = tie_key(a.bkey[g]);
  if (k > bk || (k == bk && ord < a.bord[g])) {
    a.bkey[g] = a.key[i];
    a.bord[g] = ord;
    a.bsrc[g] = (int32_t)a.row0[i];
    a.btrg[g] = (int32_t)(a.row1[i] & 0x7fffffffu);
    a.bcases[g] = (int32_t)a.cases[i];
    a.bctrls[g] = (int32_t)a.ctrls[i];
  }
}

}  // namespace

hipError_t launch_gene_fold(const GeneFoldArgs& a, int cus, hipStream_t stream) {
  if (a.count <= 0 || a.n_slots <= 0) return hipSuccess;
  const i64 want = (a.count + kGeneBlock - 1) / kGeneBlock;
  const int grid = (int)(want < (i64)cus * kGeneBlocksPerCu ? want : (i64)cus * kGeneBlocksPerCu);
  trace_launch("k_gene_fold", want, grid);
  if (a.prior) hipLaunchKernelGGL(k_gene_fold<true>, dim3(grid), dim3(kGeneBlock), 0, stream, a);
  else hipLaunchKernelGGL(k_gene_fold<false>, dim3(grid), dim3(kGeneBlock), 0, stream, a);
  hipLaunchKernelGGL(k_gene_index, dim3(grid), dim3(kGeneBlock), 0, stream, a);
  hipLaunchKernelGGL(k_gene_merge, dim3((a.n_slots + kGeneBlock - 1) / kGeneBlock), dim3(kGeneBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

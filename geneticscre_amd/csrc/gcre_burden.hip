// gcre_burden.hip -- burden tests of per-patient weights (gcre_patient_burden): for every row of
// non-negative integer weights and every permutation the weighted sum over the permutation's cases,
//     null[g][r] = sum_q w[g][q] m_r[q] = sum_b 2^b popcount(plane_b(w[g]) & m_r),
// exact in integers and independent of the order of evaluation.
//   * k_burden_planes  the uploaded int32 rows as bit planes in SetNullArgs' row layout ([W32p] dwords per plane, zero
//                      beyond the patients), every row only the planes its largest weight needs
//   * k_burden_null    count_tile (gcre_count_tile.h) with planes as rows, one half only: per item -- up to four
//                      consecutive planes of one row -- and permutation the shifted popcounts, added into sums[row][perm]
//   * k_burden_finish  per row the permutations whose sum is >= / <= the observed sum, the padding masked out (a wave
//                      walks 1,024 permutations, then one atomic per tail)
// The context-side entry (the slabs, the item list) is in gcre_host_stats.hip.  Every global write is a vector store or a
// vector atomic from plain C++.
#include "gcre_count_tile.h"

namespace gcre {
namespace {

constexpr int kBdBlock = kCtBlock;            // threads per block, of k_burden_planes and k_burden_finish as well
constexpr int kBdWaves = kCtWaves;            // one item per wave
constexpr int kBdT = kBurdenItemPlanes;       // planes per item
constexpr int kBdFinishSpan = 1024;           // permutations per wave of k_burden_finish
static_assert(kBdT == 4, "four planes per item");

}  // namespace

// grid: one wave per (listed row, 64 patients), 4 per block; wave id = listed row * Wp + word
__global__ __launch_bounds__(kBdBlock) void k_burden_planes(const BurdenPlaneArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const i64 id = (i64)blockIdx.x * kBdWaves + wave;
  if (id >= a.nact * a.Wp) return;   // the whole wave
  const i64 i = id / a.Wp;
  const int word = (int)(id % a.Wp);
  const int row = a.act[i];
  const int np = a.nplanes[i];       // 1 .. 31
  const i64 q = (i64)word * 64 + lane;
  const u32 v = q < a.n ? (u32)a.w[(i64)row * a.n + q] : 0u;   // coalesced; beyond the patients: zero bits
  u64 mine = 0;
  for (int b = 0; b < np; b++) {     // wave-uniform
    const u64 bits = __ballot((v >> b) & 1u);
    if (lane == b) mine = bits;
  }
  if (lane < np) ((u64*)a.planes)[((i64)a.pbase[i] + lane) * a.Wp + word] = mine;
}

// grid: nkt * pgroups blocks; a block stays on permutation tile kt = blockIdx.x % nkt and walks the item tiles g, g + pgroups, ..
__global__ __launch_bounds__(kBdBlock, 4) void k_burden_null(const BurdenNullArgs a) {
  constexpr int R = kCtR, PT = kCtPT, T = kBdT;

  __shared__ __attribute__((aligned(16))) u32 lds[2][kCtChunk];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kt = blockIdx.x % a.nkt;
  const int g = blockIdx.x / a.nkt;

  const u32 GCRE_CONSTANT* PLANES = as_const(a.planes);
  const BurdenItem GCRE_CONSTANT* ITEMS = as_const(a.items);

  // whether the permutation of each register is one of the K: the padding up to Kpad is never written
  bool live[R];
#pragma unroll
  for (int j = 0; j < R; j++) live[j] = kt * PT + ct_col(lane, j) < a.K;

  MaskStream ms(lds, a.masks + (size_t)kt * PT, a.Kpad);   // column offset of this permutation tile

  for (i64 pt = g; pt < a.npt; pt += a.pgroups) {
    // this wave's item; a wave past the end walks the last item and drops what it counted (the chunk loop holds a barrier)
    const i64 it = pt * kBdWaves + wave;
    const bool have = it < a.nitems;
    const BurdenItem GCRE_CONSTANT* ip = ITEMS + (have ? it : a.nitems - 1);
    const int row = ip->row, plane = ip->plane, cnt = ip->count, base = ip->base;

    // dword offsets of the item's planes, wave-uniform; a plane past the item's last reads the last one again (dropped below)
    size_t o[T];
#pragma unroll
    for (int t = 0; t < T; t++) o[t] = (size_t)(plane + (t < cnt ? t : cnt - 1)) * (size_t)a.W32p;

    const TileCounts<1, T> acc = count_tile<1, T>(ms, PLANES, o, a.W32p);

    // ---- the item's share of the sums: sum_t acc[t] << (base + t), one 64-bit integer atomic per live permutation ----
    if (!have) continue;   // wave-uniform
    unsigned long long* out = a.sums + (size_t)row * (size_t)a.Kpad + (size_t)kt * PT;
#pragma unroll
    for (int j = 0; j < R; j++) {
      u64 s = 0;
#pragma unroll
      for (int t = 0; t < T; t++)
        if (t < cnt) s += (u64)acc.v[0][t][j] << (base + t);
      if (live[j] && s != 0) atomicAdd(out + ct_col(lane, j), (unsigned long long)s);
    }
  }
}

// grid: one wave per (listed row, kBdFinishSpan permutations), 4 per block; wave id = listed row * spans + span.  A wave
// walks its span 64 permutations at a time and ends with one atomic per tail: the waves of a row meet on two addresses
__global__ __launch_bounds__(kBdBlock) void k_burden_finish(const BurdenFinishArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const i64 nsp = ((i64)a.K + kBdFinishSpan - 1) / kBdFinishSpan;
  const i64 id = (i64)blockIdx.x * kBdWaves + wave;
  if (id >= a.nact * nsp) return;   // the whole wave
  const i64 i = id / nsp;
  const i64 r0 = (id % nsp) * kBdFinishSpan;
  const unsigned long long* row = a.sums + (size_t)a.act[i] * (size_t)a.Kpad;
  const u64 obs = (u64)a.observed[i];
  u32 ge = 0, le = 0;
#pragma unroll 4
  for (int k = 0; k < kBdFinishSpan; k += 64) {
    const i64 r = r0 + k + lane;
    const bool live = r < a.K;      // a padded permutation has sum 0 <= observed: it counts in neither tail
    const u64 v = live ? row[r] : 0;
    ge += (u32)__popcll(__ballot(live && v >= obs));
    le += (u32)__popcll(__ballot(live && v <= obs));
  }
  if (lane == 0) {
    if (ge) atomicAdd(a.tails + 2 * i, (unsigned long long)ge);
    if (le) atomicAdd(a.tails + 2 * i + 1, (unsigned long long)le);
  }
}

// a grid that does not fit is refused, never clamped
hipError_t launch_burden_planes(const BurdenPlaneArgs& a, hipStream_t stream) {
  if (a.nact == 0) return hipSuccess;
  if (a.nact < 0 || a.n < 1 || a.Wp < 1 || (i64)a.Wp * 64 < a.n) return hipErrorInvalidValue;
  if (a.nact > ((i64)0x7fffffff * kBdWaves) / a.Wp) return hipErrorInvalidValue;
  const i64 blocks = (a.nact * a.Wp + kBdWaves - 1) / kBdWaves;
  if (g_launch_trace) fprintf(stderr, "launch k_burden_planes rows=%lld words=%d blocks=%lld\n", (long long)a.nact, a.Wp, (long long)blocks);
  hipLaunchKernelGGL(k_burden_planes, dim3((unsigned)blocks), dim3(kBdBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_burden_null(const BurdenNullArgs& a, hipStream_t stream) {
  if (a.nitems == 0 || a.K == 0) return hipSuccess;
  if (a.nitems < 0 || a.K < 0 || a.K > a.Kpad || a.Kpad % kCtPT != 0 || a.W32p < kCtWC || a.W32p % kCtWC != 0 ||
      a.nkt != (a.K + kCtPT - 1) / kCtPT || a.npt != (a.nitems + kBdWaves - 1) / kBdWaves || a.pgroups < 1 || a.pgroups > a.npt ||
      (i64)a.nkt * a.pgroups > 0x7fffffff)
    return hipErrorInvalidValue;
  if (g_launch_trace)   // a block walks `per` item tiles
    fprintf(stderr, "launch k_burden_null items=%lld npt=%lld pgroups=%d per=%lld\n", (long long)a.nitems, (long long)a.npt, a.pgroups,
            (long long)((a.npt + a.pgroups - 1) / a.pgroups));
  hipLaunchKernelGGL(k_burden_null, dim3((unsigned)(a.nkt * a.pgroups)), dim3(kBdBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_burden_finish(const BurdenFinishArgs& a, hipStream_t stream) {
  if (a.nact == 0 || a.K == 0) return hipSuccess;
  if (a.nact < 0 || a.K < 0 || a.K > a.Kpad) return hipErrorInvalidValue;
  const i64 nsp = ((i64)a.K + kBdFinishSpan - 1) / kBdFinishSpan;
  if (a.nact > ((i64)0x7fffffff * kBdWaves) / nsp) return hipErrorInvalidValue;
  const i64 blocks = (a.nact * nsp + kBdWaves - 1) / kBdWaves;
  if (g_launch_trace) fprintf(stderr, "launch k_burden_finish rows=%lld spans=%lld blocks=%lld\n", (long long)a.nact, (long long)nsp, (long long)blocks);
  hipLaunchKernelGGL(k_burden_finish, dim3((unsigned)blocks), dim3(kBdBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

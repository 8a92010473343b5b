// gcre_seq_prefix.hip -- sequential p-values of the variable-threshold and the multi-hit tests
// (gcre_score_sets_prefix_sequential, gcre_score_sets_dose_sequential): the null kernel between the step
// rows of gcre_prefix.hip / gcre_dose.hip and the batches of gcre_sequential.hip.
//   * k_seq_prefix_null  per (active slot, permutation of the batch): the maximum over the steps of the slot's set of the null
//                        score k_set_null gives a step row -- k_prefix_null's running maximum -- compared with the set's
//                        threshold and written as k_seq_null writes it: one ballot word per (active slot, 64 consecutive
//                        permutations), which k_seq_retire reads
// Rows are a slab's step rows (PrefixArgs' layout); the mask rows have the batch's stride, not Kpad.  No atomics; every
// global write is a vector store.  The context-side entries are in gcre_host_seq_prefix.hip, the host plan in
// gcre_seq_prefix.h.
#include "gcre_count_tile.h"
#include "gcre_sequential.h"

namespace gcre {
namespace {

constexpr int kSeqTW = kCtPT / 64;           // ballot words per tile
static_assert(kCtPT == gcre_sequential::kSeqTile, "tile");
static_assert(kCtWaves == 4, "a group is four slots: one per wave");

}  // namespace

// M method, TPW steps per wave and step tile, OCC waves per SIMD the register allocation must admit
template <int M, int TPW, int OCC>
__global__ __launch_bounds__(kCtBlock, OCC) void k_seq_prefix_null(const SeqPrefixArgs a) {
  constexpr int R = kCtR, PT = kCtPT, NW = kCtWaves;

  __shared__ __attribute__((aligned(16))) u32 lds[2][kCtChunk];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = blockIdx.x % a.nkt;
  const int g = blockIdx.x / a.nkt;

  const u32 GCRE_CONSTANT* ROWS = as_const(a.rows);
  const u32 GCRE_CONSTANT* TOT = as_const(a.tot);
  const u32 GCRE_CONSTANT* ACT = as_const(a.active);
  const int64_t GCRE_CONSTANT* ROW0 = as_const(a.row0);

  MaskStream ms(lds, a.masks + (size_t)kt * PT, a.stride);   // column offset of this permutation tile, once per block

  const size_t rs = (size_t)M * a.W32p;   // dwords per step row: (+) half, then (-) half (method 2)

  for (i64 grp = g; grp < a.ngroups; grp += a.pgroups) {
    // the step counts of the group's four slots, wave-uniform: every wave walks the step tiles of the longest of them; a wave
    // whose slot is past the list has no steps and idles on the slab's first row
    int nsteps = 0, most = 0;
    i64 row0 = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const i64 sl = grp * NW + w;
      if (sl >= a.nactive) continue;   // uniform over the block
      const u32 e = ACT[sl];
      const i64 b = ROW0[e];
      const int n = (int)(ROW0[e + 1] - b);
      most = n > most ? n : most;
      if (w == wave) {   // wave-uniform
        nsteps = n;
        row0 = b;
      }
    }
    const int ntiles = (most + TPW - 1) / TPW;

    // the running maximum over this wave's steps, per permutation of the lane
    u32 tmax[R];
#pragma unroll
    for (int j = 0; j < R; j++) tmax[j] = 0u;

    for (int st = 0; st < ntiles; st++) {
      const int kbase = st * TPW;
      // rows of this wave's steps, wave-uniform; a step past the set's end reads the set's last row (its result is dropped)
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

    // ---- the set's end: the compares by ballot, the tile's eight words (k_seq_null's finish) ----
    const i64 slot = grp * NW + wave;
    if (slot >= a.nactive) continue;   // wave-uniform; the block's barriers are all inside count_tile
    const u32 thr = as_const(a.thr)[ACT[slot]];   // (read again: nothing of it is kept across the count loop)
    // Column 64 w + i of the tile is register (w >> 2) * 4 + (i & 3) of lane (w & 3) * 16 + (i >> 2): lane i looks its bit
    // of word w up in that register's ballot, and the ballot of these bits is word w in permutation order.
    u64 mine = 0;
#pragma unroll
    for (int j0 = 0; j0 < R; j0 += 4) {
      u64 ball[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const bool live = kt * PT + ct_col(lane, j0 + j) < a.K;   // the padding of the last tile never counts
        ball[j] = __ballot(live && tmax[j0 + j] >= thr);
      }
      const u64 lo = (lane & 1) ? ball[1] : ball[0], hi = (lane & 1) ? ball[3] : ball[2];
      const u64 sel = (lane & 2) ? hi : lo;
#pragma unroll
      for (int w = 0; w < 4; w++) {
        const u64 word = __ballot(((sel >> (w * 16 + (lane >> 2))) & 1ull) != 0ull);
        if (lane == j0 + w) mine = word;
      }
    }
    const size_t wstride = (size_t)a.stride / 64;   // words per slot of the bit rows
    if (lane < kSeqTW) a.bits[(size_t)slot * wstride + (size_t)kt * kSeqTW + lane] = mine;
  }
}

// a shape that does not fit is refused, never clamped
hipError_t launch_seq_prefix_null(const SeqPrefixArgs& a, int method, hipStream_t stream) {
  if (a.nactive == 0 || a.K == 0) return hipSuccess;
  if (a.nactive < 0 || a.ngroups != (a.nactive + kCtWaves - 1) / kCtWaves || (int64_t)a.nkt * a.pgroups > 0x7fffffff || a.nkt < 1 ||
      a.pgroups < 1 || a.W32p % kCtWC != 0 || a.W32p < kCtWC || a.stride % kCtPT != 0 || (int64_t)a.nkt * kCtPT > a.stride ||
      a.K < 0 || a.K > a.nkt * kCtPT || (int64_t)a.W32p * a.stride > 0x40000000 || !a.active || !a.bits || !a.row0 || !a.thr ||
      !a.rows || !a.masks || !a.tot || (method != 1 && method != 2))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.nkt * a.pgroups));
  if (g_launch_trace)
    fprintf(stderr, "launch k_seq_prefix_null active=%lld groups=%lld pgroups=%d perms=%d\n", (long long)a.nactive, (long long)a.ngroups,
            a.pgroups, a.K);
  if (method == 1) hipLaunchKernelGGL((k_seq_prefix_null<1, 4, 4>), grid, dim3(kCtBlock), 0, stream, a);
  else hipLaunchKernelGGL((k_seq_prefix_null<2, 2, 4>), grid, dim3(kCtBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

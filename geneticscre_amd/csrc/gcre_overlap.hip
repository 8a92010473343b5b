// gcre_overlap.hip -- carrier-overlap counts of caller-given sets (gcre_set_overlap): for every pair (a[i], b[j]) the
// patients both carrier rows hold, cases and controls apart.
//   * k_set_overlap  a popcount "GEMM" of the `a` rows against the `b` rows: AND + popcount over the rows' dwords
// The context-side entry, gcre_set_overlap, is in gcre_host_stats.hip.  DESIGN.md §3.9.
//
// A block of four waves owns a 64 x 64 pair tile, a lane a 4 x 4 micro-tile of it with two counters per pair (32
// accumulators).  Both operand tiles go through LDS in chunks of 32 dwords per row (one 128-byte line), double buffered; a lane reads one
// ds_read_b128 per operand row and chunk quarter, so 8 reads feed 64 pair-dwords = 128 VALU (v_and_b32, v_bcnt_u32_b32
// with the accumulator as its addend).  Cases are the columns below n_cases: a chunk below the split dword counts into
// the case counters, one above it into the control counters, and the one chunk that holds the split dword masks its `a`
// operand both ways.  Every global access is a vector load or store.
#include "gcre_kernels.h"

#include <type_traits>

namespace gcre {
namespace {

typedef uint32_t u32;
typedef int64_t i64;
typedef u32 __attribute__((ext_vector_type(4))) u32x4;

constexpr int kOvT = kOverlapTile;    // pairs per tile edge
constexpr int kOvBlock = 256;         // threads per block: 16 x 16 lanes, 4 x 4 pairs each
constexpr int kOvKC = kOverlapChunk;  // dwords of a row per staged chunk
// LDS row stride in dwords.  A lane's rows are {t, t + 16, t + 32, t + 48} (t = its x or y index), so the 16 lanes of a
// ds_read_b128 group read rows t = 0..15 of one quarter: bank 36 t mod 64 = every multiple of 4 once --
// conflict-free for a stride of 4 * odd dwords, which also keeps every row 16-byte aligned.
constexpr int kOvStride = kOvKC + 4;
static_assert(kOvT == 64 && kOvBlock == 256 && kOvKC % 4 == 0 && (kOvT * kOvKC / 4) % kOvBlock == 0, "staging shape");
static_assert((kOvStride / 4) % 2 == 1, "row stride must be 4 * odd dwords");

// popcount(x) + acc in one instruction.  Written as C the sums of a quarter are reassociated into a tree of
// v_bcnt_u32_b32 x, 0 and v_add3_u32: 2.5 VALU per pair-dword instead of 2, and more live registers.
__device__ __forceinline__ u32 ov_bcnt(u32 x, u32 acc) {
  u32 r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}

// acc[j] += popcount(a[d] & b[j][d]) over the 4 dwords of a chunk quarter: one `a` row against the lane's four `b` rows
__device__ __forceinline__ void ov_fma(u32 (&acc)[4], const u32x4 a, const u32x4 (&b)[4]) {
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int d = 0; d < 4; d++) acc[j] = ov_bcnt(a[d] & b[j][d], acc[j]);
}

}  // namespace

__global__ __launch_bounds__(kOvBlock, 4) void k_set_overlap(const OverlapArgs p) {
  __shared__ __attribute__((aligned(16))) u32 lds[2][2][kOvT * kOvStride];   // [buffer][operand][row x stride]

  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const i64 tile_a = (i64)blockIdx.x / p.ntb, tile_b = (i64)blockIdx.x % p.ntb;
  const i64 a0 = tile_a * kOvT, b0 = tile_b * kOvT;   // first pair of the tile within the launch

  // ---- staging: thread t moves dwords [4 (t % QR), +4) of rows t / QR + RP v of both operand tiles: a row's chunk is ----
  // one 128-byte line, read by 8 neighbouring lanes.  A row past the end of its list reads the zero row, as a set with
  // an NA member does
  constexpr int QR = kOvKC / 4;          // uint4 per row and chunk
  constexpr int RP = kOvBlock / QR;      // rows per pass
  constexpr int VEC = kOvT / RP;         // passes
  const int srow = tid / QR, sq = tid % QR;
  const u32* ga[VEC];
  const u32* gb[VEC];
#pragma unroll
  for (int v = 0; v < VEC; v++) {
    const i64 ra = a0 + srow + v * RP, rb = b0 + srow + v * RP;
    const i64 ia = ra < p.na ? (i64)p.ia[ra] : p.zero_row;
    const i64 ib = rb < p.nb ? (i64)p.ib[rb] : p.zero_row;
    ga[v] = p.rows + ia * (i64)p.Wdp + sq * 4;
    gb[v] = p.rows + ib * (i64)p.Wdp + sq * 4;
  }
  u32x4 sa[VEC], sb[VEC];
  auto stage_load = [&](int c) {
#pragma unroll
    for (int v = 0; v < VEC; v++) {
      sa[v] = *(const u32x4*)(ga[v] + (size_t)c * kOvKC);
      sb[v] = *(const u32x4*)(gb[v] + (size_t)c * kOvKC);
    }
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int v = 0; v < VEC; v++) {
      *(u32x4*)(&lds[buf][0][(srow + v * RP) * kOvStride + sq * 4]) = sa[v];
      *(u32x4*)(&lds[buf][1][(srow + v * RP) * kOvStride + sq * 4]) = sb[v];
    }
  };

  u32 acc_c[4][4], acc_t[4][4];   // cases, controls
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc_c[i][j] = acc_t[i][j] = 0u;

  const int nchunks = p.Wdp / kOvKC;
  const int split = p.n_cases >> 5;                          // the dword that holds the first control
  const u32 split_mask = (1u << (p.n_cases & 31)) - 1u;      // its case bits
  const int csplit = split / kOvKC < nchunks ? split / kOvKC : nchunks;   // the chunk that holds it

  stage_load(0);
  stage_store(0);
  __syncthreads();
  int buf = 0;

  // one chunk: the next one's global loads in flight over the VALU work, then into the other LDS buffer.
  // KIND 0: every dword is cases, 1: every dword is controls, 2: the chunk of the split dword
  auto step = [&](int c, auto kind_tag) {
    constexpr int KIND = decltype(kind_tag)::value;
    // no branch in a step (the VALU work sinks below one, behind all 32 LDS reads): the last chunk stages itself again,
    // into the buffer nobody reads any more
    stage_load(c + 1 < nchunks ? c + 1 : c);
    const u32* la = &lds[buf][0][ty * kOvStride];
    const u32* lb = &lds[buf][1][tx * kOvStride];
#pragma unroll
    for (int q = 0; q < kOvKC / 4; q++) {
      u32x4 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        a[i] = *(const u32x4*)(la + i * 16 * kOvStride + q * 4);
        b[i] = *(const u32x4*)(lb + i * 16 * kOvStride + q * 4);
      }
      if constexpr (KIND == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) ov_fma(acc_c[i], a[i], b);
      } else if constexpr (KIND == 1) {
#pragma unroll
        for (int i = 0; i < 4; i++) ov_fma(acc_t[i], a[i], b);
      } else {
        u32x4 m;
#pragma unroll
        for (int d = 0; d < 4; d++) {
          const int w = c * kOvKC + q * 4 + d;
          m[d] = w < split ? 0xffffffffu : w == split ? split_mask : 0u;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
          ov_fma(acc_c[i], a[i] & m, b);
          ov_fma(acc_t[i], a[i] & ~m, b);
        }
      }
      // one quarter's 8 reads at a time: all 32 above the VALU work cost 128 registers; the block's other waves cover
      // the read latency
      __builtin_amdgcn_sched_barrier(0);
    }
    stage_store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  };

  int c = 0;
  for (; c < csplit; c++) step(c, std::integral_constant<int, 0>{});
  if (c < nchunks) step(c++, std::integral_constant<int, 2>{});
  for (; c < nchunks; c++) step(c, std::integral_constant<int, 1>{});

  // ---- guarded stores: pair (a0 + ty + 16 i, b0 + tx + 16 j), {cases, controls} as one 8-byte store ----
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const i64 ra = a0 + ty + 16 * i;
    if (ra >= p.na) continue;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const i64 rb = b0 + tx + 16 * j;
      if (rb >= p.nb) continue;
      int2 v;
      v.x = (int)acc_c[i][j];
      v.y = (int)acc_t[i][j];
      *(int2*)(p.both + (ra * p.nb + rb) * 2) = v;
    }
  }
}

hipError_t launch_set_overlap(const OverlapArgs& a, hipStream_t stream) {
  if (a.na == 0 || a.nb == 0) return hipSuccess;
  const i64 nta = (a.na + kOvT - 1) / kOvT;
  if (a.ntb != (a.nb + kOvT - 1) / kOvT || nta * a.ntb > 0x7fffffff || a.Wdp <= 0 || a.Wdp % kOvKC != 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_set_overlap, dim3((unsigned)(nta * a.ntb)), dim3(kOvBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

// gcre_count_tile.h -- device side, shared by the kernels that count one row against every mask of a permutation tile
// (k_set_null, k_family_null, k_stepdown_null, k_prefix_null, k_seq_null, k_seq_prefix_null, k_subsample_null, k_burden_null,
// k_strata_null, k_strata_check):
//   * the tile's shape and the small device helpers every such kernel needs (also used by kernels without the loop);
//   * MaskStream  the block's mask tile, double-buffered through LDS in chunks of kCtWC dwords;
//   * count_tile  acc[h][t][j] = sum over the row's dwords of popcount(row & mask), for a wave's TPW rows;
//   * null_scores the table look-up that turns a row's counts into the null score the join's kernels fold.
// It is k_null's mapping (gcre_kernels.hip) with one operand row instead of two: lanes own permutations (kCtR per lane), a
// row's words are wave-uniform (scalar loads), the mask tile is shared by the block's four waves, and a block stays on one
// permutation tile.  A kernel keeps its __shared__ arrays, how a wave finds its rows, its epilogue and its launch bounds.
#pragma once

#include "gcre_kernels.h"

namespace gcre {

typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;
typedef u32 __attribute__((ext_vector_type(4))) u32x4;

// wave-uniform read-only inputs through the constant address space: scalar loads
#define GCRE_CONSTANT __attribute__((address_space(4)))
template <typename T>
__device__ __forceinline__ const T GCRE_CONSTANT* as_const(const T* p) {
  return (const T GCRE_CONSTANT*)p;
}

// start of diagonal t of a diagonal-major table (gcre_kernels.h, "Device layout")
__device__ __forceinline__ u64 tri_index(u64 t) { return (t * (t + 1)) >> 1; }

constexpr int kCtBlock = 256;                 // threads per block
constexpr int kCtWaves = kCtBlock / 64;
constexpr int kCtR = 8;                       // permutations per lane
constexpr int kCtPT = 64 * kCtR;              // permutations per tile
constexpr int kCtWC = 4;                      // mask dwords per staged chunk (one s_load_dwordx4 per row and half)
constexpr int kCtChunk = kCtWC * kCtPT;       // dwords per staged mask chunk
constexpr int kCtVec = kCtChunk / 4 / kCtBlock;   // uint4 per thread per chunk
static_assert(kCtPT == kSetPermTile, "tile");
static_assert(kCtVec >= 1 && kCtChunk % (4 * kCtBlock) == 0, "staging shape");

// column of the permutation tile that register j of a lane holds: permutations {4 lane .. 4 lane + 3} and
// {256 + 4 lane ..}, so that both ds_read_b128 of a mask row have a 16-byte lane stride (k_null's R = 8 layout)
__device__ __forceinline__ int ct_col(int lane, int j) { return (j >> 2) * 256 + lane * 4 + (j & 3); }

// The block's (periodic) mask stream: chunk c = mask rows [c * kCtWC, c * kCtWC + kCtWC) x kCtPT columns of the tile at
// `tile`, row-major in LDS.  `stride`: dwords per mask row.  The constructor stages chunk 0 and holds a barrier; every
// thread of the block constructs it, and calls count_tile, the same number of times.
struct MaskStream {
  u32 (&lds)[2][kCtChunk];
  const char* tile;
  size_t chunk_bytes;
  u32 voff[kCtVec];
  u32x4 stage[kCtVec];
  int buf;

  __device__ __forceinline__ MaskStream(u32 (&lds_)[2][kCtChunk], const u32* tile_, int stride)
      : lds(lds_), tile((const char*)tile_), chunk_bytes((size_t)kCtWC * stride * 4), buf(1) {
#pragma unroll
    for (int i = 0; i < kCtVec; i++) {
      const int e = threadIdx.x + i * kCtBlock;
      voff[i] = (u32)((e / (kCtPT / 4)) * stride + (e % (kCtPT / 4)) * 4) * 4u;
    }
    load(0);
    store_flip();   // into buffer 0
  }
  __device__ __forceinline__ void load(int c) {
    const char* cb = tile + (size_t)c * chunk_bytes;
#pragma unroll
    for (int i = 0; i < kCtVec; i++) stage[i] = *(const u32x4*)(cb + voff[i]);
  }
  // the staged chunk into the other buffer, which becomes the current one
  __device__ __forceinline__ void store_flip() {
#pragma unroll
    for (int i = 0; i < kCtVec; i++) *(u32x4*)(&lds[buf ^ 1][(threadIdx.x + i * kCtBlock) * 4]) = stage[i];
    __syncthreads();
    buf ^= 1;
  }
  // the current chunk's masks of this lane's kCtR permutations
  __device__ __forceinline__ void read(u32 (&m)[kCtWC][kCtR]) const {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int w = 0; w < kCtWC; w++) {
      const u32* row = &lds[buf][w * kCtPT];
      const u32x4 v0 = *(const u32x4*)(row + lane * 4);
      const u32x4 v1 = *(const u32x4*)(row + 256 + lane * 4);
      m[w][0] = v0.x; m[w][1] = v0.y; m[w][2] = v0.z; m[w][3] = v0.w;
      m[w][4] = v1.x; m[w][5] = v1.y; m[w][6] = v1.z; m[w][7] = v1.w;
    }
  }
};

// acc += popcount(x) as ONE v_bcnt_u32_b32 that accumulates.  The running value is made opaque first.  Without that the
// compiler is free to take the four popcounts a register gets per chunk in pairs, each pair two v_bcnt with a zero addend, and
// to add the pairs with a v_add3_u32 -- which it does when the loop is inlined from here: a quarter more VALU work in the
// loop and some twenty more registers.  (The empty statement costs no instruction but a few s_nop behind it.)
__device__ __forceinline__ void popc_add(u32& acc, u32 x) {
  u32 run = acc;
  asm("" : "+v"(run));
  acc = run + __builtin_popcount(x);
}

// v[h][t][j]: the carriers of half h of row t among the cases of the lane's permutation j
template <int M, int TPW>
struct TileCounts {
  u32 v[M][TPW][kCtR];
};

// The counts of the rows at dword offsets o[t] (wave-uniform) of `rows`, each M halves of W32p dwords, against the whole
// stream.  A software pipeline over the flattened (chunk, row) sequence: the scalar loads of the next row's words are in
// flight while the VALU works on the current one.  W32p is a multiple of kCtWC (the launchers check).
template <int M, int TPW>
__device__ __forceinline__ TileCounts<M, TPW> count_tile(MaskStream& ms, const u32 GCRE_CONSTANT* rows, const size_t (&o)[TPW],
                                                         int W32p) {
  TileCounts<M, TPW> acc;
#pragma unroll
  for (int h = 0; h < M; h++)
#pragma unroll
    for (int t = 0; t < TPW; t++)
#pragma unroll
      for (int j = 0; j < kCtR; j++) acc.v[h][t][j] = 0u;
  const int nchunks = W32p / kCtWC;
  u32x4 nx[M];
  auto fetch = [&](int c, int t) {
    const u32 GCRE_CONSTANT* b = rows + o[t] + (size_t)c * kCtWC;
    nx[0] = *(const u32x4 GCRE_CONSTANT*)b;
    if constexpr (M == 2) nx[1] = *(const u32x4 GCRE_CONSTANT*)(b + W32p);
  };
  fetch(0, 0);
  for (int c = 0; c < nchunks; c++) {
    const int cn = (c + 1 == nchunks) ? 0 : c + 1;
    ms.load(cn);   // the next chunk of the stream

    u32 m[kCtWC][kCtR];
    ms.read(m);

#pragma unroll
    for (int t = 0; t < TPW; t++) {
      u32 jn[M][kCtWC];
#pragma unroll
      for (int h = 0; h < M; h++)
#pragma unroll
        for (int w = 0; w < kCtWC; w++) jn[h][w] = __builtin_amdgcn_readfirstlane(nx[h][w]);
      if (t + 1 < TPW) fetch(c, t + 1);
      else fetch(cn, 0);
#pragma unroll
      for (int h = 0; h < M; h++)
#pragma unroll
        for (int w = 0; w < kCtWC; w++)
#pragma unroll
          for (int j = 0; j < kCtR; j++) popc_add(acc.v[h][t][j], jn[h][w] & m[w][j]);
      __builtin_amdgcn_sched_barrier(0);   // keep each row's scalar loads in its own region
    }

    ms.store_flip();
  }
  return acc;
}

// The null score of row q as the bit pattern of a non-negative float, from the (+) half's counts pos and the (-) half's
// neg (M = 1: neg is not read).  tot: M carrier totals per row.
template <int M>
__device__ __forceinline__ void null_scores(const float* t32, const double* d64, const double* d64n, const u32 GCRE_CONSTANT* tot,
                                            i64 q, const u32 (&pos)[kCtR], const u32 (&neg)[kCtR], u32 (&v)[kCtR]) {
  if constexpr (M == 1) {
    // the sanitised f32 table: non-negative floats, ordered as their bit patterns
    const u32* diag = (const u32*)t32 + tri_index(tot[q]);
#pragma unroll
    for (int j = 0; j < kCtR; j++) v[j] = diag[pos[j]];
  } else {
    // vtmax[pp][|P| - pp] + vtmax[|N| - pn][pn] (d64n: d64, or its mirror image where vtmax is not symmetric), folded as
    // k_null folds it
    const double* dp = d64 + tri_index(tot[2 * q]);
    const double* dn = d64n + tri_index(tot[2 * q + 1]);
#pragma unroll
    for (int j = 0; j < kCtR; j++) {
      float f = (float)(dp[pos[j]] + dn[neg[j]]);
      f = (f > 0.0f) ? f : 0.0f;   // NaN and negatives fold as 0, as into the join's maxima
      v[j] = __float_as_uint(f);
    }
  }
}

}  // namespace gcre

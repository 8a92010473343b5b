// gcre_clump.hip -- greedy clumping of caller-given sets by shared carriers, on the device (gcre_clump_sets): the rule of
// report.clump_rows without a pair count leaving the GPU.  Everything is indexed by position in the walk order.
//   * k_clump_union   ORs every set's member rows into a union row in k_set_overlap's layout and counts its carriers
//   * k_clump_leads   one block: takes the next <= 64 unassigned positions as candidates, counts the 64 x 64 shared
//                     carriers among them and resolves them in walk order; the true leads go out compacted
//   * k_clump_assign  k_set_overlap's tile loop, the round's true leads against 64 later positions per block; instead of
//                     storing counts it takes the measure, picks every row's first passing lead and writes the row's result
// The context-side entry, gcre_clump_sets, is in gcre_host_stats.hip.  DESIGN.md §3.11.
//
// The chunk step is a copy of k_set_overlap's (gcre_overlap.hip), which stays as it is: a block of four waves owns a
// 64 x 64 pair tile, a lane a 4 x 4 micro-tile, both operand tiles go through LDS in chunks of 32 dwords, double buffered.
// Here the step is also compiled for 1, 2 and 3 live micro-tile rows: a round with few true leads does not pay for 64.
// Every global access is a vector load or store; the only atomics are LDS ones and the statistics counters.
#include "gcre_kernels.h"

#include <type_traits>

namespace gcre {
namespace {

typedef uint32_t u32;
typedef int64_t i64;
typedef unsigned long long u64;
typedef u32 __attribute__((ext_vector_type(4))) u32x4;

constexpr int kClT = kOverlapTile;
constexpr int kClBlock = 256;
constexpr int kClKC = kOverlapChunk;
constexpr int kClStride = kClKC + 4;     // 4 * odd dwords: conflict-free ds_read_b128, 16-byte aligned rows (gcre_overlap.hip)
constexpr int kClQR = kClKC / 4;         // uint4 per row and chunk
constexpr int kClRP = kClBlock / kClQR;  // rows per staging pass
constexpr int kClVEC = kClT / kClRP;     // passes
constexpr int kClLds = 2 * 2 * kClT * kClStride;   // [buffer][operand][row x stride]
static_assert(kClT == kClumpCand && kClBlock == 256 && kClVEC == 2 && (kClStride / 4) % 2 == 1, "tile shape");

// popcount(x) + acc in one instruction (the idiom of gcre_overlap.hip)
__device__ __forceinline__ u32 cl_bcnt(u32 x, u32 acc) {
  u32 r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}

__device__ __forceinline__ void cl_fma(u32 (&acc)[4], const u32x4 a, const u32x4 (&b)[4]) {
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int d = 0; d < 4; d++) acc[j] = cl_bcnt(a[d] & b[j][d], acc[j]);
}

// The shared counts of one 64 x 64 tile: `a` rows ia[0..63] against `b` rows ib[0..63] of U (LDS lists; the zero row for an
// absent one).  NI: the micro-tile rows i < NI are live, i.e. `a` rows below 16 NI; the others are neither staged nor
// counted and their accumulators stay 0.  All 256 threads call it; it ends behind a barrier.
template <int NI>
__device__ __forceinline__ void cl_tile(u32* lds, const u32* U, int Wdp, int n_cases, const int* ia, const int* ib,
                                        u32 (&acc_c)[4][4], u32 (&acc_t)[4][4]) {
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int srow = tid / kClQR, sq = tid % kClQR;
  const u32* ga[kClVEC];
  const u32* gb[kClVEC];
#pragma unroll
  for (int v = 0; v < kClVEC; v++) {
    ga[v] = U + (i64)ia[srow + v * kClRP] * (i64)Wdp + sq * 4;
    gb[v] = U + (i64)ib[srow + v * kClRP] * (i64)Wdp + sq * 4;
  }
  u32x4 sa[kClVEC], sb[kClVEC];
  auto stage_load = [&](int c) {
#pragma unroll
    for (int v = 0; v < kClVEC; v++) {
      if (v * kClRP < NI * 16) sa[v] = *(const u32x4*)(ga[v] + (size_t)c * kClKC);
      sb[v] = *(const u32x4*)(gb[v] + (size_t)c * kClKC);
    }
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int v = 0; v < kClVEC; v++) {
      if (v * kClRP < NI * 16) *(u32x4*)(&lds[(buf * 2 + 0) * kClT * kClStride + (srow + v * kClRP) * kClStride + sq * 4]) = sa[v];
      *(u32x4*)(&lds[(buf * 2 + 1) * kClT * kClStride + (srow + v * kClRP) * kClStride + sq * 4]) = sb[v];
    }
  };
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc_c[i][j] = acc_t[i][j] = 0u;

  const int nchunks = Wdp / kClKC;
  const int split = n_cases >> 5;
  const u32 split_mask = (1u << (n_cases & 31)) - 1u;
  const int csplit = split / kClKC < nchunks ? split / kClKC : nchunks;

  stage_load(0);
  stage_store(0);
  __syncthreads();
  int buf = 0;

  // KIND 0: every dword is cases, 1: every dword is controls, 2: the chunk of the split dword
  auto step = [&](int c, auto kind_tag) {
    constexpr int KIND = decltype(kind_tag)::value;
    stage_load(c + 1 < nchunks ? c + 1 : c);
    const u32* la = &lds[(buf * 2 + 0) * kClT * kClStride + ty * kClStride];
    const u32* lb = &lds[(buf * 2 + 1) * kClT * kClStride + tx * kClStride];
#pragma unroll
    for (int q = 0; q < kClKC / 4; q++) {
      u32x4 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (i < NI) a[i] = *(const u32x4*)(la + i * 16 * kClStride + q * 4);
        b[i] = *(const u32x4*)(lb + i * 16 * kClStride + q * 4);
      }
      if constexpr (KIND == 0) {
#pragma unroll
        for (int i = 0; i < NI; i++) cl_fma(acc_c[i], a[i], b);
      } else if constexpr (KIND == 1) {
#pragma unroll
        for (int i = 0; i < NI; i++) cl_fma(acc_t[i], a[i], b);
      } else {
        u32x4 m;
#pragma unroll
        for (int d = 0; d < 4; d++) {
          const int w = c * kClKC + q * 4 + d;
          m[d] = w < split ? 0xffffffffu : w == split ? split_mask : 0u;
        }
#pragma unroll
        for (int i = 0; i < NI; i++) {
          cl_fma(acc_c[i], a[i] & m, b);
          cl_fma(acc_t[i], a[i] & ~m, b);
        }
      }
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
}

// The measure of a pair, as report.clump_rows takes it: both / den in f64, correctly rounded, 0.0 on a zero denominator.
// ca / cb: the (cases, controls) carriers of the two rows; bc / bt: what they share.
__device__ __forceinline__ double cl_value(const ClumpArgs& p, int2 ca, int2 cb, u32 bc, u32 bt) {
  const i64 A = (i64)ca.x + (p.patients == 0 ? ca.y : 0);
  const i64 B = (i64)cb.x + (p.patients == 0 ? cb.y : 0);
  const i64 bo = (i64)bc + (p.patients == 0 ? (i64)bt : 0);
  const i64 den = p.measure == 0 ? A + B - bo : (A < B ? A : B);
  return den > 0 ? __ddiv_rn((double)bo, (double)den) : 0.0;
}

// a member row: its clump, its lead's position, the measure and the shared carriers; it is free no longer
__device__ __forceinline__ void cl_write_member(const ClumpArgs& p, i64 pos, int clump, int lead, double v, u32 bc, u32 bt) {
  p.clump[pos] = clump;
  p.lead[pos] = lead;
  p.value[pos] = v;
  int2 s;
  s.x = (int)bc;
  s.y = (int)bt;
  *(int2*)(p.shared + pos * 2) = s;
  p.free_[pos] = 0u;
}

}  // namespace

// grid: one wave per position (4 per block)
__global__ __launch_bounds__(kClBlock) void k_clump_union(const ClumpArgs p, const ClumpUnionArgs u) {
  const i64 pos = (i64)blockIdx.x * (kClBlock / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pos >= p.n) return;
  const int32_t* mem = u.members + pos * u.M;
  const int split = p.n_cases >> 5;
  const u32 split_mask = (1u << (p.n_cases & 31)) - 1u;
  u32 cases = 0, ctrls = 0;
  for (int w = lane; w < p.Wdp; w += 64) {
    u32 x = 0;
    if (w < u.W2 && w * 32 < u.n_patients) {
      for (int m = 0; m < u.M; m++) {
        const int g = mem[m];
        if (g >= 0) x |= u.rows[(i64)g * u.W2 + w];
      }
      const int left = u.n_patients - w * 32;   // patients from this dword on
      if (left < 32) x &= (1u << left) - 1u;
    }
    p.U[pos * (i64)p.Wdp + w] = x;
    const u32 cm = w < split ? 0xffffffffu : w == split ? split_mask : 0u;
    cases += __popc(x & cm);
    ctrls += __popc(x & ~cm);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    cases += __shfl_down(cases, d, 64);
    ctrls += __shfl_down(ctrls, d, 64);
  }
  if (lane == 0) {
    int2 k;
    k.x = (int)cases;
    k.y = (int)ctrls;
    *(int2*)(p.cnt + pos * 2) = k;
    p.free_[pos] = 1u;
  }
}

// one block
__global__ __launch_bounds__(kClBlock) void k_clump_leads(const ClumpArgs p) {
  __shared__ __attribute__((aligned(16))) u32 lds[kClLds];
  __shared__ int s_cand[kClT];     // the candidates' positions; the zero row behind the last
  __shared__ int2 s_cnt[kClT];
  __shared__ u64 s_pass[kClT];     // bit j of s_pass[i]: candidates i < j reach r
  __shared__ int s_own[kClT];      // the candidate that absorbed candidate j, -1: j is a lead
  __shared__ int s_id[kClT];       // the clump id of a lead
  __shared__ int s_wave[kClBlock / 64];

  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int lane = tid & 63, wv = tid >> 6;
  const ClumpState st = *p.state;
  const i64 n = p.n;
  if (st.cursor >= n) {   // the walk is over: an empty round
    if (tid == 0) {
      ClumpState o = st;
      o.ncand = o.nlead = 0;
      *p.state = o;
    }
    return;
  }

  // ---- the next <= 64 free positions at or after the cursor, found 256 positions at a time by votes ----
  if (tid < kClT) {
    s_cand[tid] = (int)n;
    s_pass[tid] = 0ull;
    s_own[tid] = -1;
    s_id[tid] = -1;
  }
  __syncthreads();
  int found = 0;
  for (i64 base = st.cursor; found < kClT && base < n; base += kClBlock) {
    const i64 pos = base + tid;
    const bool f = pos < n && p.free_[pos] != 0u;
    const u64 bal = __ballot(f);
    if (lane == 0) s_wave[wv] = __popcll(bal);
    __syncthreads();
    int off = found, total = 0;
    for (int w = 0; w < kClBlock / 64; w++) {
      if (w < wv) off += s_wave[w];
      total += s_wave[w];
    }
    const int rank = off + __popcll(bal & ((1ull << lane) - 1ull));
    if (f && rank < kClT) s_cand[rank] = (int)pos;
    found += total;   // (the same in every thread)
    __syncthreads();
  }
  const int ncand = found < kClT ? found : kClT;
  const int cursor = found >= kClT ? s_cand[kClT - 1] + 1 : (int)n;
  if (ncand == 0) {   // nothing left behind the cursor: the walk is over, an empty round
    if (tid == 0) {
      ClumpState o = st;
      o.cursor = cursor;
      o.ncand = o.nlead = 0;
      *p.state = o;
    }
    return;
  }
  if (tid < kClT) s_cnt[tid] = tid < ncand ? *(const int2*)(p.cnt + (i64)s_cand[tid] * 2) : make_int2(0, 0);
  __syncthreads();

  // ---- the shared counts among the candidates ----
  u32 acc_c[4][4], acc_t[4][4];
  cl_tile<4>(lds, p.U, p.Wdp, p.n_cases, s_cand, s_cand, acc_c, acc_t);
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int ci = ty + 16 * i, cj = tx + 16 * j;
      if (ci < cj && cj < ncand && cl_value(p, s_cnt[ci], s_cnt[cj], acc_c[i][j], acc_t[i][j]) >= p.r)
        atomicOr(&s_pass[ci], 1ull << cj);
    }
  __syncthreads();

  // ---- wave 0 resolves them in walk order, lane j = candidate j: i is a lead iff no earlier lead absorbed it, and a later
  // candidate joins the first lead it reaches ----
  if (wv == 0) {
    const bool valid = lane < ncand;
    bool absorbed = false;
    int own = -1;
    u64 absmask = 0ull, leadmask = 0ull;
    for (int i = 0; i < ncand; i++) {
      if ((absmask >> i) & 1ull) continue;   // (the same in every lane)
      leadmask |= 1ull << i;
      if (valid && lane > i && !absorbed && ((s_pass[i] >> lane) & 1ull)) {
        absorbed = true;
        own = i;
      }
      absmask = __ballot(absorbed);
    }
    const int nlead = __popcll(leadmask);
    if (valid) {
      const i64 pos = s_cand[lane];
      if (!absorbed) {
        const int rank = __popcll(leadmask & ((1ull << lane) - 1ull));
        const int id = st.next_clump + rank;
        s_id[lane] = id;
        p.leads[rank] = (int)pos;
        p.clump[pos] = id;
        p.lead[pos] = (int)pos;
        p.value[pos] = __longlong_as_double(0x7ff8000000000000ll);
        *(int2*)(p.shared + pos * 2) = make_int2(-1, -1);
        p.free_[pos] = 0u;
      } else {
        s_own[lane] = own;
      }
    }
    if (lane == 0) {
      ClumpState o;
      o.cursor = cursor;
      o.ncand = ncand;
      o.nlead = nlead;
      o.next_clump = st.next_clump + nlead;
      *p.state = o;
      p.stats[kClumpRounds] += 1ull;   // (one block, one lane)
    }
  }
  __syncthreads();

  // ---- the lane that owns pair (lead, absorbed candidate) writes the candidate's result ----
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int ci = ty + 16 * i, cj = tx + 16 * j;
      if (cj < ncand && s_own[cj] == ci)
        cl_write_member(p, s_cand[cj], s_id[ci], s_cand[ci], cl_value(p, s_cnt[ci], s_cnt[cj], acc_c[i][j], acc_t[i][j]),
                        acc_c[i][j], acc_t[i][j]);
    }
}

// block b: the round's true leads against positions [64 (tile0 + b), +64)
__global__ __launch_bounds__(kClBlock, 4) void k_clump_assign(const ClumpArgs p, const i64 tile0) {
  __shared__ __attribute__((aligned(16))) u32 lds[kClLds];
  __shared__ int s_lead[kClT];     // the leads' positions; the zero row behind the last
  __shared__ int s_row[kClT];      // the tile's positions; the zero row past the end
  __shared__ int2 s_lcnt[kClT];
  __shared__ int2 s_rcnt[kClT];
  __shared__ u32 s_free[kClT];
  __shared__ u32 s_first[kClT];    // the first lead (index into the compacted list) that a row reaches

  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const ClumpState st = *p.state;
  const int nlead = st.nlead;
  const i64 n = p.n;
  const i64 b0 = ((i64)blockIdx.x + tile0) * kClT;
  if (nlead == 0 || b0 + kClT <= st.cursor || b0 >= n) return;   // an empty round; a tile the walk has passed

  bool f = false;
  if (tid < kClT) {
    const i64 pos = b0 + tid;
    f = pos < n && p.free_[pos] != 0u;
    s_free[tid] = f ? 1u : 0u;
    s_first[tid] = 0xffffffffu;
    s_row[tid] = pos < n ? (int)pos : (int)n;
    s_rcnt[tid] = pos < n ? *(const int2*)(p.cnt + pos * 2) : make_int2(0, 0);
    const int lp = tid < nlead ? p.leads[tid] : (int)n;
    s_lead[tid] = lp;
    s_lcnt[tid] = tid < nlead ? *(const int2*)(p.cnt + (i64)lp * 2) : make_int2(0, 0);
  }
  if (!__syncthreads_or(f ? 1 : 0)) {   // no free row: one load and one vote
    if (tid == 0) atomicAdd(p.stats + kClumpTilesSkipped, 1ull);
    return;
  }
  if (tid == 0) atomicAdd(p.stats + kClumpTilesRun, 1ull);

  u32 acc_c[4][4], acc_t[4][4];
  const int ni = (nlead + 15) >> 4;   // live micro-tile rows: the work follows the round's true leads
  if (ni == 1) cl_tile<1>(lds, p.U, p.Wdp, p.n_cases, s_lead, s_row, acc_c, acc_t);
  else if (ni == 2) cl_tile<2>(lds, p.U, p.Wdp, p.n_cases, s_lead, s_row, acc_c, acc_t);
  else if (ni == 3) cl_tile<3>(lds, p.U, p.Wdp, p.n_cases, s_lead, s_row, acc_c, acc_t);
  else cl_tile<4>(lds, p.U, p.Wdp, p.n_cases, s_lead, s_row, acc_c, acc_t);

  // ---- epilogue: per pair the measure and the compare, per row the first passing lead ----
  double val[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int li = ty + 16 * i, col = tx + 16 * j;
      val[i][j] = 0.0;
      if (li < nlead && s_free[col]) {
        val[i][j] = cl_value(p, s_lcnt[li], s_rcnt[col], acc_c[i][j], acc_t[i][j]);
        if (val[i][j] >= p.r) atomicMin(&s_first[col], (u32)li);
      }
    }
  __syncthreads();
  const int base = st.next_clump - nlead;   // the clump id of the round's first lead
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int li = ty + 16 * i, col = tx + 16 * j;
      if (s_first[col] == (u32)li && s_free[col])
        cl_write_member(p, b0 + col, base + li, s_lead[li], val[i][j], acc_c[i][j], acc_t[i][j]);
    }
}

hipError_t launch_clump_union(const ClumpArgs& a, const ClumpUnionArgs& u, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  const i64 blocks = (a.n + kClBlock / 64 - 1) / (kClBlock / 64);
  if (blocks > 0x7fffffff || a.n >= 0x7fffffff || a.Wdp <= 0 || a.Wdp % kClKC != 0 || u.M < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_clump_union, dim3((unsigned)blocks), dim3(kClBlock), 0, stream, a, u);
  return hipGetLastError();
}

hipError_t launch_clump_round(const ClumpArgs& a, int64_t tile0, hipStream_t stream) {
  const i64 tiles = (a.n + kClT - 1) / kClT - tile0;
  if (a.n <= 0 || tile0 < 0 || tiles < 1 || tiles > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_clump_leads, dim3(1), dim3(kClBlock), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_clump_assign, dim3((unsigned)tiles), dim3(kClBlock), 0, stream, a, tile0);
  return hipGetLastError();
}

}  // namespace gcre

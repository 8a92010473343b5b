// gcre_ie.hip -- the inclusion-exclusion form of the permutation (null) kernel for gfx950, and the count planes
// it runs on.
//
// Same result as k_null / k_null_sparse -- count[p][r] = popc(joined_p & mask_r), reference src/methods.h:73-88 --
// but a joined path is never walked bit by bit.  Every path set keeps, next to its rows, its COUNT PLANES
//
//     N[row][r] = popc(row & mask_r)        bit-sliced: plane p of tile kt holds bit p of 2048 counts
//
// and a joined path  p0[idx] | z  (z = the row the join adds: one gene at levels 1-4, a 2-gene path at level 5) is
//
//     count = N0[idx] + Nz[z] - popc(p0[idx] & z & mask_r)
//
// N0[idx] is loaded once per uid (all `count` joins of a uid share paths0[idx], join_base.cpp:242), Nz[z] is a
// couple of wide loads, and only the OVERLAP p0[idx] & z -- a handful of patients for rare variants -- is still
// streamed as transposed mask rows through the carry-save tree of gcre_bitslice.h.  Paths whose overlap is longer
// than what the join adds fall back, per path, to streaming the delta z & ~p0 (what k_null_sparse always does).
// A kept join writes the planes of its joined paths as a by-product: they are the N0 of the next level.
//
// The epilogue is pruned exactly: the running maxima only move when T[total][count] exceeds them, and for a
// threshold theta no larger than any running maximum of the tile the counts that can matter lie outside an interval
// [lo, hi] of the path's table diagonal (precomputed ladder, k_build_ladder).  Two bit-sliced borrow chains test
// all 2048 counts of a path against (lo, hi); only when some permutation falls outside does the wave transpose its
// counters and look the table up (finish_m1).  Skipping a lookup whose value cannot exceed the maximum leaves every
// maximum bit-identical.
#include "gcre_ie_common.h"

namespace gcre {

// section clocks of a diagnostics build (-DGCRE_IE_TIMING): every mark drains the wave's memory counters first
#ifdef GCRE_IE_TIMING
#define GCRE_TM_MARK(var) __builtin_amdgcn_s_waitcnt(0); const u64 var = __builtin_amdgcn_s_memtime()
#define GCRE_TM_ADD(i, t1, t0) tm[i] += (t1) - (t0)
#else
#define GCRE_TM_MARK(var)
#define GCRE_TM_ADD(i, t1, t0)
#endif

// The general kernel: both methods, every count looked up (no pruning).  Runs the signed method, and for method 1 the
// warm-up slice that seeds the pruned kernel's thresholds.  L = counter planes of the joined paths, a multiple of 4.
//
// Work is dealt by BLOCK.  A chunk is kIeWaves neighbouring segments of one tile, one per wave of a block; the launch's
// chunks, tile-major, are cut into eight contiguous parts, one per XCD (blocks b and b + 8 share an L2), and block i of
// an XCD takes chunks i, i + blocks-per-XCD, ... of its part.  So the blocks of an XCD work on neighbouring segments of
// one tile at a time (the table is sorted by the added rows), the tiles a block visits are consecutive, and blocks
// differ by one chunk at the most.  Striding matters: segments differ in length and long ones come in runs -- contiguous
// equal shares of the table left the slowest wave at 3.2 times the mean, strides at 1.8 (profiles/warmup_after.txt).
// The four waves change tile together, and their running maxima leave LDS in ONE merged flush per (block, tile): see
// flush below.  Every wave of a block walks every chunk of the block, with or without a segment of its own in it, and
// no wave leaves before the last flush: the flush has the kernel's only barriers.
template <int M, int L>
__global__ __launch_bounds__(64 * kIeWaves) __attribute__((amdgpu_waves_per_eu(M == 1 ? 4 : 2))) void k_null_ie(const IeArgs /* read through ie_args() */) {
  // every argument is read through ap where it is used, never through the by-value copy (gcre_ie_common.h)
  const IeArgs GCRE_CONSTANT* ap = ie_args();
  static_assert(L % 4 == 0 && L >= 8 && L <= 16, "planes come in groups of 4");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int xcd = blockIdx.x & 7;
  const i64 bi = (i64)(blockIdx.x >> 3);
  const i64 bx = ap->waves_per_xcd / kIeWaves;   // blocks per XCD (launch_null_ie: waves_per_xcd is a multiple of kIeWaves)
  const i64 cpt = (ap->seg_end - ap->seg_begin + kIeWaves - 1) / kIeWaves;   // chunks per tile
  const i64 chunks = cpt * ap->nkt;                                        // < 2^45
  const u32 lane4 = (u32)lane * 4u;
  // the waves' 2048 running maxima of the block's current tile: 8 KB of LDS each, [q][lane] <-> permutation 32 * lane + q
  __shared__ u32 gmax_lds[kIeWaves][32 * 64];
  u32* scr = gmax_lds[wave] + lane;
#pragma unroll
  for (int q = 0; q < 32; q++) scr[q * 64] = 0u;

  int cur_kt = -1;
  __amdgpu_buffer_rsrc_t mt = __builtin_amdgcn_make_buffer_rsrc((void*)ap->mt, 0, 0x7fffffff, 0x00020000);
#ifdef GCRE_IE_TIMING
  u64 tm[6] = {0, 0, 0, 0, 0, 0};   // segment prologue, path loop up to the counts, transpose + look-ups, flush, flushes, total
  const u64 tm_begin = __builtin_amdgcn_s_memtime();
#endif

  // The block's merged flush, when its tile changes and at the end (cur_kt is block-uniform: all four waves come here
  // together).  Behind a barrier the four waves' arrays are combined: wave w takes permutations [512 w, 512 w + 512) of
  // the tile, 8 consecutive ones per lane -- two wide loads of the global values, past the caches that never see the
  // other XCDs' atomics (sc1, as the pruned kernels' exchange) -- and issues atomicMax only where the block's maximum is
  // larger.  A stale global value is a smaller one: an atomic too many, never one too few.  All four arrays are zero
  // again behind the second barrier, for the next tile.
  auto flush = [&]() {
    if (cur_kt < 0) return;
    GCRE_TM_MARK(tf0);
    __syncthreads();
    const u32 slot0 = (u32)wave * 512u + (u32)lane * 8u;
    __amdgpu_buffer_rsrc_t nb = __builtin_amdgcn_make_buffer_rsrc((void*)(ap->null_bits + (size_t)cur_kt * 2048), 0, 8192, 0x00020000);
    const u32x4 g0 = __builtin_amdgcn_raw_buffer_load_b128(nb, slot0 * 4u, 0, 16 /* sc1 */);
    const u32x4 g1 = __builtin_amdgcn_raw_buffer_load_b128(nb, slot0 * 4u + 16u, 0, 16 /* sc1 */);
    u32* out = ap->null_bits + (size_t)cur_kt * 2048 + slot0;
    u32* cell = &gmax_lds[0][0] + (slot0 & 31u) * 64u + (slot0 >> 5);   // permutation 32 l + q lives at [q][l]
    u32 own[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      u32 m = 0u;
#pragma unroll
      for (int w = 0; w < kIeWaves; w++) {
        const u32 v = cell[w * 32 * 64 + j * 64];
        m = v > m ? v : m;
        cell[w * 32 * 64 + j * 64] = 0u;
      }
      own[j] = m;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const u32 g = j < 4 ? g0[j & 3] : g1[j & 3];
      if (own[j] > g) atomicMax(out + j, own[j]);
    }
    __syncthreads();
    GCRE_TM_MARK(tf1);
    GCRE_TM_ADD(3, tf1, tf0);
#ifdef GCRE_IE_TIMING
    tm[4] += 1;
#endif
  };

  auto to_counts = [&](const u32 (&C)[L], u32 (&R)[16]) {
#pragma unroll
    for (int l = 0; l < 16; l++) R[l] = (l < L) ? C[l] : 0u;
    transpose16(R);
  };
  // method 1: counts -> f32 table diagonal -> running maxima (methods.h:96-103).  All 32 table cells and all 32
  // running maxima of the lane are independent loads, in flight together.
  auto finish_m1 = [&](const u32 (&C)[L], u32 total) {
    u32 R[16];
    to_counts(C, R);
    const u32* diag_g = (const u32*)ap->t32 + sp_diag_offset(total);
    u32 v[32], o[32];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      v[j] = diag_g[R[j] & 0xffffu];
      v[j + 16] = diag_g[R[j] >> 16];
    }
#pragma unroll
    for (int q = 0; q < 32; q++) o[q] = scr[q * 64];
#pragma unroll
    for (int q = 0; q < 32; q++)
      if (v[q] > o[q]) scr[q * 64] = v[q];
  };

  // method 2: vtmax[a][tp-a] + vtmax[tn-b][b] in f64, rounded to f32, clamped at 0 (methods.h:220-230)
  auto finish_m2 = [&](const u32 (&Cp)[L], const u32 (&Cn)[L], u32 tp, u32 tn) {
    u32 Rp[16], Rn[16];
    to_counts(Cp, Rp);
    to_counts(Cn, Rn);
    const double* dp = ap->d64 + sp_diag_offset(tp);
    const double* dn = ap->d64 + sp_diag_offset(tn);
#pragma unroll
    for (int g0 = 0; g0 < 16; g0 += 4) {
      double sp[8], sn[8];
      u32 o[8];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        sp[k] = dp[Rp[g0 + k] & 0xffffu];
        sn[k] = dn[Rn[g0 + k] & 0xffffu];
        sp[k + 4] = dp[Rp[g0 + k] >> 16];
        sn[k + 4] = dn[Rn[g0 + k] >> 16];
        o[k] = scr[(g0 + k) * 64];
        o[k + 4] = scr[(g0 + k + 16) * 64];
      }
#pragma unroll
      for (int k = 0; k < 8; k++) {
        float f = (float)(sp[k] + sn[k]);
        f = (f > 0.0f) ? f : 0.0f;
        const u32 v = __float_as_uint(f);
        const int q = (k < 4) ? g0 + k : g0 + k - 4 + 16;
        if (v > o[k]) scr[q * 64] = v;
      }
    }
  };

  // count planes of one (row-half, tile): `unit` = ((row*M + half) * nkt + tile) * groups; groups of 4 planes,
  // [group][lane][4] dwords = 1 KB per group
  auto load_planes = [&](u32 (&P)[L], const u32* planes, u32 unit, int groups) {
    const u32x4* src = (const u32x4*)(planes + (u64)unit * 256u) + lane;
#pragma unroll
    for (int j = 0; j < L / 4; j++) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (j < groups) v = src[j * 64];
      P[4 * j + 0] = v.x;
      P[4 * j + 1] = v.y;
      P[4 * j + 2] = v.z;
      P[4 * j + 3] = v.w;
    }
  };

  const i64 c_end = (i64)(xcd + 1) * chunks / 8;
  for (i64 c = (i64)xcd * chunks / 8 + bi; c < c_end; c += bx) {   // block-uniform
    ie_args_again(ap);
    const int kt = (int)(c / cpt);
    if (kt != cur_kt) {
      flush();
      cur_kt = kt;
      mt = __builtin_amdgcn_make_buffer_rsrc((void*)(ap->mt + (size_t)kt * ap->mt_rows * 64), 0, 0x7fffffff, 0x00020000);
    }
    const i64 sidx = ap->seg_begin + (c - (i64)kt * cpt) * kIeWaves + wave;
    if (sidx < ap->seg_end) {   // (a tile's last chunk may be short)
      GCRE_TM_MARK(ts0);
      const SparseSeg GCRE_CONSTANT* segs = (const SparseSeg GCRE_CONSTANT*)ap->segs;
      const u32 row0 = segs[sidx].row0;
      const u32 first = segs[sidx].first;
      const u32 npaths = segs[sidx].n;
      // ---- per-path metadata of the whole segment in a few coalesced loads: lane t <-> joined path first + t.
      // The path loop below takes everything out of these registers with v_readlane.
      const u32 qv = first + (((u32)lane < npaths) ? (u32)lane : 0u);
      u32 infov[M], lovv[M];   // padded list length | mode, and where a long list continues
#pragma unroll
      for (int h = 0; h < M; h++) {
        infov[h] = ap->linfo[(u64)qv * M + h];
        lovv[h] = ap->lover[(u64)qv * M + h];
      }
      const u32 rzv = ap->rowz[qv];
      u32 zunit[M];      // where the planes of the added row-half start, in 1 KB units
#pragma unroll
      for (int h = 0; h < M; h++) {
        const u32 hz = (M == 2 && (rzv >> 31)) ? (u32)(1 - h) : (u32)h;
        zunit[h] = ((u32)kt * (u32)ap->rowsz + (rzv & 0x7fffffffu) * (u32)M + hz) * (u32)ap->gz;
      }
      u32 ttv[M];
#pragma unroll
      for (int h = 0; h < M; h++) ttv[h] = ap->tot[(u64)qv * M + h];
      u32 lv[M][8];      // the first 8 entries of every list (lists are padded to 8: most lists end there)
#pragma unroll
      for (int h = 0; h < M; h++) {
        const u32x4* lp = (const u32x4*)(ap->dlist + ((u64)qv * M + h) * 8u);
        const u32x4 e0 = lp[0], e1 = lp[1];
        lv[h][0] = e0.x; lv[h][1] = e0.y; lv[h][2] = e0.z; lv[h][3] = e0.w;
        lv[h][4] = e1.x; lv[h][5] = e1.y; lv[h][6] = e1.z; lv[h][7] = e1.w;
      }

      auto stream = [&](u32 (&P)[L], const u32 GCRE_CONSTANT* list, u64 p, u64 e) {
        u32 x[16];
        for (; p + 16 <= e; p += 16) {
          load16(x, mt, lane4, *(const u32x16 GCRE_CONSTANT*)(list + p));
          add16<L>(P, x);
        }
        for (; p < e; p += 4) {
          const u32x4 offs = *(const u32x4 GCRE_CONSTANT*)(list + p);
          u32 y4[4];
#pragma unroll
          for (int j = 0; j < 4; j++) y4[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, offs[j], 0);
          add4<L>(P, y4);
        }
      };

      // ---- base counters: the planes of paths0[row0], or its bits streamed when the set has no planes ----
      u32 B[M][L];
#pragma unroll
      for (int h = 0; h < M; h++) {
        const u64 r = (u64)row0 * M + h;
        if (ap->planes0) {
          load_planes(B[h], ap->planes0, (u32)(((u64)kt * (u64)ap->rows0 + r) * (u64)ap->g0), ap->g0);
        } else if (ap->rec_slot) {
          // the set has the recipe of the join that made it (see k_null_ie_m1 / k_null_ie_m2): per half
          // A[row0'][h] + Z[z'][h'] -/+ that join's list of the half (rec_rows_a / rec_rows_z count row-halves)
          const u32 ra = ap->rec_row0[row0], rzr = ap->rec_rowz[row0], rz = rzr & 0x7fffffffu, rinfo = ap->rec_linfo[r];
          const u32 hz = (M == 2 && (rzr >> 31)) ? (u32)(1 - h) : (u32)h;
          u32 ZR[L], S[L];
          load_planes(B[h], ap->rec_planes_a, (u32)(((u64)kt * (u64)ap->rec_rows_a + (u64)ra * M + h) * (u64)ap->rec_ga), ap->rec_ga);
          load_planes(ZR, ap->rec_planes_z, (u32)(((u64)kt * (u64)ap->rec_rows_z + (u64)rz * M + hz) * (u64)ap->rec_gz), ap->rec_gz);
#pragma unroll
          for (int l = 0; l < L; l++) S[l] = 0u;
          const u32 rlen = linfo_len(rinfo);
          stream(S, (const u32 GCRE_CONSTANT*)(ap->rec_slot + r * 8u), 0, 8);
          if (rlen > 8u) stream(S, (const u32 GCRE_CONSTANT*)(ap->rec_over + ap->rec_lover[r]), 0, (u64)(rlen - 8u));
          u32 cy = 0u, bw = 0u;
#pragma unroll
          for (int l = 0; l < L; l++) {
            const u32 zl = linfo_overlap(rinfo) ? ZR[l] : S[l];   // overlap list: + Z - S; delta list: + S
            const u32 sl_ = linfo_overlap(rinfo) ? S[l] : 0u;
            const u32 s1_ = B[h][l] ^ zl ^ cy;
            cy = maj3(B[h][l], zl, cy);
            B[h][l] = s1_ ^ sl_ ^ bw;
            bw = maj3(~s1_, sl_, bw);
          }
        } else {
#pragma unroll
          for (int l = 0; l < L; l++) B[h][l] = 0u;
          const u64 GCRE_CONSTANT* loff0 = (const u64 GCRE_CONSTANT*)ap->loff0;
          stream(B[h], (const u32 GCRE_CONSTANT*)ap->lidx0, loff0[r], loff0[r + 1]);
        }
      }

      GCRE_TM_MARK(ts1);
      GCRE_TM_ADD(0, ts1, ts0);
      for (u32 t = 0; t < npaths; t++) {
        GCRE_TM_MARK(tp0);
        const u32 q = first + t;
        u32 C[M][L];
#pragma unroll
        for (int h = 0; h < M; h++) {
          const u32 r0 = rdlane(infov[h], t);
          const u32 len = linfo_len(r0);
          const bool overlap = linfo_overlap(r0);
          // the 8 mask rows every list starts with (zero rows past its real end) ...
          u32 offs[8], y[8];
#pragma unroll
          for (int j = 0; j < 8; j++) offs[j] = rdlane(lv[h][j], t);
#pragma unroll
          for (int j = 0; j < 8; j++) y[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, offs[j], 0);
          // ... and the planes of the row the join adds, when the list is the overlap with paths0
          u32 Z[L];
          if (overlap) {
            load_planes(Z, ap->planesz, rdlane(zunit[h], t), ap->gz);
          } else {
#pragma unroll
            for (int l = 0; l < L; l++) Z[l] = 0u;
          }
          // sum of the 8 rows: 4 planes
          u32 c0, a0, c1, a1, c2, a2, d0, b0;
          csa(c0, a0, y[0], y[1], y[2]);
          csa(c1, a1, y[3], y[4], y[5]);
          csa(c2, a2, a0, a1, y[6]);
          const u32 s0 = a2 ^ y[7], c3 = a2 & y[7];
          csa(d0, b0, c0, c1, c2);
          const u32 s1 = b0 ^ c3, d1 = b0 & c3;
          u32 S[L];
          S[0] = s0; S[1] = s1; S[2] = d0 ^ d1; S[3] = d0 & d1;
#pragma unroll
          for (int l = 4; l < L; l++) S[l] = 0u;
          if (len > 8u) stream(S, (const u32 GCRE_CONSTANT*)(ap->dover + rdlane(lovv[h], t)), 0, (u64)(len - 8u));   // long list (rare)
          if (overlap) {   // C = B + Nz - S
            u32 cy = 0u, bw = 0u;
#pragma unroll
            for (int l = 0; l < L; l++) {
              const u32 s1_ = B[h][l] ^ Z[l] ^ cy;
              cy = maj3(B[h][l], Z[l], cy);
              C[h][l] = s1_ ^ S[l] ^ bw;
              bw = maj3(~s1_, S[l], bw);
            }
          } else {         // C = B + S
            u32 cy = 0u;
#pragma unroll
            for (int l = 0; l < L; l++) {
              C[h][l] = B[h][l] ^ S[l] ^ cy;
              cy = maj3(B[h][l], S[l], cy);
            }
          }
        }
        if (ap->planes_out) {
#pragma unroll
          for (int h = 0; h < M; h++) {
            const u64 rh = ((u64)ap->out_first + q) * M + h;
            u32x4* dst = (u32x4*)(ap->planes_out + (((u64)cur_kt * (u64)ap->rows_out + rh) * (u64)ap->go) * 256u) + lane;
#pragma unroll
            for (int j = 0; j < 4; j++) {
              if (j < ap->go) {
                u32x4 v = {0u, 0u, 0u, 0u};
                if (4 * j < L) v = u32x4{C[h][(4 * j) % L], C[h][(4 * j + 1) % L], C[h][(4 * j + 2) % L], C[h][(4 * j + 3) % L]};
                dst[j * 64] = v;
              }
            }
          }
        }
        GCRE_TM_MARK(tp1);
        GCRE_TM_ADD(1, tp1, tp0);
        if (q < ap->score_begin || q >= ap->score_end) continue;   // planes only: the path belongs to another shard
        if constexpr (M == 1) {
          finish_m1(C[0], rdlane(ttv[0], t));
        } else {
          finish_m2(C[0], C[M - 1], rdlane(ttv[0], t), rdlane(ttv[M - 1], t));
        }
        GCRE_TM_MARK(tp2);
        GCRE_TM_ADD(2, tp2, tp1);
      }
    }
  }
  flush();
#ifdef GCRE_IE_TIMING
  tm[5] = __builtin_amdgcn_s_memtime() - tm_begin;
  if (ap->timing && lane == 0)
    for (int i = 0; i < 6; i++) atomicAdd((unsigned long long*)ap->timing + i, (unsigned long long)tm[i]);
  if (ap->timing && lane == 0) atomicMax((unsigned long long*)ap->timing + 6, (unsigned long long)tm[5]);
#endif
}

// ------------------------------------------------------------------------------------------------
// method 1, the hot kernel.  L counter planes (multiple of 4), GZ plane groups of the added rows, OUT = the joined
// paths' planes are written out (kept joins).  Both operands have planes; lists are padded to 8 entries.
// Per joined path and tile, in the common case: 12 v_readlane, 8 mask-row loads + GZ wide loads, 14 bit ops for the
// 8-row sum, ~3.3 per plane for B + (Nz - S), 2 per plane for the interval test -- every one a single v_bitop3.
// ------------------------------------------------------------------------------------------------

template <int L, int GZ, bool OUT, bool REC>
__global__ __launch_bounds__(64 * kIeWaves) __attribute__((amdgpu_waves_per_eu(L <= 12 ? 4 : 3))) void k_null_ie_m1(const IeArgs /* read through ie_args() */) {
  // every argument is read through ap where it is used, never through the by-value copy (gcre_ie_common.h)
  const IeArgs GCRE_CONSTANT* ap = ie_args();
  // L counter planes (any even number: the arithmetic runs over exactly L); plane arrays come in groups of 4
  constexpr int LP = (L + 3) / 4 * 4;
  static_assert(L >= 8 && L <= 16 && GZ >= 2 && 4 * GZ <= LP, "planes come in groups of 4");
  // the waves' running maxima: [q][lane] per wave; touched only by the few lookups that survive the interval test
  __shared__ u32 nmax_lds[kIeWaves][32 * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u32 lane4 = (u32)lane * 4u;
  u32* nm = nmax_lds[wave] + lane;
#pragma unroll
  for (int q = 0; q < 32; q++) nm[q * 64] = 0u;
  int cur_kt = -1;
  u32 valid = 0u;
  u32 lad_base = (ap->lad_mode == 0) ? 0u : (u32)(kLadderLevels - 1 + ap->lad_mode) * (u32)ap->ladder_stride;
  bool dirty = false;     // nm holds maxima the global array has not seen
  u32 n_slow = 0u;
#ifdef GCRE_IE_TIMING
  u64 tm[6] = {0, 0, 0, 0, 0, 0};   // seg prologue, load wait, compute, lookups, exchange, total
  const u64 tm_begin = __builtin_amdgcn_s_memtime();
#endif
  __amdgpu_buffer_rsrc_t mt = __builtin_amdgcn_make_buffer_rsrc((void*)ap->mt, 0, 0x7fffffff, 0x00020000);

  // publish the wave's maxima, read everybody's, set the threshold level to the smallest running maximum of the
  // tile's live permutations (a stale read only lowers it: still exact)
  auto exchange = [&]() {
    // the tile's 2048 running maxima: lane holds 32 consecutive ones = 8 wide loads, issued together.  sc1: served
    // by the memory side, not by this CU's L1 or this XCD's L2, which never see the other XCDs' atomics.
    u32* out = ap->null_bits + (size_t)cur_kt * 2048 + lane * 32;
    __amdgpu_buffer_rsrc_t nb = __builtin_amdgcn_make_buffer_rsrc((void*)(ap->null_bits + (size_t)cur_kt * 2048), 0, 8192, 0x00020000);
    u32x4 g4[8];
#pragma unroll
    for (int j = 0; j < 8; j++) g4[j] = __builtin_amdgcn_raw_buffer_load_b128(nb, (u32)lane * 128u + (u32)j * 16u, 0, 16 /* sc1 */);
    u32 lo = 0xffffffffu;
    u32 live = valid;   // (tested here, not as 32 lane masks made when the tile changes: k_null_ie_q's merge_global)
    asm volatile("" : "+v"(live));
#pragma unroll
    for (int q = 0; q < 32; q++) {
      const u32 g = g4[q >> 2][q & 3];
      const u32 own = nm[q * 64];
      if (dirty && own > g) atomicMax(out + q, own);
      const u32 v = own > g ? own : g;
      if ((live >> q) & 1u) lo = v < lo ? v : lo;
    }
    dirty = false;
    u32 theta = __builtin_amdgcn_readfirstlane(wave_min_u32(lo));
    if (theta == 0xffffffffu) theta = 0u;
    int j = (int)(__uint_as_float(theta) * (float)kLadderPerUnit);   // level j covers thresholds >= j / kLadderPerUnit
    j = j < 0 ? 0 : (j > kLadderLevels - 1 ? kLadderLevels - 1 : j);
    lad_base = (u32)j * (u32)ap->ladder_stride;
  };
  auto flush_tile = [&]() {
    if (cur_kt >= 0) {
      u32* out = ap->null_bits + (size_t)cur_kt * 2048 + lane * 32;
#pragma unroll 8
      for (int q = 0; q < 32; q++) {
        const u32 own = nm[q * 64];
        if (own != 0u) {
          atomicMax(out + q, own);
          nm[q * 64] = 0u;
        }
      }
    }
    dirty = false;
  };

  // Work queues (WorkQueue above): segments differ in length and tiles in how many counts they look up -- a fixed
  // split of the table leaves the slowest wave 10-40 % behind the average.
  __shared__ u32 wq_state[kIeWaves][8];
  WorkQueue wq;
  wq.st = wq_state[wave];
  wq.init(ap->queue, (u32)((ap->seg_end - ap->seg_begin + ap->batch - 1) / ap->batch), (u32)ap->nkt);
  {
    wq.select(blockIdx.x & 7u);   // workgroups are dealt round the XCDs: blocks b and b + 8 share an L2
  }
  u32 ticket = wq.take(lane);
  int since = 0, period = 1;   // thresholds: refresh after 1, 2, 4, .. segments while they climb, then every kIeRefresh
  for (;;) {
    ie_args_again(ap);
    const u32 work = __builtin_amdgcn_readfirstlane(ticket);
    const u32 q_n = wq.get(2);
    if (work >= q_n) {
      // this queue is empty: take from the fullest one; every wave ends once it has seen them all empty
      if (!wq.steal(lane)) break;
      ticket = wq.take(lane);
      continue;
    }
    ticket = wq.take(lane);   // the next ticket is on its way while this batch is worked on
    const u32 item = wq.get(1) + work, nb = wq.get(3);
    const int kt = (int)(item / nb);
    const i64 s_lo = ap->seg_begin + (i64)(item - (u32)kt * nb) * ap->batch;
    const i64 s_hi = s_lo + ap->batch < ap->seg_end ? s_lo + ap->batch : ap->seg_end;
    if (kt != cur_kt) {
      flush_tile();
      cur_kt = kt;
      mt = __builtin_amdgcn_make_buffer_rsrc((void*)(ap->mt + (size_t)kt * ap->mt_rows * 64), 0, 0x7fffffff, 0x00020000);
      const int live = ap->K - kt * 2048 - lane * 32;
      valid = live >= 32 ? 0xffffffffu : (live <= 0 ? 0u : ((1u << live) - 1u));
      if (ap->lad_mode == 0) lad_base = 0u;
      since = 0;
      period = 1;
    }
    // The table entries of a segment -- (row0, first, n) and, with a recipe, the twelve words k_fill_rec_segs gathered
    // for it -- are wave-uniform.  Inside a batch they are fetched one segment ahead into one VGPR (lane l = word l)
    // and moved to scalar registers with v_readlane when their turn comes: the first segment of a batch pays the
    // scalar-load round trip, the others start their plane loads at once.
    u32 nextv = 0u;
    bool have_next = false;
    for (i64 sidx = s_lo; sidx < s_hi; sidx++) {
      ie_args_again(ap);
      u32 row0, first, npaths;
      u32 rc_a = 0u, rc_z = 0u, rc_info = 0u, rc_lov = 0u;
      typedef u32 __attribute__((ext_vector_type(8))) u32x8;
      u32x8 rc_o = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      if (have_next) {
        row0 = rdlane(nextv, 0);
        first = rdlane(nextv, 1);
        npaths = rdlane(nextv, 2);
        if constexpr (REC) {
          rc_a = rdlane(nextv, 4);
          rc_z = rdlane(nextv, 5);
          rc_info = rdlane(nextv, 6);
          rc_lov = rdlane(nextv, 7);
#pragma unroll
          for (int j = 0; j < 8; j++) rc_o[j] = rdlane(nextv, 8 + j);
        }
      } else {
        const SparseSeg GCRE_CONSTANT* segs = (const SparseSeg GCRE_CONSTANT*)ap->segs;
        row0 = segs[sidx].row0;
        first = segs[sidx].first;
        npaths = segs[sidx].n;
        if constexpr (REC) {
          const u32 GCRE_CONSTANT* rs = (const u32 GCRE_CONSTANT*)ap->rec_segs + (u64)sidx * kRecSegWords;
          rc_a = rs[0];
          rc_z = rs[1];
          rc_info = rs[2];
          rc_lov = rs[3];
          rc_o = *(const u32x8 GCRE_CONSTANT*)(rs + 4);
        }
      }
      have_next = sidx + 1 < s_hi;
      if (have_next) {
        const u32* src = (const u32*)ap->segs + (u64)(sidx + 1) * 3u + (u32)(lane < 3 ? lane : 0);
        if constexpr (REC) {
          if (lane >= 4 && lane < 16) src = ap->rec_segs + (u64)(sidx + 1) * kRecSegWords + (u32)(lane - 4);
        }
        nextv = *src;
      }
      GCRE_TM_MARK(ts0);
      if (ap->lad_mode == 0 && ++since >= period) {
        exchange();
        since = 0;
        period = period < kIeRefresh ? period * 2 : kIeRefresh;
      }
      GCRE_TM_MARK(ts1);
      GCRE_TM_ADD(4, ts1, ts0);

      // ---- per-path metadata of the whole segment in a few coalesced loads: lane t <-> joined path first + t ----
      const u32 qv = first + (((u32)lane < npaths) ? (u32)lane : 0u);
      const u32 infov = ap->linfo[qv];                 // padded list length | mode
      const u32 lovv = ap->lover[qv];                  // where a long list continues
      const u32 zunit = ((u32)kt * (u32)ap->rowsz + (ap->rowz[qv] & 0x7fffffffu)) * (u32)ap->gz;   // 1 KB units into planesz
      const u32 totv = ap->tot[qv];
      // segments of another shard's rows: the all-inside row of the ladder (no count is looked up), planes only
      const u32 lhv = ap->ladder[((u64)sidx < (u64)ap->score_segs ? lad_base : (u32)kLadderLevels * (u32)ap->ladder_stride) + totv];
      // the first 8 entries of every list (lists are padded to 8: most lists end there) are wave-uniform: they come
      // through the scalar cache, one s_load_dwordx8 per path, fetched one path ahead of the loads that use them
      const u32x8 GCRE_CONSTANT* slots = (const u32x8 GCRE_CONSTANT*)(ap->dlist + (u64)first * 8u);
      // OUT (every count is needed): the path's 8 mask rows and the added row's planes.  Otherwise only the planes: the
      // rows are fetched by the lanes the bound filter leaves uncertain (see compute)
      auto issue = [&](u32 t2, const u32x8 offs, u32 (&yy)[8], u32 (&ZZ)[4 * GZ]) {
        if constexpr (OUT) {
#pragma unroll
          for (int j = 0; j < 8; j++) yy[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, offs[j], 0);
        }
        // scalar base + 32-bit lane offset: the address never sits in vector registers (a vector address pair that shares
        // registers with a load still in flight costs a full s_waitcnt vmcnt(0) per path)
        __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)ap->planesz + (u64)rdlane(zunit, t2) * 1024u), 0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int j = 0; j < GZ; j++) {
          const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rz, lane4 * 4u + (u32)j * 1024u, 0, 0);
          ZZ[4 * j + 0] = v.x; ZZ[4 * j + 1] = v.y; ZZ[4 * j + 2] = v.z; ZZ[4 * j + 3] = v.w;
        }
      };
      // the first path's loads do not depend on the base counters: they go out before those are read (and, with a
      // recipe, rebuilt), one round trip earlier
      u32 yA[8], yB[8], ZA[4 * GZ], ZB[4 * GZ];
      const u32 last = npaths - 1u;
      auto at = [&](u32 t2) -> u32 { return t2 < last ? t2 : last; };
      u32x8 oA = slots[0], oB = slots[at(1u)];
      issue(0u, oA, yA, ZA);
      // ---- base counters: the planes of paths0[row0] -- stored, or (REC) rebuilt from the recipe of the join that
      // produced the row: planes of ITS paths0 row + planes of the row it added -/+ its 8-entry list ----
      u32 B[LP];
      auto load_groups = [&](u32 (&P)[LP], const u32* planes, u64 unit, int groups) {
        const u32x4* src = (const u32x4*)(planes + unit * 256u) + lane;
#pragma unroll
        for (int j = 0; j < LP / 4; j++) {
          u32x4 v = {0u, 0u, 0u, 0u};
          if (j < groups) v = src[j * 64];
          P[4 * j + 0] = v.x; P[4 * j + 1] = v.y; P[4 * j + 2] = v.z; P[4 * j + 3] = v.w;
        }
      };
      if constexpr (!REC) {
        load_groups(B, ap->planes0, ((u64)kt * (u64)ap->rows0 + (u64)row0) * (u64)ap->g0, ap->g0);
      } else {
        const u32 ra = rc_a, rz = rc_z & 0x7fffffffu, rinfo = rc_info;
        const u32x8 ro = rc_o;
        u32 yr[8];
#pragma unroll
        for (int j = 0; j < 8; j++) yr[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, ro[j], 0);
        u32 ZR[LP];
        load_groups(B, ap->rec_planes_a, ((u64)kt * (u64)ap->rec_rows_a + (u64)ra) * (u64)ap->rec_ga, ap->rec_ga);
        load_groups(ZR, ap->rec_planes_z, ((u64)kt * (u64)ap->rec_rows_z + (u64)rz) * (u64)ap->rec_gz, ap->rec_gz);
        u32 S[L];
        {
          u32 S4[4];
          sum8(yr, S4);
#pragma unroll
          for (int l = 0; l < L; l++) S[l] = (l < 4) ? S4[l < 4 ? l : 0] : 0u;
        }
        const u32 rlen = linfo_len(rinfo);
        if (rlen > 8u) {   // the producing join's list was long: the rest of it, 8 entries at a time
          const u32 GCRE_CONSTANT* more = (const u32 GCRE_CONSTANT*)(ap->rec_over + rc_lov);
          for (u32 p = 0u; p + 8u < rlen; p += 8u) {
            const u32x8 o8 = *(const u32x8 GCRE_CONSTANT*)(more + p);
            u32 yy[8], s4[4];
#pragma unroll
            for (int j = 0; j < 8; j++) yy[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, o8[j], 0);
            sum8(yy, s4);
            u32 cy = 0u;
#pragma unroll
            for (int l = 0; l < L; l++) {
              const u32 sv = S[l];
              const u32 add = (l < 4) ? s4[l < 4 ? l : 0] : 0u;
              S[l] = xor3(sv, add, cy);
              cy = majority(sv, add, cy);
            }
          }
        }
        if (linfo_overlap(rinfo)) {   // B = A + Z - S
          u32 cy = 0u, bw = 0u;
#pragma unroll
          for (int l = 0; l < L; l++) {
            const u32 s1_ = xor3(B[l], ZR[l], cy);
            cy = majority(B[l], ZR[l], cy);
            B[l] = xor3(s1_, S[l], bw);
            bw = borrow3(s1_, S[l], bw);
          }
        } else {            // B = A + S
          u32 cy = 0u;
#pragma unroll
          for (int l = 0; l < L; l++) {
            const u32 bl = B[l];
            B[l] = xor3(bl, S[l], cy);
            cy = majority(bl, S[l], cy);
          }
        }
      }

      GCRE_TM_MARK(ts2);
      GCRE_TM_ADD(0, ts2, ts1);
      // ---- the joined paths of the segment, software-pipelined one path ahead: the 8 mask rows and the planes of
      // path t+1 are in flight while path t is computed.  Loads are issued unconditionally (the last path is simply
      // requested twice) so that the compiler's counters let the older loads retire without draining the younger.
      auto compute = [&](u32 t, const u32 (&y)[8], const u32 (&Z)[4 * GZ]) {
        GCRE_TM_MARK(tp0);
        const u32 r0 = rdlane(infov, t);
        const u32 len = linfo_len(r0);
        const bool overlap = linfo_overlap(r0);
        u32 C[L];
        u32 S4[4];
        sum8(y, S4);
        if (len <= 8u && overlap) {
          // ---- C = B + (Nz - S): the common case.  Nz - S >= 0: the overlap is part of the added row ----
          u32 T[4 * GZ];
          u32 bw = 0u;
#pragma unroll
          for (int l = 0; l < 4 * GZ; l++) {
            if (l < 4) {
              T[l] = xor3(Z[l], S4[l < 4 ? l : 0], bw);
              bw = borrow3(Z[l], S4[l < 4 ? l : 0], bw);
            } else {
              T[l] = Z[l] ^ bw;
              bw = bw & ~Z[l];
            }
          }
          u32 cy = 0u;
#pragma unroll
          for (int l = 0; l < L; l++) {
            if (l < 4 * GZ) {
              C[l] = xor3(B[l], T[l < 4 * GZ ? l : 0], cy);
              cy = majority(B[l], T[l < 4 * GZ ? l : 0], cy);
            } else {
              C[l] = B[l] ^ cy;
              cy = B[l] & cy;
            }
          }
        } else if (len <= 8u) {
          // ---- C = B + S: the join adds at most 8 patients ----
          u32 cy = 0u;
#pragma unroll
          for (int l = 0; l < L; l++) {
            if (l < 4) {
              C[l] = xor3(B[l], S4[l < 4 ? l : 0], cy);
              cy = majority(B[l], S4[l < 4 ? l : 0], cy);
            } else {
              C[l] = B[l] ^ cy;
              cy = B[l] & cy;
            }
          }
        } else {
          // ---- long list (rare): further blocks of 8 entries, each summed and rippled into a full-width S ----
          u32 S[L];
#pragma unroll
          for (int l = 0; l < L; l++) S[l] = (l < 4) ? S4[l < 4 ? l : 0] : 0u;
          const u32 GCRE_CONSTANT* more = (const u32 GCRE_CONSTANT*)(ap->dover + rdlane(lovv, t));
          for (u32 p = 0u; p + 8u < len; p += 8u) {
            const u32x8 o8 = *(const u32x8 GCRE_CONSTANT*)(more + p);
            u32 yy[8], s4[4];
#pragma unroll
            for (int j = 0; j < 8; j++) yy[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, o8[j], 0);
            sum8(yy, s4);
            u32 cy = 0u;
#pragma unroll
            for (int l = 0; l < L; l++) {
              const u32 sv = S[l];
              if (l < 4) {
                S[l] = xor3(sv, s4[l < 4 ? l : 0], cy);
                cy = majority(sv, s4[l < 4 ? l : 0], cy);
              } else {
                S[l] = sv ^ cy;
                cy = sv & cy;
              }
            }
          }
          if (overlap) {   // C = B + Nz - S
            u32 cy = 0u, bw = 0u;
#pragma unroll
            for (int l = 0; l < L; l++) {
              const u32 zl = (l < 4 * GZ) ? Z[l < 4 * GZ ? l : 0] : 0u;
              const u32 s1_ = xor3(B[l], zl, cy);
              cy = majority(B[l], zl, cy);
              C[l] = xor3(s1_, S[l], bw);
              bw = borrow3(s1_, S[l], bw);
            }
          } else {         // C = B + S
            u32 cy = 0u;
#pragma unroll
            for (int l = 0; l < L; l++) {
              C[l] = xor3(B[l], S[l], cy);
              cy = majority(B[l], S[l], cy);
            }
          }
        }
        if constexpr (OUT) {
          const u64 rh = (u64)ap->out_first + first + t;
          u32x4* dst = (u32x4*)(ap->planes_out + (((u64)kt * (u64)ap->rows_out + rh) * (u64)ap->go) * 256u) + lane;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            if (j < ap->go) {
              u32x4 v = {0u, 0u, 0u, 0u};
              if (4 * j < L) v = u32x4{C[(4 * j) % L], (4 * j + 1 < L) ? C[(4 * j + 1) % L] : 0u, (4 * j + 2 < L) ? C[(4 * j + 2) % L] : 0u,
                                       (4 * j + 3 < L) ? C[(4 * j + 3) % L] : 0u};
              dst[j * 64] = v;
            }
          }
        }
        // ---- interval test: live permutations whose count lies outside [lo, hi] of the path's diagonal ----
        const u32 lh = rdlane(lhv, t);
        const u32 lo = lh & 0xffffu, hi = lh >> 16;
        u32 blo = 0u, bhi = 0u;
#pragma unroll
        for (int l = 0; l < L; l++) {
          const u32 kl = (u32)__builtin_amdgcn_sbfe((int)lo, l, 1);   // scalar: all ones when the bound has bit l
          const u32 kh = (u32)__builtin_amdgcn_sbfe((int)hi, l, 1);
          blo = borrow3(C[l], kl, blo);    // C - lo borrows  <=>  C < lo
          bhi = borrow3(kh, C[l], bhi);    // hi - C borrows  <=>  C > hi
        }
        u32 m = (blo | bhi) & valid;
        GCRE_TM_MARK(tp2);
        GCRE_TM_ADD(2, tp2, tp0);
        if (__builtin_amdgcn_ballot_w64(m != 0u) == 0ull) return;
        // ---- the few permutations that can raise a maximum: rebuild each count from the planes, look it up ----
        n_slow++;
        const u32* diag_g = (const u32*)ap->t32 + sp_diag_offset(rdlane(totv, t));
        while (m != 0u) {
          // up to 4 permutations per round: their table cells are independent loads in flight together
          u32 bb[4], vv[4];
#pragma unroll
          for (int k = 0; k < 4; k++) {
            bb[k] = m ? (u32)__builtin_ctz(m) : bb[k ? k - 1 : 0];   // exhausted: repeat the last one (max is idempotent)
            m &= m - 1u;
            u32 cnt = 0u;
#pragma unroll
            for (int l = 0; l < L; l++) cnt |= ((C[l] >> bb[k]) & 1u) << l;
            vv[k] = diag_g[cnt];
          }
#pragma unroll
          for (int k = 0; k < 4; k++)
            __hip_atomic_fetch_max(nm + bb[k] * 64, vv[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);   // ds_max_u32
        }
        dirty = true;
        GCRE_TM_MARK(tp3);
        GCRE_TM_ADD(3, tp3, tp2);
      };

      // ---- !OUT: the bound filter.  count = W - S with W = B + Nz known from the planes alone and 0 <= S <= ov, the
      // length of the path's overlap list.  A permutation with lo + ov <= W <= hi has its count inside [lo, hi] whatever
      // its S is: it cannot raise a maximum, and its 8 mask rows need not be read.  Only the lanes that hold a permutation
      // outside that narrower interval fetch the rows (exec-masked loads), finish the count and test it exactly; what
      // still falls outside [lo, hi] is looked up as before.  ~3/4 of the path-tiles end after 2 plane loads and ~45 bit
      // instructions.  (Delta lists -- rare since the inspector prefers overlap lists -- skip the filter.)
      auto compute_f = [&](u32 t, const u32 (&Z)[4 * GZ]) {
        const u32 r0 = rdlane(infov, t);
        const u32 len = linfo_len(r0);
        const bool overlap = linfo_overlap(r0);
        const u32 ov = len - linfo_pad(r0);   // the list's true length
        const u32 lh = rdlane(lhv, t);
        const u32 lo = lh & 0xffffu, hi = lh >> 16;
        u32 W[L];
        u32 mu = valid;
        if (overlap) {
          u32 cy = 0u;
#pragma unroll
          for (int l = 0; l < L; l++) {
            if (l < 4 * GZ) {
              W[l] = xor3(B[l], Z[l < 4 * GZ ? l : 0], cy);
              cy = majority(B[l], Z[l < 4 * GZ ? l : 0], cy);
            } else {
              W[l] = B[l] ^ cy;
              cy = B[l] & cy;
            }
          }
          u32 lo2 = lo ? lo + ov : 0u;            // counts are never negative: lo = 0 needs no margin
          lo2 = lo2 > 0xffffu ? 0xffffu : lo2;
          u32 blo = 0u, bhi = 0u;
#pragma unroll
          for (int l = 0; l < L; l++) {
            const u32 kl = (u32)__builtin_amdgcn_sbfe((int)lo2, l, 1);
            const u32 kh = (u32)__builtin_amdgcn_sbfe((int)hi, l, 1);
            blo = borrow3(W[l], kl, blo);    // W < lo + ov
            bhi = borrow3(kh, W[l], bhi);    // W > hi
          }
          if ((lo2 >> L) != 0u) blo = 0xffffffffu;   // the margin pushed the bound past the counters' range
          // W = N0 + Nz can pass 2^L although no count of the path does (the planes are sized for the largest carrier total
          // of the joined paths, and W counts the overlap twice): a carry out of the top plane is "above hi", not a small W
          mu = (blo | bhi | cy) & valid;
        } else {
#pragma unroll
          for (int l = 0; l < L; l++) W[l] = B[l];
        }
        if (__builtin_amdgcn_ballot_w64(mu != 0u) == 0ull) return;
#ifdef GCRE_IE_TIMING
        tm[1] += 1;                                                            // path-tiles the filter left uncertain
        tm[3] += (u64)__popcll(__builtin_amdgcn_ballot_w64(mu != 0u));         // ... and the lanes that fetched rows
#endif
        u32 slow = 0u;
        const u32x8 o = slots[t];
        if (mu != 0u) {
          // ---- the uncertain lanes: rows, exact count, exact test ----
          u32 y[8], S4[4];
#pragma unroll
          for (int j = 0; j < 8; j++) y[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, o[j], 0);
          sum8(y, S4);
          u32 S[L];
#pragma unroll
          for (int l = 0; l < L; l++) S[l] = (l < 4) ? S4[l < 4 ? l : 0] : 0u;
          if (len > 8u) {   // long list: further blocks of 8 entries
            const u32 GCRE_CONSTANT* more = (const u32 GCRE_CONSTANT*)(ap->dover + rdlane(lovv, t));
            for (u32 p = 0u; p + 8u < len; p += 8u) {
              const u32x8 o8 = *(const u32x8 GCRE_CONSTANT*)(more + p);
              u32 yy[8], s4[4];
#pragma unroll
              for (int j = 0; j < 8; j++) yy[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, o8[j], 0);
              sum8(yy, s4);
              u32 cy = 0u;
#pragma unroll
              for (int l = 0; l < L; l++) {
                const u32 sv = S[l];
                if (l < 4) {
                  S[l] = xor3(sv, s4[l < 4 ? l : 0], cy);
                  cy = majority(sv, s4[l < 4 ? l : 0], cy);
                } else {
                  S[l] = sv ^ cy;
                  cy = sv & cy;
                }
              }
            }
          }
          u32 C[L];
          if (overlap) {   // C = W - S
            u32 bw = 0u;
#pragma unroll
            for (int l = 0; l < L; l++) {
              C[l] = xor3(W[l], S[l], bw);
              bw = borrow3(W[l], S[l], bw);
            }
          } else {         // C = B + S
            u32 cy = 0u;
#pragma unroll
            for (int l = 0; l < L; l++) {
              C[l] = xor3(W[l], S[l], cy);
              cy = majority(W[l], S[l], cy);
            }
          }
          u32 blo = 0u, bhi = 0u;
#pragma unroll
          for (int l = 0; l < L; l++) {
            const u32 kl = (u32)__builtin_amdgcn_sbfe((int)lo, l, 1);
            const u32 kh = (u32)__builtin_amdgcn_sbfe((int)hi, l, 1);
            blo = borrow3(C[l], kl, blo);
            bhi = borrow3(kh, C[l], bhi);
          }
          u32 m = (blo | bhi) & mu;
          if (m != 0u) {
            slow = 1u;
            const u32* diag_g = (const u32*)ap->t32 + sp_diag_offset(rdlane(totv, t));
            while (m != 0u) {
              u32 bb[4], vv[4];
#pragma unroll
              for (int k = 0; k < 4; k++) {
                bb[k] = m ? (u32)__builtin_ctz(m) : bb[k ? k - 1 : 0];
                m &= m - 1u;
                u32 cnt = 0u;
#pragma unroll
                for (int l = 0; l < L; l++) cnt |= ((C[l] >> bb[k]) & 1u) << l;
                vv[k] = diag_g[cnt];
              }
#pragma unroll
              for (int k = 0; k < 4; k++)
                __hip_atomic_fetch_max(nm + bb[k] * 64, vv[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);   // ds_max_u32
            }
          }
        }
        if (__builtin_amdgcn_ballot_w64(slow != 0u) != 0ull) {
          n_slow++;
          dirty = true;
        }
      };

      if constexpr (OUT) {
        for (u32 t = 0; t < npaths; t += 2) {
          issue(at(t + 1), oB, yB, ZB);
          oA = slots[at(t + 2)];
          compute(t, yA, ZA);
          if (t + 1 < npaths) {
            issue(at(t + 2), oA, yA, ZA);
            oB = slots[at(t + 3)];
            compute(t + 1, yB, ZB);
          }
        }
      } else {
        // a filtered path is ~60 instructions: one path of work does not cover a plane load's latency, so the planes are
        // requested TWO paths ahead (three buffers in rotation).  The list entries are only read by the few paths that
        // fetch rows.
        u32 ZC[4 * GZ];
        issue(at(1u), oB, yB, ZB);
        for (u32 t = 0; t < npaths; t += 3) {
          issue(at(t + 2), oA, yA, ZC);
          compute_f(t, ZA);
          if (t + 1 < npaths) {
            issue(at(t + 3), oA, yA, ZA);
            compute_f(t + 1, ZB);
          }
          if (t + 2 < npaths) {
            issue(at(t + 4), oA, yA, ZB);
            compute_f(t + 2, ZC);
          }
        }
      }
    }
  }
  flush_tile();
#ifdef GCRE_IE_TIMING
  tm[5] = __builtin_amdgcn_s_memtime() - tm_begin;
  if (ap->timing && lane == 0)
    for (int i = 0; i < 6; i++) atomicAdd((unsigned long long*)ap->timing + i, (unsigned long long)tm[i]);
  if (ap->timing && lane == 0) atomicMax((unsigned long long*)ap->timing + 6, (unsigned long long)tm[5]);
#endif
  if (ap->stats && lane == 0 && n_slow) atomicAdd(ap->stats, n_slow);
}

// method 2 runs the general kernel; method 1 the specialised one: L from the largest carrier total, GZ = plane groups of
// the added rows that can be non-zero (<= L/4), OUT = planes of the joined paths wanted
#define GCRE_IE_M2(EXPR)                    \
  if (planes <= 8) { EXPR(2, 8); }          \
  else if (planes <= 12) { EXPR(2, 12); }   \
  else { EXPR(2, 16); }

#define GCRE_IE_M1_OR(EXPR, LL, GG)                                                  \
  if (out) { if (rec) { EXPR(LL, GG, true, true); } else { EXPR(LL, GG, true, false); } }   \
  else { if (rec) { EXPR(LL, GG, false, true); } else { EXPR(LL, GG, false, false); } }

#define GCRE_IE_M1(EXPR)                                                     \
  if (planes <= 8) { GCRE_IE_M1_OR(EXPR, 8, 2) }                             \
  else if (planes <= 10) {                                                   \
    if (gz <= 2) { GCRE_IE_M1_OR(EXPR, 10, 2) } else { GCRE_IE_M1_OR(EXPR, 10, 3) }        \
  } else if (planes <= 12) {                                                 \
    if (gz <= 2) { GCRE_IE_M1_OR(EXPR, 12, 2) } else { GCRE_IE_M1_OR(EXPR, 12, 3) }        \
  } else {                                                                   \
    if (gz <= 2) { GCRE_IE_M1_OR(EXPR, 16, 2) }                              \
    else if (gz == 3) { GCRE_IE_M1_OR(EXPR, 16, 3) }                         \
    else { GCRE_IE_M1_OR(EXPR, 16, 4) }                                      \
  }

#define GCRE_IE_GEN(EXPR)                                          \
  if (method == 1) {                                               \
    if (planes <= 8) { EXPR(1, 8); }                               \
    else if (planes <= 12) { EXPR(1, 12); }                        \
    else { EXPR(1, 16); }                                          \
  } else {                                                         \
    GCRE_IE_M2(EXPR)                                               \
  }

// general = true: the general kernel (both methods; method 1 then looks every count up -- the warm-up slice that seeds
// the thresholds, and joins too small for pruning to pay)
// Per segment of a launch whose paths0 rows come with a recipe: the recipe entries of the segment's row, gathered
// next to the segment table (kRecSegWords words: paths0 row of the producing join, row it added, list info, where a
// long list continues, the list's first 8 entries) so that the pruned kernel needs no load that depends on row0.
__global__ __launch_bounds__(256) void k_fill_rec_segs(const SparseSeg* segs, i64 nsegs, const u32* r_row0, const u32* r_rowz,
                                                       const u32* r_linfo, const u32* r_lover, const u32* r_slot, const u32* r_tot,
                                                       u32* out, u32* queue) {
  const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (queue && t < 8 * 16) queue[t] = 0u;   // the ticket counters of the pruned launch behind this gather
  const i64 sidx = t >> 2;
  const int part = (int)(t & 3);   // four threads per segment: the four scalars, then the slot in two halves
  if (sidx >= nsegs) return;
  const u32 row0 = segs[sidx].row0;
  u32* o = out + sidx * kRecSegWords;
  if (part == 0) {
    o[0] = r_row0[row0];
    o[1] = r_rowz[row0];
  } else if (part == 1) {
    u32 info = r_linfo[row0];
    u32 need = 3u;   // plane groups of the row that can be non-zero, minus one: ceil(bits(carriers) / 4) - 1
    if (r_tot) {
      const u32 t = r_tot[row0];
      need = t < 16u ? 0u : (t < 256u ? 1u : (t < 4096u ? 2u : 3u));
    }
    o[2] = linfo_with_groups(info, need);
    o[3] = r_lover[row0];
  } else {
    const u32x4 v = *(const u32x4*)(r_slot + (u64)row0 * 8u + (part - 2) * 4);
    *(u32x4*)(o + 4 + (part - 2) * 4) = v;
  }
}

hipError_t launch_fill_rec_segs(const SparseSeg* segs, int64_t nsegs, const uint32_t* r_row0, const uint32_t* r_rowz,
                                const uint32_t* r_linfo, const uint32_t* r_lover, const uint32_t* r_slot, const uint32_t* r_tot,
                                uint32_t* out, uint32_t* queue, hipStream_t stream) {
  if (nsegs == 0) return hipSuccess;
  const i64 blocks = (nsegs * 4 + 255) / 256;
  hipLaunchKernelGGL(k_fill_rec_segs, dim3((unsigned)blocks), dim3(256), 0, stream, segs, nsegs, r_row0, r_rowz, r_linfo, r_lover,
                     r_slot, r_tot, out, queue);
  return hipGetLastError();
}

hipError_t launch_null_ie(const IeArgs& a, int method, int planes, bool general, hipStream_t stream) {
  const dim3 grid((unsigned)(8 * a.waves_per_xcd / kIeWaves));
  const dim3 block(64 * kIeWaves);
  if (method == 1 && !general) {
    const int gz = a.gz;
    const bool out = a.planes_out != nullptr;
    const bool rec = a.rec_slot != nullptr;
#define GCRE_LAUNCH(LL, GG, OO, RR) hipLaunchKernelGGL((k_null_ie_m1<LL, GG, OO, RR>), grid, block, 0, stream, a)
    GCRE_IE_M1(GCRE_LAUNCH)
#undef GCRE_LAUNCH
  } else if (method == 2 && !general) {
    return launch_null_ie_m2(a, planes, stream);
  } else {
    if (a.waves_per_xcd < kIeWaves || a.waves_per_xcd % kIeWaves != 0) return hipErrorInvalidValue;   // whole blocks per XCD: work is dealt by block
#define GCRE_LAUNCH(MM, LL) hipLaunchKernelGGL((k_null_ie<MM, LL>), grid, block, 0, stream, a)
    GCRE_IE_GEN(GCRE_LAUNCH)
#undef GCRE_LAUNCH
  }
  return hipGetLastError();
}

int ie_max_waves_per_cu(int method, int planes, int gz, bool out, bool rec) {
  int blocks = 0;
  hipError_t e = hipSuccess;
  if (method == 1) {
#define GCRE_OCC(LL, GG, OO, RR) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_null_ie_m1<LL, GG, OO, RR>, 64 * kIeWaves, 0)
    GCRE_IE_M1(GCRE_OCC)
#undef GCRE_OCC
  } else {
    return ie2_max_waves_per_cu(planes, gz, out, rec);
  }
  if (e != hipSuccess || blocks < 1) blocks = 1;
  return blocks * kIeWaves;
}

// ------------------------------------------------------------------------------------------------
// count planes of a path set from its bit lists: one wave per (row-half, tile)
// ------------------------------------------------------------------------------------------------
template <int L>
__global__ __launch_bounds__(256) void k_build_planes(const u32* mt_all, u32 mt_rows, int nkt, const u64* loff,
                                                      const u32* lidx, i64 nrowhalves, int groups, u32* planes) {
  const int lane = threadIdx.x & 63;
  const i64 wave = (i64)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform
  const i64 nwaves = (i64)gridDim.x * 4;
  const u32 lane4 = (u32)lane * 4u;
  const u64 GCRE_CONSTANT* off = (const u64 GCRE_CONSTANT*)loff;
  const u32 GCRE_CONSTANT* list = (const u32 GCRE_CONSTANT*)lidx;
  const i64 items = nrowhalves * nkt;
  // tile-major so that concurrently running waves share a mask tile in L2
  for (i64 it = wave; it < items; it += nwaves) {
    const i64 w = it / nrowhalves;   // tile
    const i64 rr = it - w * nrowhalves;
    __amdgpu_buffer_rsrc_t mt = __builtin_amdgcn_make_buffer_rsrc((void*)(mt_all + (size_t)w * mt_rows * 64), 0, 0x7fffffff, 0x00020000);
    u32 P[L];
#pragma unroll
    for (int l = 0; l < L; l++) P[l] = 0u;
    u64 p = off[rr];
    const u64 e = off[rr + 1];
    u32 x[16];
    for (; p + 16 <= e; p += 16) {
      load16(x, mt, lane4, *(const u32x16 GCRE_CONSTANT*)(list + p));
      add16<L>(P, x);
    }
    for (; p < e; p += 4) {
      const u32x4 offs = *(const u32x4 GCRE_CONSTANT*)(list + p);
      u32 y[4];
#pragma unroll
      for (int j = 0; j < 4; j++) y[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, offs[j], 0);
      add4<L>(P, y);
    }
    u32x4* dst = (u32x4*)(planes + (((u64)w * (u64)nrowhalves + (u64)rr) * (u64)groups) * 256u) + lane;
#pragma unroll
    for (int j = 0; j < L / 4; j++)
      if (j < groups) dst[j * 64] = u32x4{P[4 * j], P[4 * j + 1], P[4 * j + 2], P[4 * j + 3]};
  }
}

hipError_t launch_build_planes(const uint32_t* mt, uint32_t mt_rows, int nkt, const uint64_t* loff, const uint32_t* lidx,
                               int64_t nrowhalves, int groups, uint32_t* planes, hipStream_t stream) {
  const i64 items = nrowhalves * nkt;
  if (items == 0) return hipSuccess;
  const i64 blocks = (items + 3) / 4;
  const dim3 grid((unsigned)(blocks < 256 * 8 ? blocks : 256 * 8)), block(256);
  if (groups <= 2) hipLaunchKernelGGL(k_build_planes<8>, grid, block, 0, stream, mt, mt_rows, nkt, loff, lidx, nrowhalves, groups, planes);
  else if (groups == 3) hipLaunchKernelGGL(k_build_planes<12>, grid, block, 0, stream, mt, mt_rows, nkt, loff, lidx, nrowhalves, groups, planes);
  else hipLaunchKernelGGL(k_build_planes<16>, grid, block, 0, stream, mt, mt_rows, nkt, loff, lidx, nrowhalves, groups, planes);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// pruning ladder of the method-1 null table: for every diagonal t and threshold level j the largest interval
// [lo, hi] around the diagonal's minimum on which T32[t][c] <= j / kLadderPerUnit.  Entry = hi << 16 | lo;
// an empty interval is lo = 1, hi = 0 (every count is "outside").  Valid for ANY table: cells outside the interval
// are simply looked up.
// ------------------------------------------------------------------------------------------------
// One wave per diagonal.  A cell c with value d[c] blocks the levels j with j/kLadderPerUnit < d[c], i.e. j < J(c) =
// ceil(kLadderPerUnit * d[c]); the interval of level j ends next to the nearest blocking cell on either side of the
// diagonal's (first) minimum c0:  lo_j = 1 + max{c < c0 : J(c) > j},  hi_j = min{c > c0 : J(c) > j} - 1.
__global__ __launch_bounds__(64) void k_build_ladder(const u32* t32, int TD, u32* ladder) {
  __shared__ int left[kLadderLevels + 2], right[kLadderLevels + 2];
  const int t = blockIdx.x;
  const int lane = threadIdx.x;
  if (t >= TD) return;
  const u32* d = t32 + sp_diag_offset((u32)t);
  for (int k = lane; k < kLadderLevels + 2; k += 64) {
    left[k] = -1;
    right[k] = t + 1;
  }
  // first minimum of the diagonal (values are bit patterns of non-negative floats: they order like the floats)
  u64 mine = ~(u64)0;
  for (int c = lane; c <= t; c += 64) {
    const u64 key = ((u64)d[c] << 32) | (u32)c;
    mine = key < mine ? key : mine;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 other = ((u64)(u32)__shfl_xor((int)(mine >> 32), o, 64) << 32) | (u32)__shfl_xor((int)(u32)mine, o, 64);
    mine = other < mine ? other : mine;
  }
  const u32 best = (u32)(mine >> 32);
  const int c0 = (int)(u32)mine;
  __syncthreads();
  auto blocked_below = [](u32 bits) -> int {   // J: number of levels whose threshold is below the value
    const float v = __uint_as_float(bits);
    if (!(v > 0.0f)) return 0;
    const float x = v * (float)kLadderPerUnit;
    if (x >= (float)kLadderLevels) return kLadderLevels;
    const int j = (int)x;                        // thresholds j/8 are exact in f32, and so is x = 8 v
    return ((float)j < x) ? j + 1 : j;
  };
  for (int c = lane; c <= t; c += 64) {
    if (c == c0) continue;
    const int J = blocked_below(d[c]);
    if (J == 0) continue;
    if (c < c0) atomicMax(&left[J], c);
    else atomicMin(&right[J], c);
  }
  __syncthreads();
  if (lane == 0) {   // suffix max / min over J: a cell with J blocks every level below J
    int l = -1, r = t + 1;
    for (int k = kLadderLevels; k >= 0; k--) {
      l = left[k] > l ? left[k] : l;
      r = right[k] < r ? right[k] : r;
      left[k] = l;
      right[k] = r;
    }
  }
  __syncthreads();
  const int Jbest = blocked_below(best);
  for (int j = lane; j < kLadderLevels; j += 64) {
    // level j is blocked by cells with J > j: left[j + 1] / right[j + 1] after the suffix pass
    u32 e = 1u;   // lo = 1, hi = 0: empty
    if (Jbest <= j) e = ((u32)(right[j + 1] - 1) << 16) | (u32)(left[j + 1] + 1);
    ladder[(size_t)j * TD + t] = e;
  }
  if (lane == 0) {
    // two constant rows behind the levels: "every count is inside" (nothing is looked up: planes-only launches) and
    // "every count is outside" (everything is looked up: GCRE_IE_PRUNE=0)
    ladder[(size_t)kLadderLevels * TD + t] = 0xffff0000u;
    ladder[(size_t)(kLadderLevels + 1) * TD + t] = 1u;
  }
}

hipError_t launch_build_ladder(const float* t32, int TD, uint32_t* ladder, hipStream_t stream) {
  hipLaunchKernelGGL(k_build_ladder, dim3((unsigned)TD), dim3(64), 0, stream, (const u32*)t32, TD, ladder);
  return hipGetLastError();
}

// The signed method's ladder: same construction on the f64 vtmax diagonals at HALF the threshold of each level
// (row r: the interval on which vtmax <= r / (2 * kLadderPerUnit), kLadder2Levels rows), see k_null_ie_m2.
__global__ __launch_bounds__(64) void k_build_ladder2(const double* dmax, int TD, u32* ladder) {
  __shared__ int left[kLadder2Levels + 2], right[kLadder2Levels + 2];
  const int t = blockIdx.x;
  const int lane = threadIdx.x;
  if (t >= TD) return;
  const double* d = dmax + sp_diag_offset((u32)t);
  for (int k = lane; k < kLadder2Levels + 2; k += 64) {
    left[k] = -1;
    right[k] = t + 1;
  }
  // first minimum of the diagonal
  double bestv = __builtin_inf();
  int bestc = 0x7fffffff;
  for (int c = lane; c <= t; c += 64) {
    const double v = d[c];
    if (v < bestv || (v == bestv && c < bestc) || (bestc == 0x7fffffff)) {
      if (!(v != v)) { bestv = v; bestc = c; }
      else if (bestc == 0x7fffffff) { bestv = __builtin_inf(); bestc = c; }   // NaN cells never count as a minimum
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bestv, o, 64);
    const int oc = __shfl_xor(bestc, o, 64);
    if (ov < bestv || (ov == bestv && oc < bestc)) { bestv = ov; bestc = oc; }
  }
  const int c0 = bestc;
  __syncthreads();
  auto blocked_below = [](double v) -> int {   // number of levels whose half threshold j / 16 is below the value
    if (v != v) return kLadder2Levels;          // NaN: never provably small
    if (!(v > 0.0)) return 0;
    const double x = v * (double)(2 * kLadderPerUnit);
    if (x >= (double)kLadder2Levels) return kLadder2Levels;
    const int j = (int)x;
    return ((double)j < x) ? j + 1 : j;
  };
  for (int c = lane; c <= t; c += 64) {
    if (c == c0) continue;
    const int J = blocked_below(d[c]);
    if (J == 0) continue;
    if (c < c0) atomicMax(&left[J], c);
    else atomicMin(&right[J], c);
  }
  __syncthreads();
  if (lane == 0) {
    int l = -1, r = t + 1;
    for (int k = kLadder2Levels; k >= 0; k--) {
      l = left[k] > l ? left[k] : l;
      r = right[k] < r ? right[k] : r;
      left[k] = l;
      right[k] = r;
    }
  }
  __syncthreads();
  const int Jbest = blocked_below(d[c0]);
  for (int j = lane; j < kLadder2Levels; j += 64) {
    u32 e = 1u;   // lo = 1, hi = 0: empty
    if (Jbest <= j) e = ((u32)(right[j + 1] - 1) << 16) | (u32)(left[j + 1] + 1);
    ladder[(size_t)j * TD + t] = e;
  }
  if (lane == 0) {
    ladder[(size_t)kLadder2Levels * TD + t] = 0xffff0000u;
    ladder[(size_t)(kLadder2Levels + 1) * TD + t] = 1u;
  }
}

hipError_t launch_build_ladder2(const double* dmax, int TD, uint32_t* ladder, hipStream_t stream) {
  hipLaunchKernelGGL(k_build_ladder2, dim3((unsigned)TD), dim3(64), 0, stream, dmax, TD, ladder);
  return hipGetLastError();
}

}  // namespace gcre

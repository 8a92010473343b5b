// gcre_inspect.hip -- the inspectors of the inclusion-exclusion form for gfx950: per joined path the carrier counts, the
// observed score, the kept row, the check of the reduced operand and the delta / overlap list that the null kernels of
// gcre_ie.hip, gcre_ie2.hip and gcre_ieq.hip stream; and the range-union check of a hinted join (k_range_union).
#include "gcre_ie_common.h"

namespace gcre {

// ------------------------------------------------------------------------------------------------
// inspector of the IE form, one pass: real-label statistics and observed score of every joined path (what k_stats
// does, methods.h:73-93), the kept row, the check of the reduced operand, the choice delta / overlap list and the
// list itself.  One wave per joined path.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 ie_score_key(double s) {
  // order-preserving image of a double; 0 = "not a candidate" (score not > -inf, or NaN: methods.h:91)
  if (!(s > -__builtin_inf())) return 0;
  const u64 b = (u64)__double_as_longlong(s);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// inclusive prefix sum inside every row of 16 lanes (DPP row_shr: no LDS); lane 15 of a row ends up with its total
__device__ __forceinline__ u32 row_scan_add(u32 v) {
  u32 s = v;
  s += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
  s += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
  s += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x113, 0xf, 0xf, true);   // row_shr:3
  s += (u32)__builtin_amdgcn_update_dpp(0, (int)s, 0x114, 0xf, 0xe, true);   // row_shr:4, banks 1-3
  s += (u32)__builtin_amdgcn_update_dpp(0, (int)s, 0x118, 0xf, 0xc, true);   // row_shr:8, banks 2-3
  return s;
}
// value of lane 15 of the caller's row, in every lane of the row
__device__ __forceinline__ u32 row_last(u32 v, int lane) {
  return (u32)__builtin_amdgcn_ds_bpermute(((lane | 15) << 2), (int)v);
}
__device__ __forceinline__ u32 row_total(u32 v, int lane) { return row_last(row_scan_add(v), lane); }

// Long lists keep their tail (entries 8 ..) in the overflow area.  Every wave carves it out of a private chunk of
// kOverChunk entries and only goes to the shared counter a.ov_count for a new chunk (one same-address atomic with return
// per list costs microseconds).
struct OverChunk {
  u32 at = 0u, left = 0u;
  // one list per group of 16 lanes, `need` entries past its slot each: where the group's list continues
  __device__ __forceinline__ u32 take(u32 need, int group, int lane, u32* ov_count) {
    const u32 n0 = rdlane(need, 0), n1 = rdlane(need, 16), n2 = rdlane(need, 32), n3 = rdlane(need, 48);
    const u32 nsum = n0 + n1 + n2 + n3;
    u32 ovb = 0u;
    if (nsum != 0u) {
      if (left < nsum) {
        const u32 grab = nsum > kOverChunk ? nsum : kOverChunk;
        u32 wbase = 0u;
        if (lane == 0) wbase = atomicAdd(ov_count, grab);
        at = (u32)__builtin_amdgcn_readfirstlane((int)wbase);
        left = grab;
      }
      ovb = at + (group > 0 ? n0 : 0u) + (group > 1 ? n1 : 0u) + (group > 2 ? n2 : 0u);
      at += nsum;
      left -= nsum;
    }
    return ovb;
  }
};

// the wave's share of the flag block (FlagWord): largest carrier total, broken hint, overlap-mode lists, longest list
__device__ __forceinline__ void publish_flags(const StatsArgs& a, u32 max_tot, bool bad, u32 modes, u32 max_len) {
  if (max_tot) atomicMax(a.max_tot, max_tot);
  if (bad) *a.bad = 1u;
  if (modes) atomicAdd(a.bad + (kFlagOverlapLists - kFlagHintBroken), modes);   // statistics: overlap-mode lists
  if (max_len > 8u) atomicMax(a.max_tot + kFlagMaxLen, max_len);   // longest list (padded): the quad kernel sums up to 56 entries
}

// Sixteen lanes per joined path, four paths per wave: a path row is Wp <= 1024 words, a rare-variant cohort has ~80,
// and everything per path (counts, decisions, list positions) stays in vector registers, uniform inside a row.  Any
// width: the row's words are read again for the lists (launch_stats_ie runs it for rows wider than the block-staged
// kernels take).
template <int M>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_stats_ie(const StatsArgs a) {
  const int lane = threadIdx.x & 63;
  const int sl = lane & 15;
  const i64 wave = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
  const i64 nwaves = (i64)gridDim.x * 4;
  const int Wp = a.Wp;
  u32 my_max_tot = 0, my_modes = 0, my_max_len = 0;
  bool my_bad = false;
  OverChunk chunk;
  // the row numbers of the next group of four paths (two dependent loads) are fetched while this one is worked on
  // (rng: the uid's row of the excess table, or kNoRange when an earlier path of this launch shares the uid -- the
  // check "excess inside paths0[idx]" is per uid, one path of it is enough)
  constexpr u32 kNoRange = 0xffffffffu;
  auto fetch = [&](i64 base, u32& r0, u32& r1raw, u32& zraw, u32& rng) {
    const i64 i = (base + (lane >> 4) < a.count) ? base + (lane >> 4) : a.count - 1;
    r0 = a.row0[i];
    r1raw = a.row1[i];
    zraw = a.zindex ? (u32)a.zindex[r1raw & 0x7fffffffu] : (r1raw & 0x7fffffffu);
    rng = kNoRange;
    if (a.excess && (i == 0 || a.row0[i - 1] != r0)) rng = (u32)a.range_of[r0];
  };
  u32 n_r0 = 0, n_r1raw = 0, n_zraw = 0, n_rng = 0;
  if (wave * 4 < a.count) fetch(wave * 4, n_r0, n_r1raw, n_zraw, n_rng);
  for (i64 base = wave * 4; base < a.count; base += nwaves * 4) {
    const bool active = base + (lane >> 4) < a.count;
    const i64 i = active ? base + (lane >> 4) : a.count - 1;   // idle rows shadow the last path and write nothing
    const u32 r0 = n_r0, r1raw = n_r1raw, zraw = n_zraw, rng = n_rng;
    if (base + nwaves * 4 < a.count) fetch(base + nwaves * 4, n_r0, n_r1raw, n_zraw, n_rng);
    const u32 rz = zraw & 0x7fffffffu;
    const u32 zflip = (r1raw ^ (a.zindex ? zraw : 0u)) & 0x80000000u;
    const u64* x = a.p0 + (size_t)r0 * a.S;
    const u64* z = a.pz + (size_t)rz * a.S;
    // The joined row is paths0[idx] | paths1[loc] (methods.h:77-78 / :164-165).  paths1[loc] is never read here:
    // without a hint z IS paths1[loc]; with one, paths1[loc] = z | excess (k_range_union checked z inside it) and
    // the union U of the excess over every row this uid joins must lie inside paths0[idx] -- checked below -- so
    // paths0[idx] | paths1[loc] == paths0[idx] | z for every path of the uid.
    const u64* uu = (rng != kNoRange) ? a.excess + (size_t)rng * a.S : nullptr;
    u64* out = (a.res && active) ? a.res + (size_t)(a.first + i) * a.S : nullptr;
    const bool swap = (M == 2) && (r1raw >> 31) != 0;
    const u64* uh[2] = {(uu && swap) ? uu + Wp : uu, (uu && !swap) ? uu + Wp : uu};
    const u64* zh[2] = {zflip ? z + Wp : z, zflip ? z : z + Wp};

    // ---- pass 1: counts, 16 bits each, two to a register (64 * Wp < 65535) ----
    u32 cc[M], dv[M];          // carriers among cases | among controls << 16, delta | overlap << 16
#pragma unroll
    for (int h = 0; h < M; h++) cc[h] = dv[h] = 0u;
    u64 stray = 0;   // excess bits outside paths0[idx]: the hint does not describe this uid
    auto tally = [&](int h, int k, u64 xk, u64 zk, u64 uk, u64 cm) {
      const u64 j = xk | zk;
      if (out) out[h * Wp + k] = j;
      stray |= uk & ~xk;
      cc[h] += (u32)__popcll(j & cm) | ((u32)__popcll(j) << 16);          // among the cases | all (controls by difference)
      dv[h] += (u32)__popcll(zk & ~xk) | ((u32)__popcll(zk) << 16);       // new | all of z (overlap by difference)
    };
    for (int k = sl; k < Wp; k += 16) {
      const u64 cm = a.case_mask[k];
#pragma unroll
      for (int h = 0; h < M; h++) tally(h, k, x[h * Wp + k], zh[h][k], uu ? uh[h][k] : 0, cm);
    }
    if (stray) my_bad = true;
    u32 tot[M], mode[M], len[M], inc[M], inm[M];
#pragma unroll
    for (int h = 0; h < M; h++) {
      const u32 c = row_total(cc[h], lane), d = row_total(dv[h], lane);
      inc[h] = c & 0xffffu;      // carriers among the cases
      tot[h] = c >> 16;
      inm[h] = tot[h] - inc[h];  // carriers among the controls
      const u32 dl = d & 0xffffu, ov = (d >> 16) - dl;
      mode[h] = a.ie_rule ? ((ov <= 8u || ov < dl) ? 1u : 0u) : ((a.ie_bias >= 0 && ov + (u32)a.ie_bias < dl) ? 1u : 0u);
      len[h] = mode[h] ? ov : dl;
      if (active && sl == 0) {
        my_modes += mode[h];
        my_max_tot = max(my_max_tot, tot[h]);
      }
    }
    double score = 0.0;   // looked up here, stored after the lists are out: the wave does not sit on the (cold) table load
    if (active && sl == 0) {
      if constexpr (M == 1) {
        score = a.dvt[(size_t)sp_diag_offset(tot[0]) + inc[0]];   // vt[cases][ctrls], methods.h:90
        a.tot[i] = tot[0];
        a.cases[i] = inc[0];
        a.ctrls[i] = inm[0];
      } else {
        // (+) half: case_pos = inc[0], ctrl_neg = inm[0]; (-) half: ctrl_pos = inc[1], case_neg = inm[1] (methods.h:182-185)
        const u32 case_pos = inc[0], ctrl_neg = inm[0], ctrl_pos = inc[M - 1], case_neg = inm[M - 1];
        score = a.dvt[(size_t)sp_diag_offset(tot[0]) + case_pos] + a.dvt[(size_t)sp_diag_offset(tot[M - 1]) + case_neg];
        a.tot[2 * i] = tot[0];
        a.tot[2 * i + 1] = tot[M - 1];
        a.cases[i] = case_pos + case_neg;        // methods.h:256-257
        a.ctrls[i] = ctrl_pos + ctrl_neg;
      }
      a.rowz[i] = rz | zflip;
    }

    // ---- pass 2: the lists.  Entry = patient << 8 (byte offset of the patient's row in a mask tile) ----
#pragma unroll
    for (int h = 0; h < M; h++) {
      const u64 d = (u64)i * M + h;
      const u32 len8 = max(8u, (len[h] + 7u) & ~7u);
      // long lists keep their tail in the overflow area (OverChunk)
      const u32 need = (active && len8 > 8u) ? len8 - 8u : 0u;
      const u32 ovb = chunk.take(need, lane >> 4, lane, a.ov_count);
      const bool ov_ok = active && len8 > 8u && (u64)ovb + (len8 - 8u) <= (u64)a.over_cap;
      u32* slot = a.slot + d * 8;
      u32* over = a.over + ovb;
      // positions: lane-major inside the row (any order of a list is as good as any other): one row scan of the
      // lanes' entry counts, then every lane writes its own entries back to back
      auto word = [&](int it) -> u64 {
        const int k = it * 16 + sl;
        if (k >= Wp) return 0;
        const u64 xk = x[h * Wp + k], zk = zh[h][k];
        return mode[h] ? (zk & xk) : (zk & ~xk);
      };
      const int nit = (Wp + 15) / 16;
      u32 mine = 0u;
      for (int it = 0; it < nit; it++) mine += (u32)__popcll(word(it));
      u32 pos = row_scan_add(mine) - mine;
      auto emit = [&](int it) {
        u64 w = word(it);
        const u32 k = (u32)(it * 16 + sl);
        while (w) {
          const u32 b = (u32)__builtin_ctzll(w);
          w &= w - 1;
          const u32 e = (k * 64u + b) << 8;
          if (pos < 8u) { if (active) slot[pos] = e; }
          else if (ov_ok) over[pos - 8u] = e;
          pos++;
        }
      };
      for (int it = 0; it < nit; it++) emit(it);
      for (u32 p = len[h] + (u32)sl; p < len8; p += 16) {   // padding: the all-zero mask row
        if (p < 8u) { if (active) slot[p] = a.zoff; }
        else if (ov_ok) over[p - 8u] = a.zoff;
      }
      if (active && sl == 0) {
        a.linfo[d] = linfo_make(len8, mode[h], len[h]);
        a.lover[d] = ovb;
        my_max_len = max(my_max_len, len8);
      }
    }
    if (active && sl == 0) a.key[i] = ie_score_key(score);
  }
  publish_flags(a, my_max_tot, my_bad, my_modes, my_max_len);
}

// Excess of paths1 over the reduced operand, per distinct (location, count) range of the join index:
//   U[r] = OR over loc in the range of  paths1[loc] & ~z'(loc),   z'(loc) = reduced[index[loc]] in paths1's orientation
// and the check that z'(loc) lies inside paths1[loc].  A range is a block of consecutive paths1 rows (RangePiece; the host
// cuts a range of more than kRangePieceRows rows into pieces of that many).  A wave owns one (piece, 32-word column): each of
// its four 16-lane groups reads every fourth row of the piece, 16 bytes per lane and all its rows in flight at once, the
// groups' excess words meet by two shuffles, and the column of U[range] is written once, zero words included -- a plain
// store, U need not be zero on entry.  Only the pieces of a cut range meet in one row of U: they OR their non-zero words
// into it with atomics, and k_range_zero clears those rows first.
constexpr int kRangeGroupRows = kRangePieceRows / 4;
constexpr int kRangeUnionMaxBlocks = 1024;   // x 4 waves x 64 lanes x kRangeGroupRows x 32 B in flight: 33 MB

__global__ __launch_bounds__(256) void k_range_union(const u64* p1, const u64* pz, const int32_t* zindex, const RangePiece* pieces,
                                                     i64 npieces, int S, int Wp, int M, u64* excess, u32* bad) {
  const int sl = threadIdx.x & 15, grp = (threadIdx.x >> 4) & 3;
  const int ncol = (S + 31) >> 5;                     // 32-word columns of a row
  const i64 items = npieces * ncol;
  const i64 nwaves = (i64)gridDim.x * 4;
  bool my_bad = false;
  for (i64 it = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += nwaves) {   // (wave-uniform)
    const i64 pc = it / ncol;
    const int w = ((int)(it - pc * ncol) << 5) + 2 * sl;   // this lane's two words (S and Wp are multiples of 4: never split)
    const bool active = w < S;                             // (the same in the four lanes that meet below)
    const RangePiece piece = pieces[pc];
    const int n = piece.rows & 0x7fffffff;
    const int h = active ? w / Wp : 0, k = active ? w - h * Wp : 0;
    u32 zraw[kRangeGroupRows];
    ulonglong2 y[kRangeGroupRows], z[kRangeGroupRows];
#pragma unroll
    for (int j = 0; j < kRangeGroupRows; j++) {
      const bool v = active && grp + 4 * j < n;
      zraw[j] = v ? (u32)zindex[piece.first + grp + 4 * j] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kRangeGroupRows; j++) {
      const bool v = active && grp + 4 * j < n;
      const int hz = (M == 2 && (zraw[j] >> 31)) ? 1 - h : h;
      y[j] = z[j] = make_ulonglong2(0ull, 0ull);
      if (v) {
        y[j] = *reinterpret_cast<const ulonglong2*>(p1 + (size_t)(piece.first + grp + 4 * j) * S + w);
        z[j] = *reinterpret_cast<const ulonglong2*>(pz + (size_t)(zraw[j] & 0x7fffffffu) * S + (size_t)hz * Wp + k);
      }
    }
    ulonglong2 acc = make_ulonglong2(0ull, 0ull);
#pragma unroll
    for (int j = 0; j < kRangeGroupRows; j++) {
      if ((z[j].x & ~y[j].x) | (z[j].y & ~y[j].y)) my_bad = true;
      acc.x |= y[j].x & ~z[j].x;
      acc.y |= y[j].y & ~z[j].y;
    }
#pragma unroll
    for (int d = 16; d <= 32; d <<= 1) {
      acc.x |= __shfl_xor(acc.x, d);
      acc.y |= __shfl_xor(acc.y, d);
    }
    if (active && grp == 0) {
      u64* u = excess + (size_t)piece.range * S + w;
      if (piece.rows < 0) {   // a piece of a cut range
        if (acc.x) atomicOr((unsigned long long*)u, acc.x);
        if (acc.y) atomicOr((unsigned long long*)(u + 1), acc.y);
      } else {
        *reinterpret_cast<ulonglong2*>(u) = acc;
      }
    }
  }
  if (my_bad) *bad = 1u;
}

// the rows of U that the pieces of cut ranges OR into
__global__ __launch_bounds__(256) void k_range_zero(const int32_t* cut, i64 ncut, int S, u64* excess) {
  const i64 total = ncut * (S >> 1);
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < total; i += (i64)gridDim.x * 256) {
    const i64 c = i / (S >> 1);
    const int w = (int)(i - c * (S >> 1)) * 2;
    *reinterpret_cast<ulonglong2*>(excess + (size_t)cut[c] * S + w) = make_ulonglong2(0ull, 0ull);
  }
}

hipError_t launch_range_union(const uint64_t* p1, const uint64_t* pz, const int32_t* zindex, const RangePiece* pieces,
                              int64_t npieces, const int32_t* cut, int64_t ncut, int S, int Wp, int method, uint64_t* excess,
                              uint32_t* bad, hipStream_t stream) {
  if (npieces == 0) return hipSuccess;
  if (ncut) {
    const i64 zb = (ncut * (S >> 1) + 255) / 256;
    hipLaunchKernelGGL(k_range_zero, dim3((unsigned)(zb < 4096 ? zb : 4096)), dim3(256), 0, stream, cut, ncut, S, excess);
  }
  const i64 blocks = (npieces * ((S + 31) >> 5) + 3) / 4;
  const i64 grid = blocks < kRangeUnionMaxBlocks ? blocks : kRangeUnionMaxBlocks;
  trace_launch("k_range_union", blocks, grid);
  hipLaunchKernelGGL(k_range_union, dim3((unsigned)grid), dim3(256), 0, stream, p1, pz, zindex, pieces, npieces, S, Wp, method,
                     excess, bad);
  return hipGetLastError();
}

// Row totals of a path set for the inspector's counts (k_stats_ie2<NL, true>): counts[r] = carriers | carriers among the
// cases << 16 of row r.  A 16-lane group per row and round, 16 bytes per lane, up to five loads of a row in flight (rows
// of at most 160 words: what the block-staged inspectors take); no LDS, so it runs beside a resident pruned kernel.
constexpr int kRowCountsMaxBlocks = 1024;
__global__ __launch_bounds__(256) void k_row_counts(const u64* rows, i64 nrows, int Wp, const u64* case_mask, u32* counts) {
  typedef u64 __attribute__((ext_vector_type(2))) u64x2;
  const int lane = threadIdx.x & 63, sl = lane & 15;
  const i64 ngroups = (i64)gridDim.x * 16;
  for (i64 r0 = (i64)blockIdx.x * 16 + (threadIdx.x >> 6) * 4; r0 < nrows; r0 += ngroups) {   // (wave-uniform)
    const i64 r = r0 + (lane >> 4);
    const bool valid = r < nrows;
    u64x2 v[5];
#pragma unroll
    for (int it = 0; it < 5; it++) {
      const int k = it * 32 + 2 * sl;
      v[it] = u64x2{0ull, 0ull};
      if (valid && k < Wp) v[it] = *(const u64x2*)(rows + (size_t)r * Wp + k);   // Wp is a multiple of 4: k + 1 is inside
    }
    u32 c = 0u;
#pragma unroll
    for (int it = 0; it < 5; it++) {
      const int k = it * 32 + 2 * sl;
      if (k < Wp) {
        const u64x2 cm = *(const u64x2*)(case_mask + k);
        c += (u32)__popcll(v[it].x) + (u32)__popcll(v[it].y) +
             (((u32)__popcll(v[it].x & cm.x) + (u32)__popcll(v[it].y & cm.y)) << 16);
      }
    }
    c = row_total(c, lane);
    if (valid && sl == 0) counts[r] = c;
  }
}

hipError_t launch_row_counts(const uint64_t* rows, int64_t nrows, int Wp, const uint64_t* case_mask, uint32_t* counts,
                             hipStream_t stream) {
  if (nrows == 0) return hipSuccess;
  if (Wp > 160 || (Wp & 3)) return hipErrorInvalidValue;
  const i64 blocks = (nrows + 15) / 16;
  const i64 grid = blocks < kRowCountsMaxBlocks ? blocks : kRowCountsMaxBlocks;
  trace_launch("k_row_counts", blocks, grid);
  hipLaunchKernelGGL(k_row_counts, dim3((unsigned)grid), dim3(256), 0, stream, rows, nrows, Wp, case_mask, counts);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The method-1 inspector, block-staged form.  Same outputs as k_stats_ie<1>, bit for bit, but organised around what
// bounded that kernel: not its ~110 VALU instructions per path but its ~7.5 vector-memory instructions per path (the CU's
// vector-memory pipe takes ~15 clocks per wave-level load or store whatever its width, tools/row_gather_rate.hip) -- seven
// 4-byte stores per path by one lane in sixteen, one store per list entry, 8-byte row loads.  Here a wave owns 64
// CONSECUTIVE joined paths: their row numbers are read with one coalesced load per array, their seven result words and
// their 8-entry list slots are collected in LDS and written with one coalesced store per array per 64 paths, and the
// rows are read 16 bytes per lane.  Sixteen lanes per path, four paths at a time, as before.
// NL = 16-byte loads per row and lane = ceil(Wp / 32) (Wp <= 32 * NL).
// ------------------------------------------------------------------------------------------------
// 122 VGPRs with one set of row registers (below): four waves per SIMD without a spill; 6.0 against 6.7 ms per pass at
// three.  Five (96 VGPRs, 27 spilled, the pair buffer flushed in chunks to fit the LDS): 8.1 ms
constexpr int kStatsWaves = 4;
// CNT: the counts of the joined row from row totals instead of from its words (a.z_counts is set).  A join adds one short
// row z to a row x whose counts are known, with ov = popc(x & z):
//   carriers   popc(x | z)        = tot(x) + tot(z) - ov
//   cases      popc((x | z) & cm) = cases(x) + cases(z) - popc(x & z & cm)
//   delta      popc(z & ~x)       = tot(z) - ov
// tot(z) | cases(z) << 16 is read per reduced row (k_row_counts wrote it once per path set), tot(x) | cases(x) << 16 is
// counted when a group moves on to another paths0 row, and the words of x & z that are not zero -- a handful -- are what the
// list pass collects anyway: each lane counts one collected word.  Four 64-bit popcounts per word and lane less; integers,
// so the outputs are the same bit for bit.
template <int NL, bool CNT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NL <= 3 ? kStatsWaves : 2))) void k_stats_ie2(const StatsArgs a) {
  typedef u64 __attribute__((ext_vector_type(2))) u64x2;
  constexpr u32 kNoRange = 0xffffffffu;
  __shared__ u32 slot_lds[4][64 * 8];   // the 64 paths' list slots
  __shared__ u32 out_lds[4][8][64];     // their result words: tot, cases, ctrls, rowz, key lo, key hi, linfo, lover
  __shared__ u32 pair_lds[4][4][3][32 * NL];   // per group: the non-zero words of the current path's list (low, high, word index)
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sl = lane & 15, grp = lane >> 4;
  const u32 gsh = (u32)grp * 16u, ltm = (1u << sl) - 1u;
  u32 (*pairs)[32 * NL] = pair_lds[wv][grp];
  __shared__ u32 meta_lds[4][3][64];    // the 64 paths' paths0 row, reduced row, range
  u32 (*meta)[64] = meta_lds[wv];
  const i64 wave = (i64)blockIdx.x * 4 + wv;
  const i64 nwaves = (i64)gridDim.x * 4;
  const int Wp = a.Wp;
  u32* slots = slot_lds[wv];
  u32 (*outs)[64] = out_lds[wv];
  u32 my_max_tot = 0, my_modes = 0, my_max_len = 0;
  bool my_bad = false;
  OverChunk chunk;
  // this lane's words of a row: 2 sl, 2 sl + 1 of every 32-word block
  // the case mask sits in LDS (words beyond Wp zero), read where it is used: twelve registers less per lane
  __shared__ u64 cm_lds[32 * NL];
  for (int k = (int)threadIdx.x; k < 32 * NL; k += 256) cm_lds[k] = k < Wp ? a.case_mask[k] : 0;
  __syncthreads();
  const i64 nblocks = (a.count + 63) / 64;
  for (i64 blk = wave; blk < nblocks; blk += nwaves) {
    const i64 base = blk * 64;
    const i64 iq = base + lane < a.count ? base + lane : a.count - 1;
    // ---- the 64 paths' row numbers, one coalesced load per array (lane t <-> path base + t) ----
    const u32 r0v = a.row0[iq];
    const u32 r1v = a.row1[iq];
    const u32 zv = a.zindex ? (u32)a.zindex[r1v & 0x7fffffffu] : (r1v & 0x7fffffffu);
    u32 rngv = kNoRange;   // the uid's row of the excess table, for the first path of a uid in this launch only
    if (a.excess && (iq == 0 || a.row0[iq - 1] != r0v)) rngv = (u32)a.range_of[r0v];
    // (lane t <-> path t: parked in LDS, read back per group -- three registers less than keeping them for ds_bpermute)
    meta[0][lane] = r0v;
    meta[1][lane] = zv & 0x7fffffffu;
    meta[2][lane] = rngv;
    __builtin_amdgcn_wave_barrier();
    // slots start as padding
    {
      const u32x4 pad = {a.zoff, a.zoff, a.zoff, a.zoff};
      ((u32x4*)slots)[lane * 2] = pad;
      ((u32x4*)slots)[lane * 2 + 1] = pad;
    }
    // the observed score is a gather from a 100-MB table (a miss all the way to HBM): its key is written one path late,
    // so that the wave never sits on that load
    double score_prev = 0.0;
    int pl_prev = -1;
    // The rows of the next four paths are requested as soon as these four have given up their list words (behind the
    // collection pass below), straight into the registers the current rows occupied: one set of row registers instead of
    // two is what lets a fourth wave onto the SIMD, and the other waves cover what the shorter distance no longer does.
    // (consecutive joined paths mostly share their paths0 row -- one uid joins ~11 rows at level 4: a group that stays
    // on the same row keeps its words, and when no group moves on the load is not issued at all)
    u64 xw[NL][2], zw[NL][2];
#pragma unroll
    for (int it = 0; it < NL; it++) xw[it][0] = xw[it][1] = zw[it][0] = zw[it][1] = 0ull;
    u32 n_rz = 0u, n_rng = kNoRange, n_r0 = 0xffffffffu;
    // CNT: the reduced row's totals, asked for a round ahead like its words; whether the round starts on another paths0 row;
    // that row's totals, kept while the group stays on it
    u32 n_zc = 0u, x_cnt = 0u;
    bool n_newx = false;
    auto fetch_rows = [&](int it4n) {
      const int pln = it4n * 4 + grp;
      const u32 r0n = meta[0][pln];
      n_rz = meta[1][pln];
      n_rng = meta[2][pln];
      const bool new_x = r0n != n_r0;
      n_r0 = r0n;
      if constexpr (CNT) {
        n_newx = new_x;
        n_zc = a.z_counts[n_rz];
      }
      const u64* xn = a.p0 + (size_t)r0n * a.S;
      const u64* zn = a.pz + (size_t)n_rz * a.S;
#pragma unroll
      for (int it = 0; it < NL; it++) {
        const int k = it * 32 + 2 * sl;
        if (k < Wp) {            // Wp is a multiple of 4: words k and k + 1 are both inside
          if (new_x) {
            const u64x2 v = *(const u64x2*)(xn + k);
            xw[it][0] = v.x; xw[it][1] = v.y;
          }
          const u64x2 v = *(const u64x2*)(zn + k);
          zw[it][0] = v.x; zw[it][1] = v.y;
        }
      }
    };
    fetch_rows(0);
    for (int it4 = 0; it4 < 16; it4++) {
      const int pl = it4 * 4 + grp;                 // the group's path inside the block
      const bool active = base + pl < a.count;
      if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
      const u32 rz = n_rz, rng = n_rng;
      const u64* uu = (rng != kNoRange) ? a.excess + (size_t)rng * a.S : nullptr;
      u64* out = (a.res && active) ? a.res + (size_t)(a.first + base + pl) * a.S : nullptr;
      u32 inc, tot, inm, mode, len, npair = 0u;
      if constexpr (CNT) {
        // ---- the hint check, in the rounds where some group starts a uid; the kept row ----
        if (__builtin_amdgcn_ballot_w64(rng != kNoRange) != 0ull) {
          u64 stray = 0;
#pragma unroll
          for (int it = 0; it < NL; it++) {
            const int k = it * 32 + 2 * sl;
            u64x2 uv = {0, 0};
            if (k < Wp && uu) uv = *(const u64x2*)(uu + k);
            stray |= (uv.x & ~xw[it][0]) | (uv.y & ~xw[it][1]);
          }
          if (stray) my_bad = true;
        }
        if (out) {
#pragma unroll
          for (int it = 0; it < NL; it++) {
            const int k = it * 32 + 2 * sl;
            if (k < Wp) *(u64x2*)(out + k) = u64x2{xw[it][0] | zw[it][0], xw[it][1] | zw[it][1]};
          }
        }
        // ---- the paths0 row's totals, when the group has moved on to another row ----
        if (n_newx) {
          u32 xc = 0u;
#pragma unroll
          for (int it = 0; it < NL; it++) {
            const u64x2 cmv = *(const u64x2*)(cm_lds + it * 32 + 2 * sl);
            xc += (u32)__popcll(xw[it][0]) + (u32)__popcll(xw[it][1]) +
                  (((u32)__popcll(xw[it][0] & cmv.x) + (u32)__popcll(xw[it][1] & cmv.y)) << 16);
          }
          x_cnt = row_total(xc, lane);
        }
        const u32 zc = n_zc;
        // ---- the words of x & z that are not zero, collected per group as the list pass wants them (below) ----
#pragma unroll
        for (int it = 0; it < NL; it++) {
#pragma unroll
          for (int e = 0; e < 2; e++) {
            const u64 w = zw[it][e] & xw[it][e];
            const bool nz = active && w != 0;
            const u64 bal = __builtin_amdgcn_ballot_w64(nz);
            if (bal == 0ull) continue;
            const u32 m = (u32)(bal >> gsh) & 0xffffu;
            const u32 at = npair + (u32)__builtin_popcount(m & ltm);
            if (nz) {
              pairs[0][at] = (u32)w;
              pairs[1][at] = (u32)(w >> 32);
              pairs[2][at] = (u32)(it * 32 + 2 * sl + e);
            }
            npair += (u32)__builtin_popcount(m);
          }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- overlap | overlap among the cases << 16: every lane counts one collected word ----
        u32 ovc = 0u;
        {
          const u32 npmax = max(max(rdlane(npair, 0), rdlane(npair, 16)), max(rdlane(npair, 32), rdlane(npair, 48)));
          for (u32 p0 = 0u; p0 < npmax; p0 += 16u) {
            const u32 pi = p0 + (u32)sl;
            const bool has = pi < npair;
            const u64 w = has ? ((u64)pairs[1][pi] << 32) | (u64)pairs[0][pi] : 0ull;
            const u32 k = has ? pairs[2][pi] : 0u;
            ovc += (u32)__popcll(w) | ((u32)__popcll(w & cm_lds[k]) << 16);
          }
          if (npmax != 0u) ovc = row_total(ovc, lane);
        }
        const u32 c = x_cnt + zc - ovc;                     // (no borrow: each half of ovc is at most that half of zc)
        tot = c & 0xffffu, inc = c >> 16, inm = tot - inc;
        const u32 ov = ovc & 0xffffu, dl = (zc & 0xffffu) - ov;
        mode = a.ie_rule ? ((ov <= 8u || ov < dl) ? 1u : 0u) : ((a.ie_bias >= 0 && ov + (u32)a.ie_bias < dl) ? 1u : 0u);
        len = mode ? ov : dl;
        // ---- a delta list (rare: an overlap above 8 and not below the delta): the group collects z & ~x instead ----
        const bool delta = active && mode == 0u;
        if (__builtin_amdgcn_ballot_w64(delta) != 0ull) {
          if (delta) npair = 0u;
#pragma unroll
          for (int it = 0; it < NL; it++) {
#pragma unroll
            for (int e = 0; e < 2; e++) {
              const u64 w = zw[it][e] & ~xw[it][e];
              const bool nz = delta && w != 0;
              const u64 bal = __builtin_amdgcn_ballot_w64(nz);
              if (bal == 0ull) continue;
              const u32 m = (u32)(bal >> gsh) & 0xffffu;
              const u32 at = npair + (u32)__builtin_popcount(m & ltm);
              if (nz) {
                pairs[0][at] = (u32)w;
                pairs[1][at] = (u32)(w >> 32);
                pairs[2][at] = (u32)(it * 32 + 2 * sl + e);
              }
              npair += (u32)__builtin_popcount(m);
            }
          }
        }
      } else {
        u32 cc = 0u, dv = 0u;
        u64 stray = 0;
#pragma unroll
        for (int it = 0; it < NL; it++) {
          const int k = it * 32 + 2 * sl;
          u64x2 uv = {0, 0};
          if (k < Wp && uu) uv = *(const u64x2*)(uu + k);
          const u64x2 cmv = *(const u64x2*)(cm_lds + k);
          const u64 cme[2] = {cmv.x, cmv.y};
#pragma unroll
          for (int e = 0; e < 2; e++) {
            const u64 xk = xw[it][e], zk = zw[it][e], uk = e ? uv.y : uv.x;
            stray |= uk & ~xk;
            const u64 j = xk | zk;
            cc += (u32)__popcll(j & cme[e]) | ((u32)__popcll(j) << 16);
            dv += (u32)__popcll(zk & ~xk) | ((u32)__popcll(zk) << 16);
          }
          if (out && k < Wp) *(u64x2*)(out + k) = u64x2{xw[it][0] | zw[it][0], xw[it][1] | zw[it][1]};
        }
        if (stray) my_bad = true;
        const u32 c = row_total(cc, lane), d = row_total(dv, lane);
        inc = c & 0xffffu, tot = c >> 16, inm = tot - inc;
        const u32 dl = d & 0xffffu, ov = (d >> 16) - dl;
        mode = a.ie_rule ? ((ov <= 8u || ov < dl) ? 1u : 0u) : ((a.ie_bias >= 0 && ov + (u32)a.ie_bias < dl) ? 1u : 0u);
        len = mode ? ov : dl;
        // The list's bits are few and scattered -- three overlapping patients among a path's 96 lane-words -- so a loop per
        // word runs its body for one lane at a time.  Instead the non-zero words are first collected per group (word, its
        // index; positions from a ballot), then every lane takes one collected word and all of them give up a bit per round:
        // two rounds instead of eight bodies.  Entries come out in collection order, not ascending (the list is a set).
#pragma unroll
        for (int it = 0; it < NL; it++) {
#pragma unroll
          for (int e = 0; e < 2; e++) {
            const u64 w = mode ? (zw[it][e] & xw[it][e]) : (zw[it][e] & ~xw[it][e]);
            const bool nz = active && w != 0;
            const u64 bal = __builtin_amdgcn_ballot_w64(nz);
            if (bal == 0ull) continue;
            const u32 m = (u32)(bal >> gsh) & 0xffffu;
            const u32 at = npair + (u32)__builtin_popcount(m & ltm);
            if (nz) {
              pairs[0][at] = (u32)w;
              pairs[1][at] = (u32)(w >> 32);
              pairs[2][at] = (u32)(it * 32 + 2 * sl + e);
            }
            npair += (u32)__builtin_popcount(m);
          }
        }
      }
      const u32 len8 = max(8u, (len + 7u) & ~7u);
      fetch_rows(it4 < 15 ? it4 + 1 : 15);   // (changes rz / rng of the NEXT iteration only: this one read them above)
      double score = 0.0;
      if (active && sl == 0) {
        my_modes += mode;
        my_max_tot = max(my_max_tot, tot);
        my_max_len = max(my_max_len, len8);
        score = a.dvt[(size_t)sp_diag_offset(tot) + inc];   // vt[cases][ctrls], methods.h:90
      }
      // ---- the list: first 8 entries into the LDS slot, the rest into the overflow area (chunk reserved per wave) ----
      const u32 need = (active && len8 > 8u) ? len8 - 8u : 0u;
      const u32 ovb = chunk.take(need, grp, lane, a.ov_count);
      const bool ov_ok = active && len8 > 8u && (u64)ovb + (len8 - 8u) <= (u64)a.over_cap;
      u32* over = a.over + ovb;
      __builtin_amdgcn_wave_barrier();
      {
        const u32 npmax = max(max(rdlane(npair, 0), rdlane(npair, 16)), max(rdlane(npair, 32), rdlane(npair, 48)));
        u32 cnt = 0u;
        for (u32 p0 = 0u; p0 < npmax; p0 += 16u) {
          const u32 pi = p0 + (u32)sl;
          const bool has = pi < npair;
          u64 w = has ? ((u64)pairs[1][pi] << 32) | (u64)pairs[0][pi] : 0ull;
          const u32 k = has ? pairs[2][pi] : 0u;
          while (__builtin_amdgcn_ballot_w64(w != 0ull) != 0ull) {
            const bool nzb = w != 0ull;
            const u32 m = (u32)(__builtin_amdgcn_ballot_w64(nzb) >> gsh) & 0xffffu;
            const u32 pos = cnt + (u32)__builtin_popcount(m & ltm);
            const u32 b = nzb ? (u32)__builtin_ctzll(w) : 0u;
            w &= w - 1ull;
            const u32 en = (k * 64u + b) << 8;
            if (nzb) {
              if (pos < 8u) slots[pl * 8 + (int)pos] = en;
              else if (ov_ok) over[pos - 8u] = en;
            }
            cnt += (u32)__builtin_popcount(m);
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      for (u32 p = max(len, 8u) + (u32)sl; p < len8; p += 16)   // padding of the overflow part
        if (ov_ok) over[p - 8u] = a.zoff;
      // ---- the path's result words into LDS, lane pl of every array ----
      if (pl_prev >= 0) {
        const u64 key = ie_score_key(score_prev);
        outs[4][pl_prev] = (u32)key;
        outs[5][pl_prev] = (u32)(key >> 32);
      }
      pl_prev = -1;
      if (active && sl == 0) {
        outs[0][pl] = tot;
        outs[1][pl] = inc;
        outs[2][pl] = inm;
        outs[3][pl] = rz;
        outs[6][pl] = linfo_make(len8, mode, len);
        outs[7][pl] = ovb;
        score_prev = score;
        pl_prev = pl;
      }
    }
    if (pl_prev >= 0) {
      const u64 key = ie_score_key(score_prev);
      outs[4][pl_prev] = (u32)key;
      outs[5][pl_prev] = (u32)(key >> 32);
    }
    // ---- 64 paths' results and slots, one coalesced store per array ----
    if (base + lane < a.count) {
      const i64 i = base + lane;
      a.tot[i] = outs[0][lane];
      a.cases[i] = outs[1][lane];
      a.ctrls[i] = outs[2][lane];
      a.rowz[i] = outs[3][lane];
      a.key[i] = ((u64)outs[5][lane] << 32) | outs[4][lane];
      a.linfo[i] = outs[6][lane];
      a.lover[i] = outs[7][lane];
      u32x4* dst = (u32x4*)(a.slot + (u64)i * 8u);
      dst[0] = ((const u32x4*)slots)[lane * 2];
      dst[1] = ((const u32x4*)slots)[lane * 2 + 1];
    }
  }
  publish_flags(a, my_max_tot, my_bad, my_modes, my_max_len);
}

// ------------------------------------------------------------------------------------------------
// The signed method's inspector, block-staged like k_stats_ie2 (round 4).  A joined path is two half-rows; every 16-lane
// group works on ONE (path, half) -- a "virtual row" -- so a wave owns 32 consecutive joined paths = 64 virtual rows, the
// group's half is fixed (group & 1: a group that stays on the same paths0 row keeps that half's words), and the per-half
// outputs (carriers, carriers among the cases, list info, list slot) are staged in LDS exactly as the unsigned kernel
// stages its per-path ones.  What needs both halves -- the observed score vt[case_pos][ctrl_neg] + vt[case_neg][ctrl_pos]
// (methods.h:255), the reported counts (:256-257) -- is put together per path when the block is written out.
// Same outputs as k_stats_ie<2>, bit for bit.
// ------------------------------------------------------------------------------------------------
template <int NL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NL <= 3 ? kStatsWaves : 2))) void k_stats_ie2s(const StatsArgs a) {
  typedef u64 __attribute__((ext_vector_type(2))) u64x2;
  constexpr u32 kNoRange = 0xffffffffu;
  __shared__ u32 slot_lds[4][64 * 8];   // the 64 virtual rows' list slots
  __shared__ u32 out_lds[4][4][64];     // per virtual row: carriers, carriers among the cases, linfo, lover
  __shared__ u32 pair_lds[4][4][3][32 * NL];
  __shared__ u32 meta_lds[4][4][32];    // per path: paths0 row, reduced row | flip, range, swap of paths1
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sl = lane & 15, grp = lane >> 4;
  const int h = grp & 1;                // the half this group works on, in the joined path's orientation
  const u32 gsh = (u32)grp * 16u, ltm = (1u << sl) - 1u;
  u32 (*pairs)[32 * NL] = pair_lds[wv][grp];
  u32 (*meta)[32] = meta_lds[wv];
  const i64 wave = (i64)blockIdx.x * 4 + wv;
  const i64 nwaves = (i64)gridDim.x * 4;
  const int Wp = a.Wp;
  u32* slots = slot_lds[wv];
  u32 (*outs)[64] = out_lds[wv];
  u32 my_max_tot = 0, my_modes = 0, my_max_len = 0;
  bool my_bad = false;
  OverChunk chunk;
  __shared__ u64 cm_lds[32 * NL];
  for (int k = (int)threadIdx.x; k < 32 * NL; k += 256) cm_lds[k] = k < Wp ? a.case_mask[k] : 0;
  __syncthreads();
  const i64 nblocks = (a.count + 31) / 32;
  for (i64 blk = wave; blk < nblocks; blk += nwaves) {
    const i64 base = blk * 32;
    {
      // ---- the 32 paths' row numbers (lanes t and t + 32 both read path base + t) ----
      const i64 iq = base + (lane & 31) < a.count ? base + (lane & 31) : a.count - 1;
      const u32 r0v = a.row0[iq];
      const u32 r1v = a.row1[iq];
      const u32 zraw = a.zindex ? (u32)a.zindex[r1v & 0x7fffffffu] : (r1v & 0x7fffffffu);
      const u32 zflip = (r1v ^ (a.zindex ? zraw : 0u)) & 0x80000000u;
      u32 rngv = kNoRange;   // the uid's row of the excess table, for the first path of a uid in this launch only
      if (a.excess && (iq == 0 || a.row0[iq - 1] != r0v)) rngv = (u32)a.range_of[r0v];
      if (lane < 32) {
        meta[0][lane] = r0v;
        meta[1][lane] = (zraw & 0x7fffffffu) | zflip;
        meta[2][lane] = rngv;
        meta[3][lane] = r1v >> 31;
      }
    }
    __builtin_amdgcn_wave_barrier();
    {
      const u32x4 pad = {a.zoff, a.zoff, a.zoff, a.zoff};
      ((u32x4*)slots)[lane * 2] = pad;
      ((u32x4*)slots)[lane * 2 + 1] = pad;
    }
    u64 xw[NL][2], zw[NL][2];
#pragma unroll
    for (int it = 0; it < NL; it++) xw[it][0] = xw[it][1] = zw[it][0] = zw[it][1] = 0ull;
    u32 n_rzf = 0u, n_rng = kNoRange, n_r0 = 0xffffffffu, n_swap = 0u;
    auto fetch_rows = [&](int itn) {
      const int pln = (itn * 4 + grp) >> 1;
      const u32 r0n = meta[0][pln];
      n_rzf = meta[1][pln];
      n_rng = meta[2][pln];
      n_swap = meta[3][pln];
      const bool new_x = r0n != n_r0;
      n_r0 = r0n;
      const int hz = (n_rzf >> 31) ? 1 - h : h;   // the reduced row's half that lands in half h
      const u64* xn = a.p0 + (size_t)r0n * a.S + (size_t)h * Wp;
      const u64* zn = a.pz + (size_t)(n_rzf & 0x7fffffffu) * a.S + (size_t)hz * Wp;
#pragma unroll
      for (int it = 0; it < NL; it++) {
        const int k = it * 32 + 2 * sl;
        if (k < Wp) {
          if (new_x) {
            const u64x2 v = *(const u64x2*)(xn + k);
            xw[it][0] = v.x; xw[it][1] = v.y;
          }
          const u64x2 v = *(const u64x2*)(zn + k);
          zw[it][0] = v.x; zw[it][1] = v.y;
        }
      }
    };
    fetch_rows(0);
    for (int it8 = 0; it8 < 16; it8++) {
      const int vl = it8 * 4 + grp;                 // the group's virtual row inside the block
      const int pl = vl >> 1;                       // ... and its path
      const bool active = base + pl < a.count;
      if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
      const u32 rng = n_rng, swap = n_swap;
      // the excess row is in paths1's orientation: its half (swap ? 1 - h : h) lands in half h
      const u64* uu = (rng != kNoRange) ? a.excess + (size_t)rng * a.S + (size_t)(swap ? 1 - h : h) * Wp : nullptr;
      u64* out = (a.res && active) ? a.res + (size_t)(a.first + base + pl) * a.S + (size_t)h * Wp : nullptr;
      u32 cc = 0u, dv = 0u;
      u64 stray = 0;
#pragma unroll
      for (int it = 0; it < NL; it++) {
        const int k = it * 32 + 2 * sl;
        u64x2 uv = {0, 0};
        if (k < Wp && uu) uv = *(const u64x2*)(uu + k);
        const u64x2 cmv = *(const u64x2*)(cm_lds + k);
        const u64 cme[2] = {cmv.x, cmv.y};
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const u64 xk = xw[it][e], zk = zw[it][e], uk = e ? uv.y : uv.x;
          stray |= uk & ~xk;
          const u64 j = xk | zk;
          cc += (u32)__popcll(j & cme[e]) | ((u32)__popcll(j) << 16);
          dv += (u32)__popcll(zk & ~xk) | ((u32)__popcll(zk) << 16);
        }
        if (out && k < Wp) *(u64x2*)(out + k) = u64x2{xw[it][0] | zw[it][0], xw[it][1] | zw[it][1]};
      }
      if (stray) my_bad = true;
      const u32 c = row_total(cc, lane), d = row_total(dv, lane);
      const u32 inc = c & 0xffffu, tot = c >> 16;
      const u32 dl = d & 0xffffu, ov = (d >> 16) - dl;
      const u32 mode = a.ie_rule ? ((ov <= 8u || ov < dl) ? 1u : 0u) : ((a.ie_bias >= 0 && ov + (u32)a.ie_bias < dl) ? 1u : 0u);
      const u32 len = mode ? ov : dl;
      const u32 len8 = max(8u, (len + 7u) & ~7u);
      u32 npair = 0u;
#pragma unroll
      for (int it = 0; it < NL; it++) {
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const u64 w = mode ? (zw[it][e] & xw[it][e]) : (zw[it][e] & ~xw[it][e]);
          const bool nz = active && w != 0;
          const u64 bal = __builtin_amdgcn_ballot_w64(nz);
          if (bal == 0ull) continue;
          const u32 m = (u32)(bal >> gsh) & 0xffffu;
          const u32 at = npair + (u32)__builtin_popcount(m & ltm);
          if (nz) {
            pairs[0][at] = (u32)w;
            pairs[1][at] = (u32)(w >> 32);
            pairs[2][at] = (u32)(it * 32 + 2 * sl + e);
          }
          npair += (u32)__builtin_popcount(m);
        }
      }
      fetch_rows(it8 < 15 ? it8 + 1 : 15);   // (changes the NEXT iteration's words and row numbers only)
      if (active && sl == 0) {
        my_modes += mode;
        my_max_tot = max(my_max_tot, tot);
        my_max_len = max(my_max_len, len8);
      }
      const u32 need = (active && len8 > 8u) ? len8 - 8u : 0u;
      const u32 ovb = chunk.take(need, grp, lane, a.ov_count);
      const bool ov_ok = active && len8 > 8u && (u64)ovb + (len8 - 8u) <= (u64)a.over_cap;
      u32* over = a.over + ovb;
      __builtin_amdgcn_wave_barrier();
      {
        const u32 npmax = max(max(rdlane(npair, 0), rdlane(npair, 16)), max(rdlane(npair, 32), rdlane(npair, 48)));
        u32 cnt = 0u;
        for (u32 q0 = 0u; q0 < npmax; q0 += 16u) {
          const u32 pi = q0 + (u32)sl;
          const bool has = pi < npair;
          u64 w = has ? ((u64)pairs[1][pi] << 32) | (u64)pairs[0][pi] : 0ull;
          const u32 k = has ? pairs[2][pi] : 0u;
          while (__builtin_amdgcn_ballot_w64(w != 0ull) != 0ull) {
            const bool nzb = w != 0ull;
            const u32 m = (u32)(__builtin_amdgcn_ballot_w64(nzb) >> gsh) & 0xffffu;
            const u32 pos = cnt + (u32)__builtin_popcount(m & ltm);
            const u32 b = nzb ? (u32)__builtin_ctzll(w) : 0u;
            w &= w - 1ull;
            const u32 en = (k * 64u + b) << 8;
            if (nzb) {
              if (pos < 8u) slots[vl * 8 + (int)pos] = en;
              else if (ov_ok) over[pos - 8u] = en;
            }
            cnt += (u32)__builtin_popcount(m);
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      for (u32 p = max(len, 8u) + (u32)sl; p < len8; p += 16)   // padding of the overflow part
        if (ov_ok) over[p - 8u] = a.zoff;
      if (active && sl == 0) {
        outs[0][vl] = tot;
        outs[1][vl] = inc;
        outs[2][vl] = linfo_make(len8, mode, len);
        outs[3][vl] = ovb;
      }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- per path: both halves together -> observed score, reported counts (lanes 0..31) ----
    if (lane < 32 && base + lane < a.count) {
      const i64 i = base + lane;
      const u32 tot0 = outs[0][2 * lane], tot1 = outs[0][2 * lane + 1];
      // (+) half: case_pos = inc0, ctrl_neg = tot0 - inc0; (-) half: ctrl_pos = inc1, case_neg = tot1 - inc1 (methods.h:182-185)
      const u32 case_pos = outs[1][2 * lane], ctrl_neg = tot0 - case_pos;
      const u32 ctrl_pos = outs[1][2 * lane + 1], case_neg = tot1 - ctrl_pos;
      const double score = a.dvt[(size_t)sp_diag_offset(tot0) + case_pos] + a.dvt[(size_t)sp_diag_offset(tot1) + case_neg];
      a.tot[2 * i] = tot0;
      a.tot[2 * i + 1] = tot1;
      a.cases[i] = case_pos + case_neg;        // methods.h:256-257
      a.ctrls[i] = ctrl_pos + ctrl_neg;
      a.rowz[i] = meta[1][lane];
      a.key[i] = ie_score_key(score);
    }
    // ---- per virtual row: list info and slot, one coalesced store per array ----
    if (base * 2 + lane < a.count * 2) {
      const i64 dd = base * 2 + lane;
      a.linfo[dd] = outs[2][lane];
      a.lover[dd] = outs[3][lane];
      u32x4* dst = (u32x4*)(a.slot + (u64)dd * 8u);
      dst[0] = ((const u32x4*)slots)[lane * 2];
      dst[1] = ((const u32x4*)slots)[lane * 2 + 1];
    }
    __builtin_amdgcn_wave_barrier();
  }
  publish_flags(a, my_max_tot, my_bad, my_modes, my_max_len);
}

// ------------------------------------------------------------------------------------------------
// The signed method's inspector when every reduced row has an EMPTY half (genes: a gene's carriers sit in one half, the
// other half of its row is zero -- every join below level 5).  Then only one half of a joined path differs from its paths0
// row: k_stats_ie2s spends a round of sixteen lanes on each half of every path, this kernel one round per PATH --
// the half that changes (side of the reduced row, flipped when the relation's sign says so) -- and takes the other half's
// carriers from the paths0 row, counted once per uid when a group of lanes moves on to it (both halves of that row stay in
// registers: consecutive paths of a uid change either half).  A wave owns 64 consecutive paths.  Same outputs as
// k_stats_ie2s except the (unused) overflow offset of an empty list.  a.lz_off: the CSR offsets of the reduced rows' bit
// lists (two lists per row): list 2 r + 1 empty <=> the (-) half of row r is.
// ------------------------------------------------------------------------------------------------
constexpr int kStats2hWaves = 4;   // 128 VGPRs, 5 spilled: 7.0 ms per pass on configs[2] geometry against 7.7 at three waves (134, none)
template <int NL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NL <= 3 ? kStats2hWaves : 2))) void k_stats_ie2h(const StatsArgs a) {
  typedef u64 __attribute__((ext_vector_type(2))) u64x2;
  constexpr u32 kNoRange = 0xffffffffu;
  __shared__ u32 slot_lds[4][64 * 8];   // the 64 paths' list slots (of the half that changes)
  __shared__ u32 out_lds[4][7][64];     // per path: carriers (+), (-), among the cases (+), (-), linfo, lover, the half that changes
  __shared__ u32 pair_lds[4][4][3][32 * NL];
  __shared__ u32 meta_lds[4][5][64];    // per path: paths0 row, reduced row | flip, range, swap of paths1, side of the reduced row
  __shared__ u64 cm_lds[32 * NL];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sl = lane & 15, grp = lane >> 4;
  const u32 gsh = (u32)grp * 16u, ltm = (1u << sl) - 1u;
  u32 (*pairs)[32 * NL] = pair_lds[wv][grp];
  u32 (*meta)[64] = meta_lds[wv];
  const i64 wave = (i64)blockIdx.x * 4 + wv;
  const i64 nwaves = (i64)gridDim.x * 4;
  const int Wp = a.Wp;
  u32* slots = slot_lds[wv];
  u32 (*outs)[64] = out_lds[wv];
  u32 my_max_tot = 0, my_modes = 0, my_max_len = 0;
  bool my_bad = false;
  OverChunk chunk;
  for (int k = (int)threadIdx.x; k < 32 * NL; k += 256) cm_lds[k] = k < Wp ? a.case_mask[k] : 0;
  __syncthreads();
  // an empty list as the inspector writes it: no entries, eight of padding (the bias rule of the signed method: delta list)
  const u32 empty_mode = a.ie_rule ? 1u : 0u;   // (overlap 0, delta 0: the slot rule says overlap list, the bias rule delta list)
  const u32 empty_linfo = linfo_make(8u, empty_mode, 0u);
  const i64 nblocks = (a.count + 63) / 64;
  for (i64 blk = wave; blk < nblocks; blk += nwaves) {
    const i64 base = blk * 64;
    {
      // ---- the 64 paths' row numbers, one coalesced load per array (lane t <-> path base + t) ----
      const i64 iq = base + lane < a.count ? base + lane : a.count - 1;
      const u32 r0v = a.row0[iq];
      const u32 r1v = a.row1[iq];
      const u32 zraw = a.zindex ? (u32)a.zindex[r1v & 0x7fffffffu] : (r1v & 0x7fffffffu);
      const u32 zflip = (r1v ^ (a.zindex ? zraw : 0u)) & 0x80000000u;
      const u32 zrow = zraw & 0x7fffffffu;
      u32 rngv = kNoRange;   // the uid's row of the excess table, for the first path of a uid in this launch only
      if (a.excess && (iq == 0 || a.row0[iq - 1] != r0v)) rngv = (u32)a.range_of[r0v];
      const u32 side = a.lz_off[2 * (size_t)zrow + 2] > a.lz_off[2 * (size_t)zrow + 1] ? 1u : 0u;   // the row's (-) half has carriers
      meta[0][lane] = r0v;
      meta[1][lane] = zrow | zflip;
      meta[2][lane] = rngv;
      meta[3][lane] = r1v >> 31;
      meta[4][lane] = side;
    }
    __builtin_amdgcn_wave_barrier();
    {
      const u32x4 pad = {a.zoff, a.zoff, a.zoff, a.zoff};
      ((u32x4*)slots)[lane * 2] = pad;
      ((u32x4*)slots)[lane * 2 + 1] = pad;
    }
    u64 xw[2][NL][2], zw[NL][2];
#pragma unroll
    for (int it = 0; it < NL; it++) xw[0][it][0] = xw[0][it][1] = xw[1][it][0] = xw[1][it][1] = zw[it][0] = zw[it][1] = 0ull;
    u32 n_rzf = 0u, n_rng = kNoRange, n_r0 = 0xffffffffu, n_swap = 0u, n_hc = 0u;
    bool n_newx = false;
    auto fetch_rows = [&](int itn) {
      const int pln = itn * 4 + grp;
      const u32 r0n = meta[0][pln];
      n_rzf = meta[1][pln];
      n_rng = meta[2][pln];
      n_swap = meta[3][pln];
      const u32 side = meta[4][pln];
      n_hc = (n_rzf >> 31) ? 1u - side : side;   // the half of the joined path the reduced row's carriers land in
      n_newx = r0n != n_r0;
      n_r0 = r0n;
      const u64* xn = a.p0 + (size_t)r0n * a.S;
      const u64* zn = a.pz + (size_t)(n_rzf & 0x7fffffffu) * a.S + (size_t)side * Wp;
#pragma unroll
      for (int it = 0; it < NL; it++) {
        const int k = it * 32 + 2 * sl;
        if (k < Wp) {
          if (n_newx) {
            const u64x2 v0 = *(const u64x2*)(xn + k);
            const u64x2 v1 = *(const u64x2*)(xn + Wp + k);
            xw[0][it][0] = v0.x; xw[0][it][1] = v0.y;
            xw[1][it][0] = v1.x; xw[1][it][1] = v1.y;
          }
          const u64x2 v = *(const u64x2*)(zn + k);
          zw[it][0] = v.x; zw[it][1] = v.y;
        }
      }
    };
    fetch_rows(0);
    u32 tx0 = 0u, tx1 = 0u;   // carriers | carriers among the cases << 16 of the paths0 row's halves
    for (int it4 = 0; it4 < 16; it4++) {
      const int pl = it4 * 4 + grp;                 // the group's path inside the block
      const bool active = base + pl < a.count;
      if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
      const u32 rng = n_rng, swap = n_swap, hc = n_hc;
      const bool newx = n_newx;
      // ---- a new paths0 row: the carriers of both its halves; (first path of a uid) the check of the hint, both halves ----
      if (__builtin_amdgcn_ballot_w64(newx) != 0ull) {
        u32 c0 = 0u, c1 = 0u;
        u64 stray = 0;
        // the excess row is in paths1's orientation: its half (swap ? 1 - h : h) lands in half h
        const u64* uu = (newx && rng != kNoRange) ? a.excess + (size_t)rng * a.S : nullptr;
#pragma unroll
        for (int it = 0; it < NL; it++) {
          const int k = it * 32 + 2 * sl;
          const u64x2 cmv = *(const u64x2*)(cm_lds + k);
          c0 += ((u32)__popcll(xw[0][it][0]) + (u32)__popcll(xw[0][it][1])) |
                (((u32)__popcll(xw[0][it][0] & cmv.x) + (u32)__popcll(xw[0][it][1] & cmv.y)) << 16);
          c1 += ((u32)__popcll(xw[1][it][0]) + (u32)__popcll(xw[1][it][1])) |
                (((u32)__popcll(xw[1][it][0] & cmv.x) + (u32)__popcll(xw[1][it][1] & cmv.y)) << 16);
          if (uu && k < Wp) {
            const u64x2 u0 = *(const u64x2*)(uu + (size_t)(swap ? 1 : 0) * Wp + k);   // lands in half 0
            const u64x2 u1 = *(const u64x2*)(uu + (size_t)(swap ? 0 : 1) * Wp + k);   // lands in half 1
            stray |= (u0.x & ~xw[0][it][0]) | (u0.y & ~xw[0][it][1]) | (u1.x & ~xw[1][it][0]) | (u1.y & ~xw[1][it][1]);
          }
        }
        if (stray) my_bad = true;
        const u32 t0 = row_total(c0, lane), t1 = row_total(c1, lane);
        if (newx) { tx0 = t0; tx1 = t1; }
      }
      u64* out = (a.res && active) ? a.res + (size_t)(a.first + base + pl) * a.S : nullptr;
      // ---- the half that changes ----
      u32 cc = 0u, dv = 0u;
      u64 xk_[NL][2];
#pragma unroll
      for (int it = 0; it < NL; it++) {
        const int k = it * 32 + 2 * sl;
        const u64x2 cmv = *(const u64x2*)(cm_lds + k);
        const u64 cme[2] = {cmv.x, cmv.y};
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const u64 xk = hc ? xw[1][it][e] : xw[0][it][e], zk = zw[it][e];
          xk_[it][e] = xk;
          const u64 j = xk | zk;
          cc += (u32)__popcll(j & cme[e]) | ((u32)__popcll(j) << 16);
          dv += (u32)__popcll(zk & ~xk) | ((u32)__popcll(zk) << 16);
        }
        if (out && k < Wp) {   // the kept row: the changed half joined, the other as it was
          const u64x2 jc = u64x2{xk_[it][0] | zw[it][0], xk_[it][1] | zw[it][1]};
          const u64x2 ju = hc ? u64x2{xw[0][it][0], xw[0][it][1]} : u64x2{xw[1][it][0], xw[1][it][1]};
          *(u64x2*)(out + (size_t)hc * Wp + k) = jc;
          *(u64x2*)(out + (size_t)(1u - hc) * Wp + k) = ju;
        }
      }
      const u32 c = row_total(cc, lane), d = row_total(dv, lane);
      const u32 inc = c & 0xffffu, tot = c >> 16;
      const u32 dl = d & 0xffffu, ov = (d >> 16) - dl;
      const u32 mode = a.ie_rule ? ((ov <= 8u || ov < dl) ? 1u : 0u) : ((a.ie_bias >= 0 && ov + (u32)a.ie_bias < dl) ? 1u : 0u);
      const u32 len = mode ? ov : dl;
      const u32 len8 = max(8u, (len + 7u) & ~7u);
      u32 npair = 0u;
#pragma unroll
      for (int it = 0; it < NL; it++) {
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const u64 w = mode ? (zw[it][e] & xk_[it][e]) : (zw[it][e] & ~xk_[it][e]);
          const bool nz = active && w != 0;
          const u64 bal = __builtin_amdgcn_ballot_w64(nz);
          if (bal == 0ull) continue;
          const u32 m = (u32)(bal >> gsh) & 0xffffu;
          const u32 at = npair + (u32)__builtin_popcount(m & ltm);
          if (nz) {
            pairs[0][at] = (u32)w;
            pairs[1][at] = (u32)(w >> 32);
            pairs[2][at] = (u32)(it * 32 + 2 * sl + e);
          }
          npair += (u32)__builtin_popcount(m);
        }
      }
      // the other half's carriers: the paths0 row's
      const u32 tu = hc ? tx0 : tx1;
      const u32 tot_u = tu & 0xffffu, inc_u = tu >> 16;
      fetch_rows(it4 < 15 ? it4 + 1 : 15);   // (changes the NEXT iteration's words and row numbers only)
      if (active && sl == 0) {
        my_modes += mode + empty_mode;
        my_max_tot = max(my_max_tot, max(tot, tot_u));
        my_max_len = max(my_max_len, len8);
      }
      const u32 need = (active && len8 > 8u) ? len8 - 8u : 0u;
      const u32 ovb = chunk.take(need, grp, lane, a.ov_count);
      const bool ov_ok = active && len8 > 8u && (u64)ovb + (len8 - 8u) <= (u64)a.over_cap;
      u32* over = a.over + ovb;
      __builtin_amdgcn_wave_barrier();
      {
        const u32 npmax = max(max(rdlane(npair, 0), rdlane(npair, 16)), max(rdlane(npair, 32), rdlane(npair, 48)));
        u32 cnt = 0u;
        for (u32 q0 = 0u; q0 < npmax; q0 += 16u) {
          const u32 pi = q0 + (u32)sl;
          const bool has = pi < npair;
          u64 w = has ? ((u64)pairs[1][pi] << 32) | (u64)pairs[0][pi] : 0ull;
          const u32 k = has ? pairs[2][pi] : 0u;
          while (__builtin_amdgcn_ballot_w64(w != 0ull) != 0ull) {
            const bool nzb = w != 0ull;
            const u32 m = (u32)(__builtin_amdgcn_ballot_w64(nzb) >> gsh) & 0xffffu;
            const u32 pos = cnt + (u32)__builtin_popcount(m & ltm);
            const u32 b = nzb ? (u32)__builtin_ctzll(w) : 0u;
            w &= w - 1ull;
            const u32 en = (k * 64u + b) << 8;
            if (nzb) {
              if (pos < 8u) slots[pl * 8 + (int)pos] = en;
              else if (ov_ok) over[pos - 8u] = en;
            }
            cnt += (u32)__builtin_popcount(m);
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      for (u32 p = max(len, 8u) + (u32)sl; p < len8; p += 16)   // padding of the overflow part
        if (ov_ok) over[p - 8u] = a.zoff;
      if (active && sl == 0) {
        outs[0][pl] = hc ? tot_u : tot;
        outs[1][pl] = hc ? tot : tot_u;
        outs[2][pl] = hc ? inc_u : inc;
        outs[3][pl] = hc ? inc : inc_u;
        outs[4][pl] = linfo_make(len8, mode, len);
        outs[5][pl] = ovb;
        outs[6][pl] = hc;
      }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- per path: both halves together -> observed score, reported counts ----
    if (base + lane < a.count) {
      const i64 i = base + lane;
      const u32 tot0 = outs[0][lane], tot1 = outs[1][lane];
      // (+) half: case_pos = inc0, ctrl_neg = tot0 - inc0; (-) half: ctrl_pos = inc1, case_neg = tot1 - inc1 (methods.h:182-185)
      const u32 case_pos = outs[2][lane], ctrl_neg = tot0 - case_pos;
      const u32 ctrl_pos = outs[3][lane], case_neg = tot1 - ctrl_pos;
      const double score = a.dvt[(size_t)sp_diag_offset(tot0) + case_pos] + a.dvt[(size_t)sp_diag_offset(tot1) + case_neg];
      a.tot[2 * i] = tot0;
      a.tot[2 * i + 1] = tot1;
      a.cases[i] = case_pos + case_neg;        // methods.h:256-257
      a.ctrls[i] = ctrl_pos + ctrl_neg;
      a.rowz[i] = meta[1][lane];
      a.key[i] = ie_score_key(score);
    }
    // ---- per virtual row (two per path): list info and slot, coalesced; the half that did not change has the empty list ----
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int v = j * 64 + lane, pv = v >> 1;
      if (base + pv < a.count) {
        const i64 dd = base * 2 + v;
        const bool ch = outs[6][pv] == (u32)(v & 1);
        a.linfo[dd] = ch ? outs[4][pv] : empty_linfo;
        a.lover[dd] = ch ? outs[5][pv] : 0u;
        const u32x4 pad = {a.zoff, a.zoff, a.zoff, a.zoff};
        u32x4* dst = (u32x4*)(a.slot + (u64)dd * 8u);
        dst[0] = ch ? ((const u32x4*)slots)[pv * 2] : pad;
        dst[1] = ch ? ((const u32x4*)slots)[pv * 2 + 1] : pad;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  publish_flags(a, my_max_tot, my_bad, my_modes, my_max_len);
}

// a block-staged inspector: kernel[NL - 1], NL = ceil(Wp / 32) <= 5, a wave per `per_wave` consecutive paths
using StatsKernel = void (*)(StatsArgs);
static hipError_t launch_staged(const StatsKernel (&kernel)[5], const char* name, i64 per_wave, const StatsArgs& a,
                                hipStream_t stream) {
  const i64 nb = (a.count + per_wave - 1) / per_wave;
  const i64 blocks = (nb + kInspectBlockWaves - 1) / kInspectBlockWaves;
  const dim3 grid((unsigned)(blocks < kInspectMaxBlocks ? blocks : kInspectMaxBlocks)), block(64 * kInspectBlockWaves);
  const int nl = (a.Wp + 31) / 32;
  trace_launch(name, blocks, grid.x);
  hipLaunchKernelGGL(kernel[nl <= 1 ? 0 : nl - 1], grid, block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_stats_ie(const StatsArgs& a, int method, hipStream_t stream) {
  if (a.count == 0) return hipSuccess;
  static const StatsKernel ie2[5] = {k_stats_ie2<1, false>, k_stats_ie2<2, false>, k_stats_ie2<3, false>, k_stats_ie2<4, false>,
                                     k_stats_ie2<5, false>};
  static const StatsKernel ie2c[5] = {k_stats_ie2<1, true>, k_stats_ie2<2, true>, k_stats_ie2<3, true>, k_stats_ie2<4, true>,
                                      k_stats_ie2<5, true>};
  static const StatsKernel ie2h[5] = {k_stats_ie2h<1>, k_stats_ie2h<2>, k_stats_ie2h<3>, k_stats_ie2h<4>, k_stats_ie2h<5>};
  static const StatsKernel ie2s[5] = {k_stats_ie2s<1>, k_stats_ie2s<2>, k_stats_ie2s<3>, k_stats_ie2s<4>, k_stats_ie2s<5>};
  if (a.Wp <= 160) {
    if (method == 1 && a.z_counts) return launch_staged(ie2c, "k_stats_ie2", 64, a, stream);   // counts from row totals
    if (method == 1) return launch_staged(ie2, "k_stats_ie2", 64, a, stream);
    // the signed method with one-sided reduced rows: one round per path (k_stats_ie2h); otherwise one per half
    if (a.lz_off) return launch_staged(ie2h, "k_stats_ie2h", 64, a, stream);
    return launch_staged(ie2s, "k_stats_ie2s", 32, a, stream);
  }
  const i64 blocks = (a.count + kStatsIeBlockPaths - 1) / kStatsIeBlockPaths;
  const dim3 grid((unsigned)(blocks < kInspectMaxBlocks ? blocks : kInspectMaxBlocks)), block(64 * kInspectBlockWaves);
  trace_launch("k_stats_ie<M>", blocks, grid.x);
  if (method == 1) hipLaunchKernelGGL(k_stats_ie<1>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(k_stats_ie<2>, grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

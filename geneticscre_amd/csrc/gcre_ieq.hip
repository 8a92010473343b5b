// gcre_ieq.hip -- the pruned method-1 null kernel, "quad" form: one wave works on up to kQSegs segments (two; four in round 2) at a time that
// join the same paths1 rows, and fetches the planes of every added row once for all of them.
//
// Same arithmetic and the same lane layout as k_null_ie_m1 (gcre_ie.hip; lane = 32 permutations of a 2048-permutation
// tile): for every joined path
//
//     count = N0[idx] + Nz[z] - popc(p0[idx] & z & mask_r)        (bit-sliced, reference src/methods.h:73-88)
//
// tested against the pruning ladder's interval [lo, hi] of the path's table diagonal; only what falls outside is looked
// up (methods.h:96-103).  With the bound filter (W = N0 + Nz against [lo + ov, hi], see k_null_ie_m1) nine path-tiles in
// ten never read a mask row.  What binds the kernel is instruction issue: neither HBM nor latency -- a
// section's time follows its instruction count, vector, scalar and read-lane alike.  Faster = fewer instructions per
// path-tile: 63 of them are the filter's arithmetic, the rest is control, addressing and scalar-spill traffic, which is
// why the filter pass is one of three loops chosen once per quad and an added row costs one read-lane to address
// (tools/isa_count.py counts a build's instructions per loop).
//
// All uids with the same pivot gene join the same paths1 rows (the join index gives them the same location and count), so
// their segments walk the same sequence of added rows.  The host groups up to kQSegs such segments into a "quad" (the name stayed from the four-segment form)
// (gcre_host.hip ensure_quads).  The wave keeps the base counters of all of them (kQSegs x L registers) and, for every position
// t of the shared sequence, loads Nz[z_t] once and scores path t of each segment against it: the plane loads per
// path-tile drop from 2 to 0.5, the instruction stream per path-tile is unchanged.
#include "gcre_ie_common.h"

#include <type_traits>

namespace gcre {

// Segments per quad and the occupancy the register allocation aims at.  Round 3 (profiles/r03_quad_shapes.txt): two
// segments at four waves per SIMD beat four at three (25.9 vs 27.4 ms of null kernels per pass on configs[2]: the prologue
// and the exact pass wait on memory, a fourth wave covers more of that than sharing a plane load four ways saves);
// four segments at four waves spill (128 VGPRs), three at four do too.
#ifndef GCRE_REFINE_MAX
#define GCRE_REFINE_MAX 2   // flagged permutations per lane up to which a path-tile is queued (or takes the second look); above: exact pass (tuning builds)
#endif
#ifndef GCRE_QSEGS
#define GCRE_QSEGS 2
#endif
#ifndef GCRE_QWAVES
#define GCRE_QWAVES 4
#endif
constexpr int kQSegs = GCRE_QSEGS;

// -DGCRE_IE_TIMING: per-section s_memtime sums (a mark only reads the clock)
#ifdef GCRE_IE_TIMING
#define GCRE_QT(var) const u64 var = __builtin_amdgcn_s_memtime()
#define GCRE_QT_ADD(i, t1, t0) tm[i] += (t1) - (t0)
#else
#define GCRE_QT(var)
#define GCRE_QT_ADD(i, t1, t0)
#endif

// `count` is one of 1..N: calls f with it as a compile-time constant
template <int N, class F>
__device__ __forceinline__ void with_count(u32 count, F&& f) {
  if constexpr (N > 1) {
    if (count != (u32)N) return with_count<N - 1>(count, f);
  }
  f(std::integral_constant<int, N>{});
}

// WIDE: one tile of the added rows' planes does not fit a 32-bit byte offset (IeArgs::z_wide)
template <int L, int GZ, bool REC, bool WIDE>
__global__ __launch_bounds__(64 * kIeWaves) __attribute__((amdgpu_waves_per_eu(GCRE_QWAVES))) void k_null_ie_q(const IeArgs /* read through ie_args() */) {
  constexpr int LP = (L + 3) / 4 * 4;
  constexpr int LZ = 4 * GZ;
  static_assert(L >= 8 && L <= 16 && GZ >= 2 && LZ <= LP, "planes come in groups of 4");
  typedef u32 __attribute__((ext_vector_type(8))) u32x8;
  // every argument is read through ap, where it is used, and never through the by-value copy (gcre_ie_common.h): the
  // lambdas below capture ap by reference and see the pointer as the loops renew it
  const IeArgs GCRE_CONSTANT* ap = ie_args();
  __shared__ u32 nmax_lds[kIeWaves][32 * 64];   // the waves' running maxima [bit][lane]
  __shared__ u32 wq_state[kIeWaves][8];
  // look-ups are queued (cell of the table, slot of the maximum) and made 64 at a time: one memory round trip per 64
  // look-ups instead of one per path (as k_null_ie_m2; a threshold read before a drain is only lower, never wrong)
  constexpr u32 kLqCap = 128u;
  __shared__ u32 lq_lds[kIeWaves][2][kLqCap];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u32 lane4 = (u32)lane * 4u;
  u32* nm = nmax_lds[wave] + lane;
#pragma unroll
  for (int q = 0; q < 32; q++) nm[q * 64] = 0u;
  u32 (*lq)[kLqCap] = lq_lds[wave];
  u32 lq_n = 0u;   // entries waiting (wave-uniform)
  // flagged permutations of the filter pass, queued (joined path; count W | bit << 17 | lane << 22) and scored 64 at a
  // time by fq_drain below: the items address the current tile's masks and maxima
  constexpr u32 kFqCap = 64u;
  __shared__ u32 fq_lds[kIeWaves][2][kFqCap];
  u32 (*fq)[kFqCap] = fq_lds[wave];
  u32 fq_n = 0u;
  auto lq_drain = [&]() {
    for (u32 base = 0u; base < lq_n; base += 64u) {
      const u32 i = base + (u32)lane;
      if (i < lq_n)
        __hip_atomic_fetch_max(nmax_lds[wave] + lq[1][i], ((const u32*)ap->t32)[lq[0][i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);   // ds_max_u32
    }
    lq_n = 0u;
  };
  // No launch constant is pinned to a register (they were, with readfirstlane: read as `a.field` the compiler re-loaded
  // arguments on both sides of the `lane == 0` branch around the ticket atomic and what was derived from such a pair
  // counted as divergent).  A field read through ap is uniform -- the pointer comes out of a scalar asm operand -- and is
  // loaded where it is used; uni() remains for values that come out of vector registers.
  auto uni = [](u32 v) -> u32 { return (u32)__builtin_amdgcn_readfirstlane((int)v); };
  auto uni_ptr = [&](const void* p) -> const char* { return (const char*)(((u64)uni((u32)((u64)p >> 32)) << 32) | (u64)uni((u32)(u64)p)); };
  // what a path-tile with flagged permutations does: 2 queue them (GCRE_IE_FLAGQ=1), 1 the second look of the ladder,
  // 0 the exact pass at once (thresholds that do not come from the maxima)
  auto road = [&]() -> u32 { return (ap->lad_mode == 0) ? (ap->flagq != 0u ? 2u : 1u) : 0u; };

  int cur_kt = -1;
  u32 valid = 0u;
  u32 lad_base = (ap->lad_mode == 0) ? 0u : ((u32)kLadderLevels - 1u + (u32)ap->lad_mode) * (u32)ap->ladder_stride;
  u32 n_slow = 0u;
#ifdef GCRE_IE_TIMING
  // header + loads issued, base counters, filter intervals, filter pass, exact pass, exchange, total, quads; inside the
  // filter pass: second look or queueing, drains; flagged path-tiles; (per lane) flagged permutations
  u64 tm[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  u32 n_flagged = 0u;
  const u64 tm_begin = __builtin_amdgcn_s_memtime();
#endif
  __amdgpu_buffer_rsrc_t mt = __builtin_amdgcn_make_buffer_rsrc((void*)ap->mt, 0, 0x7fffffff, 0x00020000);
  // the planes of the rows the joins add, one descriptor per tile: a row is then a scalar byte offset into it (the
  // scalar offset takes no part in the range check).  WIDE builds a descriptor per row instead.
  __amdgpu_buffer_rsrc_t zt = __builtin_amdgcn_make_buffer_rsrc((void*)ap->planesz, 0, 0x7fffffff, 0x00020000);

  // The queued permutations, one per lane: S = how many of the path's (at most 8) overlap patients are cases in that
  // permutation -- bit `bb` of one dword of each patient's mask row, padding entries point at the all-zero row --
  // count = W - S, one table cell, one maximum.  Three memory round trips per 64 items.
  auto fq_drain = [&]() {
    GCRE_QT(td0);
    if ((u32)lane < fq_n) {
      const u32 q = fq[0][lane], w = fq[1][lane];
      const u32 bb = (w >> 17) & 31u, at = (w >> 22) * 4u;
      const u32x4* e = (const u32x4*)(ap->dlist + (u64)q * 8u);
      const u32x4 e0 = e[0], e1 = e[1];
      const u32 tot = ap->tot[q];
      // (the entry is per lane here, so it goes into the vector offset, which the descriptor's 2-GiB range check sees --
      // the exact pass has it in the unchecked scalar offset.  The host switches the queue off where a tile of masks
      // reaches 2 GiB, gcre_host.hip: 8 million patients)
      u32 y[8];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        y[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, e0[j] + at, 0, 0);
        y[4 + j] = __builtin_amdgcn_raw_buffer_load_b32(mt, e1[j] + at, 0, 0);
      }
      u32 S = 0u;
#pragma unroll
      for (int j = 0; j < 8; j++) S += (y[j] >> bb) & 1u;
      const u32 cell = sp_diag_offset(tot) + (w & 0x1ffffu) - S;
      __hip_atomic_fetch_max(nmax_lds[wave] + bb * 64u + (w >> 22), ((const u32*)ap->t32)[cell], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);   // ds_max_u32
    }
    fq_n = 0u;
    GCRE_QT(td1);
    GCRE_QT_ADD(9, td1, td0);
  };

  // publish the wave's maxima, read everybody's, set the threshold level to the smallest running maximum of the tile's
  // live permutations (a stale read only lowers it: still exact).  The merged values stay in LDS: nm[] is then the best
  // maximum this wave KNOWS of every permutation of the tile (its own finds + the others' as of the last exchange), which
  // is what the queued permutations are folded into (fq_drain) and what the second look of the filter tests against.
  auto merge_global = [&](bool want_theta) {
    u32* out = ap->null_bits + (size_t)cur_kt * 2048 + lane * 32;
    __amdgpu_buffer_rsrc_t nb = __builtin_amdgcn_make_buffer_rsrc((void*)(ap->null_bits + (size_t)cur_kt * 2048), 0, 8192, 0x00020000);
    u32x4 g4[8];
#pragma unroll
    for (int j = 0; j < 8; j++) g4[j] = __builtin_amdgcn_raw_buffer_load_b128(nb, (u32)lane * 128u + (u32)j * 16u, 0, 16 /* sc1 */);
    u32 lo = 0xffffffffu;
    // (the live bits tested HERE: left to itself the compiler turns the 32 tests into 32 lane masks when the tile
    // changes -- 64 scalar registers, spilled once per ticket and reloaded at every exchange)
    u32 live = valid;
    asm volatile("" : "+v"(live));
#pragma unroll
    for (int q = 0; q < 32; q++) {
      const u32 g = g4[q >> 2][q & 3];
      const u32 own = nm[q * 64];
      if (own > g) atomicMax(out + q, own);     // only what this wave raised itself can be above the global value
      const u32 v = own > g ? own : g;
      nm[q * 64] = want_theta ? v : 0u;         // the tile ends: the next tile starts from nothing
      if ((live >> q) & 1u) lo = v < lo ? v : lo;
    }
    return lo;
  };
  auto exchange = [&]() {
    fq_drain();
    lq_drain();
    u32 theta = __builtin_amdgcn_readfirstlane(wave_min_u32(merge_global(true)));
    if (theta == 0xffffffffu) theta = 0u;
    int j = (int)(__uint_as_float(theta) * (float)kLadderPerUnit);
    j = j < 0 ? 0 : (j > kLadderLevels - 1 ? kLadderLevels - 1 : j);
    lad_base = (u32)j * (u32)ap->ladder_stride;
  };
  auto flush_tile = [&]() {   // (before the tile changes: queued items address this tile's masks)
    fq_drain();
    lq_drain();
    if (cur_kt >= 0) (void)merge_global(false);
  };

  WorkQueue wq;
  wq.st = wq_state[wave];
  wq.init(ap->queue, ((u32)ap->quad_end - (u32)ap->quad_begin + (u32)ap->batch - 1u) / (u32)ap->batch, (u32)ap->nkt);
  wq.select(blockIdx.x & 7u);
  u32 ticket = wq.take(lane);
  int since = 0, period = 1;
  for (;;) {
    ie_args_again(ap);
    const u32 work = __builtin_amdgcn_readfirstlane(ticket);
    const u32 q_n = wq.get(2);
    if (work >= q_n) {
      if (!wq.steal(lane)) break;
      ticket = wq.take(lane);
      continue;
    }
    ticket = wq.take(lane);
    const u32 item = wq.get(1) + work, nbt = wq.get(3);
    const int kt = __builtin_amdgcn_readfirstlane((int)(item / nbt));
    const u32 q_lo = uni((u32)ap->quad_begin + (item - (u32)kt * nbt) * (u32)ap->batch);
    const u32 q_hi = uni(q_lo + (u32)ap->batch < (u32)ap->quad_end ? q_lo + (u32)ap->batch : (u32)ap->quad_end);
    if (kt != cur_kt) {
      flush_tile();
      cur_kt = kt;
      mt = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)ap->mt + (size_t)kt * ap->mt_rows * 256u), 0, 0x7fffffff, 0x00020000);
      if constexpr (!WIDE) zt = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)ap->planesz + (u64)kt * (u64)ap->z_tile_units * 1024u), 0, 0x7fffffff, 0x00020000);
      const int live = ap->K - kt * 2048 - lane * 32;
      valid = live >= 32 ? 0xffffffffu : (live <= 0 ? 0u : ((1u << live) - 1u));
      if (ap->lad_mode == 0) lad_base = 0u;
      since = 0;
      period = 1;
    }
    // The table entries of a quad's segments -- (row0, first, n) and, with a recipe, the twelve words k_fill_rec_segs
    // gathered per segment -- are wave-uniform, but a scalar load of them misses all the way to HBM (the tables are tens
    // of MB and every entry is read once): four dependent round trips per quad.  They are fetched one quad ahead into
    // one vector register per segment (lane l = word l) and moved to scalar registers with v_readlane.
    auto load_hdr = [&](u32 qe_, u32 (&h)[kQSegs]) {
      const u32 cnt_ = (qe_ >> 30) + 1u, s0_ = qe_ & 0x3fffffffu;
#pragma unroll
      for (int g = 0; g < kQSegs; g++) {
        h[g] = 0u;
        if ((u32)g < cnt_) {
          const u32* src = (const u32*)ap->segs + (u64)(s0_ + (u32)g) * 3u + (u32)(lane < 3 ? lane : 0);
          if constexpr (REC) {
            if (lane >= 4 && lane < 16) src = ap->rec_segs + (u64)(s0_ + (u32)g) * kRecSegWords + (u32)(lane - 4);
          }
          h[g] = *src;
        }
      }
    };
    u32 hdr_n[kQSegs] = {};
    u32 qe_n = 0u;
    bool have_next = false;
    for (u32 qi = q_lo; qi < q_hi; qi++) {
      // ---- the quad: up to kQSegs consecutive segments of the table, same added rows, same length ----
      ie_args_again(ap);
      GCRE_QT(t0);
      u32 hdr[kQSegs];
      u32 qe;
      if (have_next) {
        qe = qe_n;
#pragma unroll
        for (int g = 0; g < kQSegs; g++) hdr[g] = hdr_n[g];
      } else {
        qe = uni(((const u32 GCRE_CONSTANT*)ap->quads)[qi]);
        load_hdr(qe, hdr);
      }
      have_next = qi + 1u < q_hi;
      if (have_next) qe_n = uni(((const u32 GCRE_CONSTANT*)ap->quads)[qi + 1u]);   // its headers go out below, behind this quad's loads
      const u32 qcnt = (qe >> 30) + 1u;
      const u32 s0 = qe & 0x3fffffffu;
      const u32 npaths = rdlane(hdr[0], 2);
      GCRE_QT(te0);
      if (ap->lad_mode == 0 && ++since >= period) {
        exchange();
        since = 0;
        period = period < kIeRefresh ? period * 2 : kIeRefresh;
      }
      GCRE_QT(te1);
      GCRE_QT_ADD(5, te1, te0);
      const u32 lad_keep = (u32)kLadderLevels * (u32)ap->ladder_stride;
      const u32 lad_row = (s0 < ap->score_segs) ? lad_base : lad_keep;

      // ---- per segment: the metadata of its paths (lane t <-> path first + t) and its base counters ----
      u32 infov[kQSegs], lhv[kQSegs], lfv[kQSegs], firstg[kQSegs];
      u32 B[kQSegs][L];
      u32 zunit = 0u;
      // (P holds L or LP planes: the base counters are loaded in place, what a group has above L is dropped)
      auto load_groups = [&](auto& P, const u32* planes, u64 unit, int groups) {
        constexpr int NP = (int)(sizeof(P) / sizeof(u32));
        __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)(uni_ptr(planes) + unit * 1024u), 0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int j = 0; j < LP / 4; j++) {
          u32x4 v = {0u, 0u, 0u, 0u};
          if (j < groups) v = __builtin_amdgcn_raw_buffer_load_b128(rp, lane4 * 4u + (u32)j * 1024u, 0, 0);
#pragma unroll
          for (int i = 0; i < 4; i++)
            if (4 * j + i < NP) P[4 * j + i] = v[i];
        }
      };
      // (a) everything the quad's segments need from memory goes out together: their paths' metadata, the planes their
      // base counters start from and -- with a recipe -- the mask rows of the producing join's list.  One round trip per
      // quad, not one per segment.
      u32 totv[kQSegs];
      u32 yr[REC ? kQSegs : 1][8];
      u32 rinfo_g[kQSegs] = {}, rlov_g[kQSegs] = {}, rz_g[kQSegs] = {};
      // the paths' metadata first: the ladder gather below needs the carrier totals and must not queue behind the planes
#pragma unroll
      for (int g = 0; g < kQSegs; g++) {
        totv[g] = 0u;
        if ((u32)g < qcnt) {
          const u32 first = rdlane(hdr[g], 1);
          firstg[g] = first;
          const u32 qv = first + (((u32)lane < npaths) ? (u32)lane : 0u);
          infov[g] = ap->linfo[qv];
          totv[g] = ap->tot[qv];
          if (g == 0) {   // the same for every segment of the quad: 1-KB units from planesz, or bytes from the tile's first row
            if constexpr (WIDE) zunit = ((u32)kt * (u32)ap->rowsz + (ap->rowz[qv] & 0x7fffffffu)) * (u32)ap->gz;
            else zunit = ((ap->rowz[qv] & 0x7fffffffu) * (u32)ap->gz) << 10;
          }
        }
      }
#pragma unroll
      for (int g = 0; g < kQSegs; g++) {
        if ((u32)g < qcnt) {
          const u32 row0 = rdlane(hdr[g], 0);
          if constexpr (!REC) {
            load_groups(B[g], ap->planes0, ((u64)kt * (u64)ap->rows0 + (u64)row0) * (u64)ap->g0, ap->g0);
          } else {
            // the segment's recipe words sit next to the segment table (k_fill_rec_segs): paths0 row of the producing
            // join, row it added, list info, where a long list continues, the list's first 8 entries
            const u32 ra = rdlane(hdr[g], 4);
            rz_g[g] = rdlane(hdr[g], 5) & 0x7fffffffu;
            rinfo_g[g] = rdlane(hdr[g], 6);
            rlov_g[g] = rdlane(hdr[g], 7);
            u32 ro[8];
#pragma unroll
            for (int j = 0; j < 8; j++) ro[j] = rdlane(hdr[g], 8 + j);
            const u32 rtrue = linfo_true_len(rinfo_g[g]);   // entries that are not padding
#pragma unroll
            for (int j = 0; j < 8; j++) {
              yr[REC ? g : 0][j] = 0u;
              if ((u32)j < rtrue) yr[REC ? g : 0][j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, ro[j], 0);
            }
            // the row's carrier total bounds the counts of everything it was made from: planes above it are zero and are
            // not read (3 KB -> 2 KB of HBM per segment and tile for most rows: this load is the kernel's HBM traffic)
            const int ga_need = (int)linfo_groups(rinfo_g[g]) + 1;
            load_groups(B[g], ap->rec_planes_a, ((u64)kt * (u64)ap->rec_rows_a + (u64)ra) * (u64)ap->rec_ga, ga_need < ap->rec_ga ? ga_need : ap->rec_ga);
          }
        }
      }
      if (have_next) load_hdr(qe_n, hdr_n);
      GCRE_QT(t1);
      GCRE_QT_ADD(0, t1, t0);
      // (b) with a recipe: row = A + Z -/+ list.  The segments of a quad end in the same pivot gene, so the row the
      // producing join added -- that gene -- is the same for all of them: its planes are loaded once
      if constexpr (REC) {
        u32 ZR[LP];
        load_groups(ZR, ap->rec_planes_z, ((u64)kt * (u64)ap->rec_rows_z + (u64)rz_g[0]) * (u64)ap->rec_gz, ap->rec_gz);
#pragma unroll
        for (int g = 0; g < kQSegs; g++) {
          if ((u32)g < qcnt) {
            if (rz_g[g] != rz_g[0]) load_groups(ZR, ap->rec_planes_z, ((u64)kt * (u64)ap->rec_rows_z + (u64)rz_g[g]) * (u64)ap->rec_gz, ap->rec_gz);
            const u32 rinfo = rinfo_g[g];
            const u32 rlen = linfo_len(rinfo);
            u32 S[L];
            {
              u32 S4[4];
              sum8(yr[REC ? g : 0], S4);
#pragma unroll
              for (int l = 0; l < L; l++) S[l] = (l < 4) ? S4[l < 4 ? l : 0] : 0u;
            }
            if (rlen > 8u) {   // the producing join's list was long: the rest of it, 8 entries at a time
              const u32 GCRE_CONSTANT* more = (const u32 GCRE_CONSTANT*)(ap->rec_over + rlov_g[g]);
              for (u32 p = 0u; p + 8u < rlen; p += 8u) {
                const u32x8 o8 = *(const u32x8 GCRE_CONSTANT*)(more + p);
                u32 yy[8], s4[4];
#pragma unroll
                for (int j = 0; j < 8; j++) yy[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, uni(o8[j]), 0);
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
                const u32 s1_ = xor3(B[g][l], ZR[l], cy);
                cy = majority(B[g][l], ZR[l], cy);
                B[g][l] = xor3(s1_, S[l], bw);
                bw = borrow3(s1_, S[l], bw);
              }
            } else {            // B = A + S
              u32 cy = 0u;
#pragma unroll
              for (int l = 0; l < L; l++) {
                const u32 bl = B[g][l];
                B[g][l] = xor3(bl, S[l], cy);
                cy = majority(bl, S[l], cy);
              }
            }
            if (rz_g[g] != rz_g[0]) load_groups(ZR, ap->rec_planes_z, ((u64)kt * (u64)ap->rec_rows_z + (u64)rz_g[0]) * (u64)ap->rec_gz, ap->rec_gz);
          }
        }
      }
      GCRE_QT(t2);
      GCRE_QT_ADD(1, t2, t1);
      // (c) the filter's interval per path, ready to use: [lo + ov, hi] packed as hi << 16 | lo; the empty interval (lo 1,
      // hi 0: "everything is outside") for delta lists and for bounds the margin pushes out of range
#pragma unroll
      for (int g = 0; g < kQSegs; g++) {
        if ((u32)g < qcnt) {
          const u32 lh = ap->ladder[lad_row + totv[g]];
          const u32 r0 = infov[g];
          const u32 ov = linfo_true_len(r0);
          const u32 lo = lh & 0xffffu;
          const u32 lo2 = lo ? lo + ov : 0u;              // counts are never negative: lo = 0 needs no margin
          lhv[g] = lh;
          lfv[g] = (!linfo_overlap(r0) || (lo2 >> L) != 0u) ? 1u : ((lh & 0xffff0000u) | lo2);
        }
      }

      GCRE_QT(t3);
      GCRE_QT_ADD(2, t3, t2);
      const u32x8 GCRE_CONSTANT* slots = (const u32x8 GCRE_CONSTANT*)ap->dlist;
      // (zu = rdlane(zunit, position): the filter pass reads it one step ahead, a scalar that comes out of a read-lane
      // cannot address a load in the next few cycles)
      auto issue_at = [&](u32 zu, u32 (&ZZ)[LZ]) {
        __amdgpu_buffer_rsrc_t rz = zt;
        u32 so = 0u;
        if constexpr (WIDE) rz = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)ap->planesz + (u64)zu * 1024u), 0, 0x7fffffff, 0x00020000);
        else so = zu;
#pragma unroll
        for (int j = 0; j < GZ; j++) {
          const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rz, lane4 * 4u + (u32)j * 1024u, so, 0);
          ZZ[4 * j + 0] = v.x; ZZ[4 * j + 1] = v.y; ZZ[4 * j + 2] = v.z; ZZ[4 * j + 3] = v.w;
        }
      };
      auto issue = [&](u32 t2, u32 (&ZZ)[LZ]) { issue_at(rdlane(zunit, t2), ZZ); };

      // ---- first pass: the bound filter.  Path t of segment g against the planes Z of the row the quad's segments all
      // add: W = B_g + Z is inside [lo + ov, hi] for every live permutation <=> no count of the path can raise a maximum
      // whatever its overlap rows say.  Paths that fail (about one in ten) -- and the rare delta-list paths -- are only
      // marked, one bit per path in a scalar mask per segment: nothing in this loop waits for anything but the planes.
      u64 todo[kQSegs] = {};
      auto filter_f = [&](int g, u32 t, const u32 (&Bg)[L], const u32 (&Z)[LZ]) {
        const u32 lf = rdlane(lfv[g], t);   // hi << 16 | lo + ov
        u32 cy = 0u, blo = 0u, bhi = 0u;
#pragma unroll
        for (int l = 0; l < L; l++) {
          u32 w;
          if (l < LZ) {
            w = xor3(Bg[l], Z[l < LZ ? l : 0], cy);
            cy = majority(Bg[l], Z[l < LZ ? l : 0], cy);
          } else {
            w = Bg[l] ^ cy;
            cy = Bg[l] & cy;
          }
          const u32 kl = (u32)__builtin_amdgcn_sbfe((int)lf, l, 1);
          const u32 kh = (u32)__builtin_amdgcn_sbfe((int)lf, 16 + l, 1);
          blo = borrow3(w, kl, blo);    // W < lo + ov
          bhi = borrow3(kh, w, bhi);    // W > hi
        }
        // (W counts the overlap twice and can pass 2^L although no count of the path does: a carry out of the top plane is
        // "above hi", not a small W)
        u32 fm = (blo | bhi | cy) & valid;
        if (__builtin_amdgcn_ballot_w64(fm != 0u) == 0ull) return;
        // ---- a flagged path-tile (one in ten).  A flagged permutation needs its own count W - S, one table cell and one
        // max: the path queues its flagged permutations with their W (the carry out of the top plane is part of it) and
        // fq_drain scores them 64 at a time -- no ladder, no whole-tile arithmetic, and the path is not marked.  Overlap
        // lists of at most 8 entries only, thresholds from the maxima only; a path with many flagged permutations in
        // one lane -- dense genotypes, where the margin eats the interval -- goes to the exact pass as before, and so
        // does everything else.
        // GCRE_IE_FLAGQ=0 keeps the second look the queue replaced: the interval above belongs to the LOWEST running
        // maximum of the tile's 2048 permutations; a flagged permutation only matters if its count can leave the (wider)
        // interval of its OWN maximum as far as this wave knows it (nm[], refreshed at every exchange).  count = W - S
        // with 0 <= S <= ov, so [W - ov, W] inside that interval settles it without a mask row. ----
        const u32 info = rdlane(infov[g], t);
        // ((info & 1u) != 0u is linfo_overlap(info) written out: with the helper here the compiler schedules this kernel
        // differently)
        if ((info & 1u) != 0u && road() != 0u && __builtin_amdgcn_ballot_w64(__builtin_popcount(fm) > GCRE_REFINE_MAX) == 0ull) {
          GCRE_QT(ts0);
#ifdef GCRE_IE_TIMING
          tm[10] += 1;
          n_flagged += (u32)__builtin_popcount(fm);
#endif
          // W again, kept this time: the filter loop above holds no plane of it
          u32 Wp[L];
          u32 c2 = 0u;
          auto sum_w = [&]() {
#pragma unroll
            for (int l = 0; l < L; l++) {
              if (l < LZ) {
                Wp[l] = xor3(Bg[l], Z[l < LZ ? l : 0], c2);
                c2 = majority(Bg[l], Z[l < LZ ? l : 0], c2);
              } else {
                Wp[l] = Bg[l] ^ c2;
                c2 = Bg[l] & c2;
              }
            }
          };
          if (road() == 2u && linfo_len(info) <= 8u) {
            // how many items the path-tile queues (at most GCRE_REFINE_MAX per lane): room is made before W is rebuilt,
            // so that a drain does not have the planes of W to keep
            u32 total = 0u;
            {
              u32 f = fm;
              asm volatile("" : "+v"(f));   // (not the ballot of the hot path: that one stays a compare into vcc)
#pragma unroll
              for (int r = 0; r < GCRE_REFINE_MAX; r++) {
                total += (u32)__builtin_popcountll(__builtin_amdgcn_ballot_w64(f != 0u));
                f &= f - 1u;
              }
            }
            if (total <= kFqCap) {
              if (fq_n + total > kFqCap) fq_drain();
              sum_w();
              const u32 q = firstg[g] + t;
              while (__builtin_amdgcn_ballot_w64(fm != 0u) != 0ull) {   // one flagged permutation per lane and round
                const bool has = fm != 0u;
                const u32 bb = has ? (u32)__builtin_ctz(fm) : 0u;
                fm &= fm - 1u;
                u32 cnt = ((c2 >> bb) & 1u) << L;   // the carry out of the top plane is part of W
#pragma unroll
                for (int l = 0; l < L; l++) cnt |= ((Wp[l] >> bb) & 1u) << l;
                const u64 hm = __builtin_amdgcn_ballot_w64(has);
                const u32 pos = fq_n + __builtin_amdgcn_mbcnt_hi((u32)(hm >> 32), __builtin_amdgcn_mbcnt_lo((u32)hm, 0u));
                if (has) {
                  fq[0][pos] = q;
                  fq[1][pos] = cnt | (bb << 17) | ((u32)lane << 22);
                }
                fq_n += (u32)__builtin_popcountll(hm);
              }
              n_slow++;
              GCRE_QT(ts1);
              GCRE_QT_ADD(8, ts1, ts0);
              return;
            }
          }
          // the second look at the ladder: the old road, and what the queue does not take (lists of more than 8 entries:
          // marking those at once, as first planned, took the exact pass of the level-4 launch from 2.8 to 6.4 of a
          // wave's 41 Mcycles and the gain with it)
          const u32 ov = linfo_true_len(info);
          const u32* lad_t = ap->ladder + rdlane(totv[g], t);
          sum_w();
          bool unsafe = false;
          while (__builtin_amdgcn_ballot_w64(fm != 0u) != 0ull) {   // one flagged permutation per lane and round
            const bool has = fm != 0u;
            const u32 bb = has ? (u32)__builtin_ctz(fm) : 0u;
            fm &= fm - 1u;
            u32 cnt = ((c2 >> bb) & 1u) << L;   // the carry out of the top plane is part of W
#pragma unroll
            for (int l = 0; l < L; l++) cnt |= ((Wp[l] >> bb) & 1u) << l;
            if (has) {
              int j = (int)(__uint_as_float(nm[bb * 64]) * (float)kLadderPerUnit);
              j = j < 0 ? 0 : (j > kLadderLevels - 1 ? kLadderLevels - 1 : j);
              const u32 lh = lad_t[(u32)j * (u32)ap->ladder_stride];
              const u32 lo = lh & 0xffffu, hi = lh >> 16;
              // every count in [max(0, W - ov), W] inside [lo, hi]?  (counts are never negative: lo = 0 needs no margin)
              if (cnt > hi || (lo != 0u && cnt < lo + ov)) unsafe = true;
            }
          }
          GCRE_QT(ts1);
          GCRE_QT_ADD(8, ts1, ts0);
          if (__builtin_amdgcn_ballot_w64(unsafe) == 0ull) return;
        }
        todo[g] |= 1ull << t;
      };

      // The pass is decided once per quad.  Rows of another shard (the ladder's all-inside row) skip it with its loads:
      // nothing of theirs is scored, so nothing is examined -- neither a carry out of the top plane nor a delta list may
      // send such a path to the second look or the exact pass.  (No launch has such quads today: segments outside the
      // scored range exist only for rows that get count planes, and those joins stay on k_null_ie_m1.)  Every other
      // quad takes the loop made for its number of
      // segments.  The planes of the next added row are in flight while the quad's paths are tested against the current
      // one; the last one or two positions are peeled, so that no row is requested twice and every iteration of the
      // loop has the same loads in flight.
      if (lad_row != lad_keep && npaths != 0u) {
        with_count<kQSegs>(qcnt, [&](auto ns) {
          u32 ZA[LZ], ZB[LZ];
          auto position = [&](u32 t, const u32 (&Z)[LZ]) {
#pragma unroll
            for (int g = 0; g < decltype(ns)::value; g++) filter_f(g, t, B[g], Z);
          };
          issue(0u, ZA);
          u32 zu = rdlane(zunit, 1u);   // (a lane past the quad's last path is read and not used)
          u32 t = 0u;
          for (; t + 2u < npaths; t += 2u) {
            issue_at(zu, ZB);
            zu = rdlane(zunit, t + 2u);
            position(t, ZA);
            issue_at(zu, ZA);
            zu = rdlane(zunit, t + 3u);
            position(t + 1u, ZB);
          }
          if (t + 1u < npaths) {
            issue_at(zu, ZB);
            position(t, ZA);
            position(t + 1u, ZB);
          } else {
            position(t, ZA);
          }
        });
      }

      GCRE_QT(t4);
      GCRE_QT_ADD(3, t4, t3);
      // ---- second pass: the marked paths, exactly.  The planes of the added row again, the mask rows of the list's real
      // entries, count = B + Nz - S (or B + S), the interval test, look-ups for what falls outside -- with the loads of
      // the next marked path in flight while this one is computed.
      struct Item { u32 t, info, lov, tot, lh; u32x8 o; };
      auto item_meta = [&](int g, u32 t) -> Item {
        Item it;
        const u64 q = (u64)firstg[g] + t;
        it.t = t;
        it.info = rdlane(infov[g], t);
        it.lh = rdlane(lhv[g], t);
        it.lov = (u32)q;                  // where a long list continues is only read for a long list (exact_f)
        it.tot = rdlane(totv[g], t);
        it.o = slots[q];
        return it;
      };
      auto item_issue = [&](const Item& it, u32 (&yy)[8], u32 (&ZZ)[LZ]) {
        const u32 ov = linfo_true_len(it.info);
#pragma unroll
        for (int j = 0; j < 8; j++) {
          yy[j] = 0u;
          if ((u32)j < ov) yy[j] = __builtin_amdgcn_raw_buffer_load_b32(mt, lane4, it.o[j], 0);   // padding entries are not fetched
        }
        if (linfo_overlap(it.info)) issue(it.t, ZZ);
      };
      auto exact_f = [&](const Item& it, const u32 (&Bg)[L], const u32 (&y)[8], const u32 (&Z)[LZ]) {
        const u32 len = linfo_len(it.info);
        const bool overlap = linfo_overlap(it.info);
        const u32 lo = it.lh & 0xffffu, hi = it.lh >> 16;
        u32 S4[4];
        sum8(y, S4);
        u32 S[L];
#pragma unroll
        for (int l = 0; l < L; l++) S[l] = (l < 4) ? S4[l < 4 ? l : 0] : 0u;
        if (len > 8u) {   // long list: further blocks of 8 entries
          const u32 GCRE_CONSTANT* more = (const u32 GCRE_CONSTANT*)(ap->dover + ((const u32 GCRE_CONSTANT*)ap->lover)[it.lov]);
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
        if (overlap) {   // C = B + Nz - S
          u32 cy = 0u, bw = 0u;
#pragma unroll
          for (int l = 0; l < L; l++) {
            const u32 zl = (l < LZ) ? Z[l < LZ ? l : 0] : 0u;
            const u32 w = xor3(Bg[l], zl, cy);
            cy = majority(Bg[l], zl, cy);
            C[l] = xor3(w, S[l], bw);
            bw = borrow3(w, S[l], bw);
          }
        } else {         // C = B + S
          u32 cy = 0u;
#pragma unroll
          for (int l = 0; l < L; l++) {
            C[l] = xor3(Bg[l], S[l], cy);
            cy = majority(Bg[l], S[l], cy);
          }
        }
        u32 blo = 0u, bhi = 0u;
#pragma unroll
        for (int l = 0; l < L; l++) {
          const u32 kl = (u32)__builtin_amdgcn_sbfe((int)lo, l, 1);
          const u32 kh = (u32)__builtin_amdgcn_sbfe((int)hi, l, 1);
          blo = borrow3(C[l], kl, blo);    // C < lo
          bhi = borrow3(kh, C[l], bhi);    // C > hi
        }
        u32 m = (blo | bhi) & valid;
        if (__builtin_amdgcn_ballot_w64(m != 0u) == 0ull) return;
        n_slow++;
        const u32 diag = sp_diag_offset(it.tot);
        while (__builtin_amdgcn_ballot_w64(m != 0u) != 0ull) {   // one permutation per lane and round
          if (lq_n + 64u > kLqCap) lq_drain();
          const bool has = m != 0u;
          const u32 bb = has ? (u32)__builtin_ctz(m) : 0u;
          m &= m - 1u;
          u32 cnt = 0u;
#pragma unroll
          for (int l = 0; l < L; l++) cnt |= ((C[l] >> bb) & 1u) << l;
          const u64 hm = __builtin_amdgcn_ballot_w64(has);
          const u32 pos = lq_n + __builtin_amdgcn_mbcnt_hi((u32)(hm >> 32), __builtin_amdgcn_mbcnt_lo((u32)hm, 0u));
          if (has) {
            lq[0][pos] = diag + cnt;
            lq[1][pos] = bb * 64u + (u32)lane;
          }
          lq_n += (u32)__builtin_popcountll(hm);
        }
      };
#pragma unroll
      for (int g = 0; g < kQSegs; g++) {
        if ((u32)g < qcnt && todo[g] != 0ull) {
          u64 m = todo[g];
          u32 yA[8], yB[8], ZA[LZ], ZB[LZ];
#pragma unroll
          for (int l = 0; l < LZ; l++) ZA[l] = ZB[l] = 0u;
          // three stages: the list entries and totals of a marked path are read (scalar loads) while the path before it
          // has its rows and planes in flight and the one before that is computed
          auto pop = [&]() -> u32 {
            const u32 t = (u32)__builtin_ctzll(m);
            m &= m - 1ull;
            return t;
          };
          Item cur = item_meta(g, pop()), nxt = cur, aft = cur;
          bool has_n = m != 0ull, has_a = false;
          if (has_n) nxt = item_meta(g, pop());
          item_issue(cur, yA, ZA);
          for (;;) {
            if (has_n) item_issue(nxt, yB, ZB);
            has_a = m != 0ull;
            if (has_a) aft = item_meta(g, pop());
            exact_f(cur, B[g], yA, ZA);
            if (!has_n) break;
            cur = nxt; nxt = aft; has_n = has_a;
            if (has_n) item_issue(nxt, yA, ZA);
            has_a = m != 0ull;
            if (has_a) aft = item_meta(g, pop());
            exact_f(cur, B[g], yB, ZB);
            if (!has_n) break;
            cur = nxt; nxt = aft; has_n = has_a;
          }
        }
      }
      GCRE_QT(t5);
      GCRE_QT_ADD(4, t5, t4);
#ifdef GCRE_IE_TIMING
      tm[7] += 1;
#endif
    }
  }
  flush_tile();
#ifdef GCRE_IE_TIMING
  tm[6] = __builtin_amdgcn_s_memtime() - tm_begin;
  if (ap->timing && lane == 0)
    for (int i = 0; i < 11; i++) atomicAdd((unsigned long long*)ap->timing + i, (unsigned long long)tm[i]);
  if (ap->timing && n_flagged) atomicAdd((unsigned long long*)ap->timing + 11, (unsigned long long)n_flagged);
#endif
  if (ap->stats && lane == 0 && n_slow) atomicAdd(ap->stats, n_slow);
}

#define GCRE_IEQ_W(EXPR, LL, GG, RR) if (wide) { EXPR(LL, GG, RR, true); } else { EXPR(LL, GG, RR, false); }
#define GCRE_IEQ_R(EXPR, LL, GG) if (rec) { GCRE_IEQ_W(EXPR, LL, GG, true) } else { GCRE_IEQ_W(EXPR, LL, GG, false) }

#ifdef GCRE_IEQ_ONLY   // quick builds while tuning: one variant
#define GCRE_IEQ(EXPR) { (void)gz; (void)planes; GCRE_IEQ_R(EXPR, 10, 2) }
#else
#define GCRE_IEQ(EXPR)                                                     \
  if (planes <= 8) { GCRE_IEQ_R(EXPR, 8, 2) }                              \
  else if (planes <= 10) {                                                 \
    if (gz <= 2) { GCRE_IEQ_R(EXPR, 10, 2) } else { GCRE_IEQ_R(EXPR, 10, 3) }        \
  } else if (planes <= 11) {                                               \
    if (gz <= 2) { GCRE_IEQ_R(EXPR, 11, 2) } else { GCRE_IEQ_R(EXPR, 11, 3) }        \
  } else if (planes <= 12) {                                               \
    if (gz <= 2) { GCRE_IEQ_R(EXPR, 12, 2) } else { GCRE_IEQ_R(EXPR, 12, 3) }        \
  } else {                                                                 \
    if (gz <= 2) { GCRE_IEQ_R(EXPR, 16, 2) }                               \
    else if (gz == 3) { GCRE_IEQ_R(EXPR, 16, 3) }                          \
    else { GCRE_IEQ_R(EXPR, 16, 4) }                                       \
  }
#endif

// quad form: method 1, pruned, no plane output (kept joins stay on k_null_ie_m1)
hipError_t launch_null_ie_quad(const IeArgs& a, int planes, hipStream_t stream) {
  const dim3 grid((unsigned)(8 * a.waves_per_xcd / kIeWaves));
  const dim3 block(64 * kIeWaves);
  const int gz = a.gz;
  const bool rec = a.rec_slot != nullptr, wide = a.z_wide != 0u;
#define GCRE_LAUNCHQ(LL, GG, RR, WW) hipLaunchKernelGGL((k_null_ie_q<LL, GG, RR, WW>), grid, block, 0, stream, a)
  GCRE_IEQ(GCRE_LAUNCHQ)
#undef GCRE_LAUNCHQ
  return hipGetLastError();
}

int ieq_quad_segs() { return kQSegs; }

int ieq_max_waves_per_cu(int planes, int gz, bool rec, bool wide) {
  int blocks = 0;
  hipError_t e = hipSuccess;
#define GCRE_OCCQ(LL, GG, RR, WW) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_null_ie_q<LL, GG, RR, WW>, 64 * kIeWaves, 0)
  GCRE_IEQ(GCRE_OCCQ)
#undef GCRE_OCCQ
  if (e != hipSuccess || blocks < 1) blocks = 1;
  return blocks * kIeWaves;
}

}  // namespace gcre

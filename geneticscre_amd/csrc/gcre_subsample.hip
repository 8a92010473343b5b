// gcre_subsample.hip -- split-half stability of caller-given sets (gcre_score_sets_subsample): every set
// scored on random halves of the cohort and on their complements.
//   * k_subsample_masks  the masks S_b of a slab of draws by the rule of gcre_subsample.h, one draw per lane, in k_set_null's
//                        mask layout [W32p][Kpad] (draw-minor; padding rows and padding draws zero)
//   * k_subsample_null   per (set, draw): the AND+popcount of the set's union row(s) with S_b, cases and controls apart; the
//                        complement's counts as the set's totals minus them; both scores from the f64 tables of the half
//                        cohorts; per cut the draws in which half A, half B and both reach it
// k_subsample_null has the mapping, the constants and the mask stream of gcre_count_tile.h: lanes own draws (8 per lane), a
// set's words are wave-uniform (scalar loads), the mask tile goes through LDS and is shared by the block's four waves.  Its
// chunk loop is its own, count_tile's with another accumulate step (a count_tile that takes the step as a functor cost
// k_set_null 15 registers when it was tried, and this kernel stands at 243-248 of 256): it keeps two accumulators per
// half-row; which one a mask dword feeds is wave-uniform by its word index, so the chunks left of the one that holds patient
// n_cases feed the cases, the chunks right of it the controls, and only in that chunk is a set word split by constant masks.
// Every global write is a vector store or a vector atomic.  The context-side entry is in gcre_host_subsample.hip.
#include "gcre_count_tile.h"
#include "gcre_subsample.h"

#include <type_traits>

namespace gcre {
namespace {

// the low x bits set (x <= 0: none, x >= 32: all)
__device__ __forceinline__ u32 sub_below(int x) { return x <= 0 ? 0u : (x >= 32 ? 0xffffffffu : ((1u << x) - 1u)); }

static_assert(kCtPT == gcre_subsample::kSubsampleTile, "tile");

}  // namespace

// One draw per lane.  Patients are walked in order, the cases' stratum first; a finished dword goes to row c >> 5 of the
// draw's column, so a wave stores 256 contiguous bytes.  Draws at and beyond nb (up to Kpad) get zero columns.
__global__ __launch_bounds__(64) void k_subsample_masks(uint64_t seed1, int64_t b0, int nb, int n_cases, int n_ctrls, int m_cases,
                                                        int m_ctrls, int W32p, int Kpad, uint32_t* __restrict__ masks) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= Kpad) return;
  const int n = n_cases + n_ctrls;
  const int words = (n + 31) >> 5;            // <= W32p (launch_subsample_masks)
  if (r >= nb) {
    for (int k = 0; k < W32p; k++) masks[(size_t)k * Kpad + r] = 0u;
    return;
  }
  const u64 base = gcre_subsample::subsample_base(seed1, b0 + r);
  u32 rem = (u32)n_cases, need = (u32)m_cases;
  u32 word = 0;
  for (int c = 0; c < n; c++) {
    if (c == n_cases) { rem = (u32)n_ctrls; need = (u32)m_ctrls; }
    if (gcre_subsample::subsample_step(base, (u32)c, rem, need)) word |= 1u << (c & 31);
    if ((c & 31) == 31 || c == n - 1) {
      masks[(size_t)(c >> 5) * Kpad + r] = word;
      word = 0;
    }
  }
  for (int k = words; k < W32p; k++) masks[(size_t)k * Kpad + r] = 0u;
}

// M method, TPW sets per wave and set tile, OCC waves per SIMD the register allocation must admit
template <int M, int TPW, int OCC>
__global__ __launch_bounds__(kCtBlock, OCC) void k_subsample_null(const SubsampleArgs a) {
  constexpr int R = kCtR, WC = kCtWC, PT = kCtPT;
  constexpr int TPB = kCtWaves * TPW;

  __shared__ __attribute__((aligned(16))) u32 lds[2][kCtChunk];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kt = blockIdx.x % a.nkt;
  const int g = blockIdx.x / a.nkt;

  const u32 GCRE_CONSTANT* ROWS = as_const(a.rows);
  const u32 GCRE_CONSTANT* TOT = as_const(a.tot);
  const double GCRE_CONSTANT* CUT = as_const(a.cut);

  const int nchunks = a.W32p / WC;

  // the chunk that holds patient n_cases, and per dword of it the bits that are cases
  const int cbx = (a.n_cases >> 5) / WC;
  const int cb = cbx < nchunks ? cbx : nchunks - 1;
  u32 cm[WC];
#pragma unroll
  for (int w = 0; w < WC; w++) cm[w] = sub_below(a.n_cases - 32 * (cb * WC + w));

  // whether the draw of each register is one of the K (the padding up to Kpad never counts, and is never looked up)
  bool live[R];
#pragma unroll
  for (int j = 0; j < R; j++) live[j] = kt * PT + ct_col(lane, j) < a.K;

  MaskStream ms(lds, a.masks + (size_t)kt * PT, a.Kpad);   // column offset of this draw tile

  const size_t rs = (size_t)M * a.W32p;   // dwords per set: (+) half, then (-) half (method 2)

  for (i64 pt = g; pt < a.npt; pt += a.pgroups) {
    const i64 qbase = pt * TPB + (i64)wave * TPW;
    u32 acc[M][2][TPW][R];                // [half-row][cases, controls]
#pragma unroll
    for (int h = 0; h < M; h++)
#pragma unroll
      for (int k = 0; k < 2; k++)
#pragma unroll
        for (int t = 0; t < TPW; t++)
#pragma unroll
          for (int j = 0; j < R; j++) acc[h][k][t][j] = 0u;

    // row offsets of this wave's sets, wave-uniform; a set past the end reads the last set's row (its result is dropped)
    size_t o[TPW];
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const i64 q = qbase + t < a.nsets ? qbase + t : a.nsets - 1;
      o[t] = (size_t)q * rs;
    }

    // software pipeline over the flattened (chunk, set) sequence, as count_tile
    u32x4 nx[M];
    auto fetch = [&](int c, int t) {
      const u32 GCRE_CONSTANT* b = ROWS + o[t] + (size_t)c * WC;
      nx[0] = *(const u32x4 GCRE_CONSTANT*)b;
      if constexpr (M == 2) nx[1] = *(const u32x4 GCRE_CONSTANT*)(b + a.W32p);
    };
    fetch(0, 0);

    // one chunk; SIDE 0: every dword feeds the cases, 2: the controls, 1: the chunk of the boundary, split by cm
    auto chunk = [&](int c, auto side) {
      constexpr int SIDE = decltype(side)::value;
      const int cn = (c + 1 == nchunks) ? 0 : c + 1;
      ms.load(cn);   // the next chunk of the stream

      u32 m[WC][R];
      ms.read(m);

#pragma unroll
      for (int t = 0; t < TPW; t++) {
        u32 jn[M][WC];
#pragma unroll
        for (int h = 0; h < M; h++)
#pragma unroll
          for (int w = 0; w < WC; w++) jn[h][w] = __builtin_amdgcn_readfirstlane(nx[h][w]);
        if (t + 1 < TPW) fetch(c, t + 1);
        else fetch(cn, 0);
#pragma unroll
        for (int h = 0; h < M; h++)
#pragma unroll
          for (int w = 0; w < WC; w++) {
            if constexpr (SIDE == 1) {
              const u32 jc = jn[h][w] & cm[w], jt = jn[h][w] & ~cm[w];   // scalar
#pragma unroll
              for (int j = 0; j < R; j++) {
                acc[h][0][t][j] += __builtin_popcount(jc & m[w][j]);
                acc[h][1][t][j] += __builtin_popcount(jt & m[w][j]);
              }
            } else {
#pragma unroll
              for (int j = 0; j < R; j++) acc[h][SIDE / 2][t][j] += __builtin_popcount(jn[h][w] & m[w][j]);
            }
          }
        __builtin_amdgcn_sched_barrier(0);   // keep each set's scalar loads in its own region
      }

      ms.store_flip();
    };
    for (int c = 0; c < cb; c++) chunk(c, std::integral_constant<int, 0>{});
    chunk(cb, std::integral_constant<int, 1>{});
    for (int c = cb + 1; c < nchunks; c++) chunk(c, std::integral_constant<int, 2>{});

    // ---- per set: the complement's counts, the two look-ups, the compares by ballot, the adds, the optional stores ----
#pragma unroll
    for (int t = 0; t < TPW; t++) {
      const i64 q = qbase + t;
      if (q >= a.nsets) continue;   // wave-uniform
      const u32 GCRE_CONSTANT* T = TOT + (size_t)q * (2 * M);
      double sa[R], sb[R];
#pragma unroll
      for (int j = 0; j < R; j++) {
        // half A: table_a[cases of P][controls of P] (+ table_a[controls of N][cases of N], in this order)
        const u64 pc = acc[0][0][t][j], pt_ = acc[0][1][t][j];
        sa[j] = a.dvt_a[live[j] ? tri_index(pc + pt_) + pc : 0];
        if constexpr (M == 2) {
          const u64 nc = acc[1][0][t][j], nt = acc[1][1][t][j];
          sa[j] = sa[j] + a.dvt_a[live[j] ? tri_index(nc + nt) + nt : 0];
        }
        sb[j] = 0.0;
        if (a.dvt_b) {              // uniform over the grid
          const u64 qc = (u64)T[0] - pc, qt = (u64)T[1] - pt_;
          sb[j] = a.dvt_b[live[j] ? tri_index(qc + qt) + qc : 0];
          if constexpr (M == 2) {
            const u64 nc = (u64)T[2] - acc[1][0][t][j], nt = (u64)T[3] - acc[1][1][t][j];
            sb[j] = sb[j] + a.dvt_b[live[j] ? tri_index(nc + nt) + nt : 0];
          }
        }
      }
      for (int jc = 0; jc < a.n_cut; jc++) {
        const double cv = CUT[(size_t)q * a.n_cut + jc];
        u32 na = 0, nb = 0, nab = 0;
#pragma unroll
        for (int j = 0; j < R; j++) {
          const bool ga = live[j] && sa[j] >= cv;   // a NaN score never counts
          na += (u32)__popcll(__ballot(ga));
          if (a.dvt_b) {
            const bool gb = live[j] && sb[j] >= cv;
            nb += (u32)__popcll(__ballot(gb));
            nab += (u32)__popcll(__ballot(ga && gb));
          }
        }
        if (lane == 0) {
          const size_t at = (size_t)q * a.n_cut + jc;
          if (na != 0u) atomicAdd(a.n_a + at, (unsigned long long)na);
          if (nb != 0u) atomicAdd(a.n_b + at, (unsigned long long)nb);
          if (nab != 0u) atomicAdd(a.n_both + at, (unsigned long long)nab);
        }
      }
      if (a.scores_a) {
        double* out = a.scores_a + (size_t)q * (size_t)a.stride + (size_t)kt * PT;
#pragma unroll
        for (int j = 0; j < R; j++)
          if (live[j]) out[ct_col(lane, j)] = sa[j];
      }
      if (a.scores_b) {
        double* out = a.scores_b + (size_t)q * (size_t)a.stride + (size_t)kt * PT;
#pragma unroll
        for (int j = 0; j < R; j++)
          if (live[j]) out[ct_col(lane, j)] = sb[j];
      }
    }
  }
}

hipError_t launch_subsample_masks(uint64_t seed1, int64_t b0, int nb, int n_cases, int n_ctrls, int m_cases, int m_ctrls, int W32p,
                                  int Kpad, uint32_t* masks, hipStream_t stream) {
  if (Kpad == 0) return hipSuccess;
  if (Kpad % 64 != 0 || nb > Kpad || (n_cases + n_ctrls + 31) / 32 > W32p) return hipErrorInvalidValue;
  if (g_launch_trace) fprintf(stderr, "launch k_subsample_masks draws=%d of %d\n", nb, Kpad);
  hipLaunchKernelGGL(k_subsample_masks, dim3((unsigned)(Kpad / 64)), dim3(64), 0, stream, seed1, b0, nb, n_cases, n_ctrls, m_cases,
                     m_ctrls, W32p, Kpad, masks);
  return hipGetLastError();
}

hipError_t launch_subsample_null(const SubsampleArgs& a, int method, hipStream_t stream) {
  if (a.nsets == 0 || a.K == 0) return hipSuccess;
  if ((int64_t)a.nkt * a.pgroups > 0x7fffffff || a.W32p % kCtWC != 0 || a.W32p < kCtWC || a.Kpad % kCtPT != 0 ||
      (int64_t)a.nkt * kCtPT > a.Kpad || a.K > a.Kpad || a.stride < a.Kpad || a.n_cut < 0 ||
      a.n_cut > gcre_subsample::kSubsampleMaxCuts || (a.n_cut > 0 && (!a.cut || !a.n_a)) || (a.dvt_b && a.n_cut > 0 && (!a.n_b || !a.n_both)))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.nkt * a.pgroups));
  if (g_launch_trace)
    fprintf(stderr, "launch k_subsample_null npt=%lld pgroups=%d draws=%d cuts=%d\n", (long long)a.npt, a.pgroups, a.K, a.n_cut);
  if (method == 1) hipLaunchKernelGGL((k_subsample_null<1, 4, 2>), grid, dim3(kCtBlock), 0, stream, a);
  else hipLaunchKernelGGL((k_subsample_null<2, 2, 2>), grid, dim3(kCtBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre

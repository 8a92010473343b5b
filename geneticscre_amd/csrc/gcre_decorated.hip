// gcre_decorated.hip -- decorated p-values (getDecoratedPvalues / computeDecoratedPvalue, R/DecoratedPvalue.R:48-304).
//   * gcre_decorated_splits   host stage: the splits of every path, their counts, observed scores and urn parameters
//   * k_decorated_observed    the observed score of every split, read from the device's value table
//   * k_decorated_null        one lane per (split, permutation): the urn draws, the permutation score, the count of
//                             permutation scores >= the observed one
// The context-side entry, gcre_decorated_pvalues, is in gcre_host_stats.hip.  DESIGN.md "Decorated p-values".
#include "../../include/gcre_hip.h"
#include "gcre_kernels.h"

#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

namespace gcre {

// Successes among k draws without replacement from an urn of `rem` balls, `need` of them successes.  Draw t reads
// u = gcre_mix64(base + t0 + t) and succeeds when floor(u * rem / 2^64) < need (k_generate_masks' idiom).  Once no success
// is left, or every ball left is one, the rest of the draws are decided: the loop stops there (the draw counter of the
// next urn starts at t0 + k all the same).
__device__ inline uint32_t dp_urn(uint64_t base, uint32_t t0, uint32_t k, uint32_t rem, uint32_t need) {
  uint32_t got = 0;
  for (uint32_t t = 0; t < k; t++) {
    if (need == 0) break;
    if (need == rem) {
      got += k - t;
      break;
    }
    const uint64_t u = gcre_mix64(base + (uint64_t)(t0 + t));
    const uint32_t pick = (uint32_t)(((unsigned __int128)u * rem) >> 64);
    if (pick < need) {
      got++;
      need--;
    }
    rem--;
  }
  return got;
}

// table[a][b] of the diagonal-major device table (-1 outside the caller's table, k_table_to_diag)
__device__ inline double dp_vt(const double* dvt, uint32_t a, uint32_t b) {
  const uint64_t t = (uint64_t)a + b;
  return dvt[t * (t + 1) / 2 + a];
}

// The score of a split when gene 2 contributes (xp cases, yp controls) to the pos half and (xn controls, yn cases) to the
// neg half (DecoratedPvalue.R:227-231 and :289-293).  Method 1 has no neg half: its terms are 0.
__device__ inline double dp_score(const double* dvt, int method, const DpUrns& s, uint32_t xp, uint32_t yp, uint32_t xn,
                                  uint32_t yn) {
  if (method == 1)
    return dp_vt(dvt, s.case_pos1 + xp + s.case_neg1 + xn, s.ctrl_pos1 + yp + s.ctrl_neg1 + yn);
  return dp_vt(dvt, s.case_pos1 + xp, s.ctrl_pos1 + yp) + dp_vt(dvt, s.case_neg1 + xn, s.ctrl_neg1 + yn);
}

__global__ __launch_bounds__(256) void k_decorated_observed(const DpUrns* urns, int S, int method, const double* dvt,
                                                            double* obs) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const DpUrns u = urns[s];
  obs[s] = dp_score(dvt, method, u, u.case_pos2, u.ctrl_pos2, u.case_neg2, u.ctrl_neg2);
}

__device__ inline int32_t uni(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline uint64_t uni64(uint64_t v) {
  return ((uint64_t)(uint32_t)uni((int32_t)(v >> 32)) << 32) | (uint32_t)uni((int32_t)v);
}

constexpr int kDpBlock = 256;

// Grid: S * tiles blocks, block b = split b / tiles, permutations [(b % tiles) * 256, +256); lane = one permutation.
// Everything about the split is wave-uniform (readfirstlane: SGPRs); only the draws and the counts are per lane.
__global__ __launch_bounds__(kDpBlock) void k_decorated_null(const DpUrns* __restrict__ urns,
                                                             const DpStratum* __restrict__ strata, int K, int tiles,
                                                             int method, const double* __restrict__ dvt,
                                                             const double* __restrict__ obs,
                                                             unsigned long long* n_ge, int32_t* perm_counts) {
  const int split = uni((int)(blockIdx.x / (unsigned)tiles));
  const int r = (int)(blockIdx.x % (unsigned)tiles) * kDpBlock + (int)threadIdx.x;
  const DpUrns* sp = urns + split;
  DpUrns u{};
  u.case_pos1 = uni(sp->case_pos1);
  u.ctrl_pos1 = uni(sp->ctrl_pos1);
  u.case_neg1 = uni(sp->case_neg1);
  u.ctrl_neg1 = uni(sp->ctrl_neg1);
  const uint32_t k_pos = (uint32_t)uni(sp->k_pos), k_neg = (uint32_t)uni(sp->k_neg);
  const int st_n = uni(sp->st_n);
  const uint64_t key = uni64(sp->key);
  const double o = __builtin_bit_cast(double, uni64(__builtin_bit_cast(uint64_t, obs[split])));
  const bool live = r < K;
  uint32_t xp = 0, xn = 0;   // cases drawn for the pos half, controls drawn for the neg half
  if (live) {
    const uint64_t base = dp_perm_base(key, r);
    if (st_n == 0) {
      xp = dp_urn(base, 0, k_pos, (uint32_t)uni(sp->pop_pos), (uint32_t)uni(sp->succ_pos));
      xn = dp_urn(base, k_pos, k_neg, (uint32_t)uni(sp->pop_neg), (uint32_t)uni(sp->succ_neg));
    } else {
      // strata ascending, pos before neg; the neg urn of a stratum holds what its pos draw left (DecoratedPvalue.R:262-272)
      const int st_off = uni(sp->st_off);
      uint32_t t0 = 0;
      for (int q = 0; q < st_n; q++) {
        const DpStratum* g = strata + st_off + q;
        const uint32_t pop = (uint32_t)uni(g->pop), cases = (uint32_t)uni(g->cases);
        const uint32_t kp = (uint32_t)uni(g->k_pos), kn = (uint32_t)uni(g->k_neg);
        const uint32_t x = dp_urn(base, t0, kp, pop, cases);
        t0 += kp;
        xn += dp_urn(base, t0, kn, pop - kp, (pop - cases) - (kp - x));
        t0 += kn;
        xp += x;
      }
    }
  }
  const double ps = dp_score(dvt, method, u, xp, k_pos - xp, xn, k_neg - xn);
  const unsigned long long ge = __ballot(live && ps >= o);
  if ((threadIdx.x & 63) == 0 && ge) atomicAdd(n_ge + split, (unsigned long long)__popcll(ge));
  if (perm_counts && live) {
    int2* pc = reinterpret_cast<int2*>(perm_counts) + (size_t)split * K + r;
    *pc = make_int2((int)xp, (int)xn);
  }
}

hipError_t launch_decorated_observed(const DpUrns* urns, int S, int method, const double* dvt, double* obs,
                                     hipStream_t stream) {
  if (S == 0) return hipSuccess;
  hipLaunchKernelGGL(k_decorated_observed, dim3((S + 255) / 256), dim3(256), 0, stream, urns, S, method, dvt, obs);
  return hipGetLastError();
}

hipError_t launch_decorated_null(const DpUrns* urns, const DpStratum* strata, int S, int K, int method, const double* dvt,
                                 const double* obs, unsigned long long* n_ge, int32_t* perm_counts, hipStream_t stream) {
  if (S == 0 || K == 0) return hipSuccess;
  const int tiles = (K + kDpBlock - 1) / kDpBlock;
  if ((int64_t)S * tiles > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_decorated_null, dim3((unsigned)(S * tiles)), dim3(kDpBlock), 0, stream, urns, strata, K, tiles,
                     method, dvt, obs, n_ge, perm_counts);
  return hipGetLastError();
}

}  // namespace gcre

namespace {

inline int popc(uint64_t w) { return __builtin_popcountll(w); }

// |a & b| over W words
inline int count_and(const uint64_t* a, const uint64_t* b, int W) {
  int c = 0;
  for (int w = 0; w < W; w++) c += popc(a[w] & b[w]);
  return c;
}

}  // namespace

extern "C" {

int gcre_decorated_splits(const gcre_dp_input* in, const double* table, int nrow, int ncol, int col_major,
                          gcre_dp_split* out, int64_t cap, int64_t* n_out) {
  if (!in || !n_out || cap < 0 || (cap > 0 && !out)) return GCRE_ERR_ARG;
  *n_out = 0;
  if ((in->method != 1 && in->method != 2) || in->n_cases <= 0 || in->n_ctrls <= 0 || in->n_paths < 0 ||
      in->n_rows < 0 || in->iterations < 0 || (in->n_paths > 0 && (!in->path_len || !in->path_rows)) ||
      (in->n_rows > 0 && !in->rows) || (table && (nrow < 0 || ncol < 0)))
    return GCRE_ERR_ARG;
  const int n = in->n_cases + in->n_ctrls;
  const int W = (n + 63) / 64;
  const bool strat = in->stratum != nullptr;
  if (strat && (in->n_strata < 1 || (cap > 0 && !in->strata_out))) return GCRE_ERR_ARG;
  int64_t S = 0;
  for (int p = 0; p < in->n_paths; p++) {
    const int L = in->path_len[p];
    if (L < 1 || L > 5) return GCRE_ERR_ARG;
    for (int i = 0; i < L; i++)
      if (in->path_rows[p * 5 + i] < -1 || in->path_rows[p * 5 + i] >= in->n_rows) return GCRE_ERR_RANGE;
    S += 2 * (L - 1);
  }
  *n_out = S;
  if (S > cap) return GCRE_ERR_RANGE;
  const int NS = strat ? in->n_strata : 0;
  if (strat)
    for (int c = 0; c < n; c++)
      if (in->stratum[c] < 0 || in->stratum[c] >= NS) return GCRE_ERR_RANGE;

  // patient classes and strata as masks; bits >= n of a carrier row are dropped by these
  std::vector<uint64_t> cases((size_t)W, 0), ctrls((size_t)W, 0), smask((size_t)NS * W, 0);
  for (int c = 0; c < n; c++) {
    (c < in->n_cases ? cases : ctrls)[(size_t)c / 64] |= uint64_t(1) << (c % 64);
    if (strat) smask[(size_t)in->stratum[c] * W + c / 64] |= uint64_t(1) << (c % 64);
  }
  // VT[a][b] the way the device holds it: -1 beyond n patients or outside the caller's table (k_table_to_diag)
  auto vt = [&](int a, int b) -> double {
    if (a > n || b > n || a >= nrow || b >= ncol) return -1.0;
    return col_major ? table[(size_t)b * nrow + a] : table[(size_t)a * ncol + b];
  };
  const double nan = std::numeric_limits<double>::quiet_NaN();

  std::vector<uint64_t> pos((size_t)5 * W), neg((size_t)5 * W), pos1((size_t)W), neg1((size_t)W), pos2((size_t)W),
      neg2((size_t)W), g((size_t)W);
  int64_t at = 0;
  for (int p = 0; p < in->n_paths; p++) {
    const int L = in->path_len[p];
    bool valid = true;
    // path_data_pos / path_data_neg (DecoratedPvalue.R:125-130)
    for (int i = 0; i < L; i++) {
      const int row = in->path_rows[p * 5 + i];
      const bool is_neg = in->method == 2 && in->path_sign && in->path_sign[p * 5 + i] == -1;
      for (int w = 0; w < W; w++) {
        const uint64_t v = row < 0 ? 0 : in->rows[(size_t)row * W + w] & (cases[w] | ctrls[w]);
        pos[(size_t)i * W + w] = is_neg ? 0 : v;
        neg[(size_t)i * W + w] = is_neg ? v : 0;
      }
      if (row < 0) valid = false;
    }
    for (int dir = 0; dir < 2; dir++)
      for (int k = 0; k < L - 1; k++) {
        // Forward j = k + 1: sub-path 1 = genes [0, j), gene 2 = j.  Backward j = L - k: sub-path 1 = genes [j - 1, L),
        // gene 2 = j - 2 (0-based)
        const int j = dir == 0 ? k + 1 : L - k;
        const int lo = dir == 0 ? 0 : j - 1, hi = dir == 0 ? j : L, g2 = dir == 0 ? j : j - 2;
        gcre_dp_split& o = out[at];
        std::memset(&o, 0, sizeof o);
        o.path = p;
        o.direction = dir;
        o.j = j;
        o.valid = valid ? 1 : 0;
        o.score = nan;
        o.pvalue = nan;
        o.strata_off = strat ? at * NS : -1;
        if (strat) std::memset(in->strata_out + at * NS, 0, sizeof(gcre_dp_stratum) * (size_t)NS);
        at++;
        if (!valid) continue;
        // pos1 / neg1 = OR of sub-path 1's rows; gene 2 minus them, within its own half (:206-209)
        for (int w = 0; w < W; w++) {
          uint64_t a = 0, b = 0;
          for (int i = lo; i < hi; i++) { a |= pos[(size_t)i * W + w]; b |= neg[(size_t)i * W + w]; }
          pos1[w] = a;
          neg1[w] = b;
          pos2[w] = pos[(size_t)g2 * W + w] & ~a;
          neg2[w] = neg[(size_t)g2 * W + w] & ~b;
        }
        // the neg half counts the other way round (:223-230)
        o.case_pos1 = count_and(pos1.data(), cases.data(), W);
        o.ctrl_pos1 = count_and(pos1.data(), ctrls.data(), W);
        o.case_neg1 = count_and(neg1.data(), ctrls.data(), W);
        o.ctrl_neg1 = count_and(neg1.data(), cases.data(), W);
        o.case_pos2 = count_and(pos2.data(), cases.data(), W);
        o.ctrl_pos2 = count_and(pos2.data(), ctrls.data(), W);
        o.case_neg2 = count_and(neg2.data(), ctrls.data(), W);
        o.ctrl_neg2 = count_and(neg2.data(), cases.data(), W);
        o.cases1 = o.case_pos1 + o.case_neg1;
        o.ctrls1 = o.ctrl_pos1 + o.ctrl_neg1;
        o.cases2 = o.case_pos2 + o.case_neg2;
        o.ctrls2 = o.ctrl_pos2 + o.ctrl_neg2;
        if (table) {
          if (in->method == 1)
            o.score = vt(o.case_pos1 + o.case_pos2 + o.case_neg1 + o.case_neg2,
                         o.ctrl_pos1 + o.ctrl_pos2 + o.ctrl_neg1 + o.ctrl_neg2);
          else
            o.score = vt(o.case_pos1 + o.case_pos2, o.ctrl_pos1 + o.ctrl_pos2) +
                      vt(o.case_neg1 + o.case_neg2, o.ctrl_neg1 + o.ctrl_neg2);
        }
        if (!strat) {
          // draw |pos2| from the complement of pos1 and |neg2| from the complement of neg1, independently (:278-280)
          o.k_pos = o.case_pos2 + o.ctrl_pos2;
          o.pop_pos = n - o.case_pos1 - o.ctrl_pos1;
          o.succ_pos = in->n_cases - o.case_pos1;
          o.k_neg = o.case_neg2 + o.ctrl_neg2;
          o.pop_neg = n - o.case_neg1 - o.ctrl_neg1;
          o.succ_neg = in->n_ctrls - o.case_neg1;
          continue;
        }
        // G_s = stratum s minus both halves of sub-path 1; gene-2 carriers outside G_s are not drawn (:240-247)
        gcre_dp_stratum* st = in->strata_out + o.strata_off;
        for (int s = 0; s < NS; s++) {
          const uint64_t* sm = smask.data() + (size_t)s * W;
          for (int w = 0; w < W; w++) g[w] = sm[w] & ~(pos1[w] | neg1[w]);
          st[s].pop = count_and(g.data(), g.data(), W);
          st[s].cases = count_and(g.data(), cases.data(), W);
          st[s].k_pos = count_and(g.data(), pos2.data(), W);
          st[s].k_neg = count_and(g.data(), neg2.data(), W);
          o.k_pos += st[s].k_pos;
          o.k_neg += st[s].k_neg;
        }
      }
  }
  return GCRE_OK;
}

}  // extern "C"

// gcre_weighted.h -- covariate-adjusted permutation masks (gcre_generate_weighted_masks), defined once: the
// target law, its calibration to 32-bit thresholds, what the entry refuses of its own arguments, the plan (expected attempts)
// and the draw rule.  Plain C++17 over include/gcre_hip.h, no HIP: the kernels of gcre_weighted.hip include it under hipcc,
// where the draw functions are __host__ __device__, the host stage (gcre_host_weighted.hip) too, and
// tests/native/weighted_main.cpp under plain g++.  report.weighted_masks restates the draw rule in numpy.
//
// Target law (Epstein et al. 2012; Fisher's non-central hypergeometric law with one patient per class).  Inside stratum s,
// with Z_s its patients and cases_s those among the columns < n_cases, mask r is a subset A of Z_s with |A| = cases_s and
// P(A) proportional to the product of odds_c over c in A; the strata are independent.  Equal odds give the uniform law of
// gcre_generate_perm_masks (not its bits).
//
// Calibration.  The law does not change when the odds of a stratum are multiplied by a constant, so per stratum the odds are
// divided by their maximum (w_c in [0, 1]; a power-of-two rescaling of a stratum's odds therefore changes nothing at all) and
// the tilt t_s is found by bisection on x = log2 t_s such that p_c = t_s w_c / (1 + t_s w_c) sums to cases_s over Z_s.  Then
// thr_c = min(floor(p_c 2^32), 2^32 - 1), and from there on the thresholds ARE the definition: what is sampled is conditional
// Bernoulli with p_c = thr_c / 2^32, exactly.  Degenerate strata: cases_s = 0 gives thr = 0 throughout; cases_s = the
// patients with positive odds (cases_s = |Z_s| among them) gives 2^32 - 1 for those and 0 for the others.
//
// Tolerance (weighted_sum_bound).  The bisection ends when the interval of x holds no further double: |x| < 4096, so x is
// within 2^-41 of the root, t within a factor 1 + ln 2 * 2^-41, and sum p within V ln 2 * 2^-41 <= |Z_s| 2^-44 (V = sum p (1 -
// p) <= |Z_s| / 4).  The sum itself is a plain loop over at most |Z_s| terms <= 1: rounding below |Z_s|^2 2^-52.  The floor
// (and the clamp of p = 1) take less than 2^-32 per patient.  Hence | sum thr_c / 2^32 - cases_s | < |Z_s| (2^-32 + 2^-44) +
// |Z_s|^2 2^-52.
//
// The draw: exact rejection in integers.  Attempt a = 0, 1, 2, ... of (permutation r, stratum s) labels patient c of Z_s a
// case when a 32-bit uniform is below thr_c.  One gcre_mix64 serves two attempts -- its HIGH half goes to the even attempt 2j,
// its LOW half to the odd attempt 2j + 1:
//   seed'    = gcre_mix64(seed ^ kWeightedTag)                              (a tag no other stream of gcre_kernels.h uses)
//   key_r    = gcre_mix64(seed' ^ (0x51ed270b7f3c9a1d * (r + 1)))
//   base_rs  = gcre_mix64(key_r ^ (0xd1b54a32d192ed03 * (s + 1)))
//   pair_rsj = gcre_mix64(base_rs + j)                                      j = a >> 1
//   u        = gcre_mix64(pair_rsj + c)                                     c = the patient's COLUMN
//   case     = (a & 1 ? (uint32_t)u : (uint32_t)(u >> 32)) < thr_c
// The accepted attempt a*(r, s) is the SMALLEST a whose case count over Z_s is exactly cases_s; mask r is the union over s of
// the accepted attempts.  Everything is a pure function of (seed, r, s, a, c): nothing depends on grid, batch, launch order
// or the order of Z_s in memory.  No accepted attempt below max_attempts for some (r, s): the call is refused.
#pragma once
#include "../../include/gcre_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define GCRE_WT_HD __host__ __device__
#else
#define GCRE_WT_HD
#endif

namespace gcre_weighted __attribute__((visibility("hidden"))) {

constexpr int kWeightedStrataMax = GCRE_STRATA_MAX;
constexpr uint64_t kWeightedTag = 0x7765696768746564ull;          // "weighted"
constexpr uint32_t kWeightedNone = 0xffffffffu;                   // a*(r, s) of a pair that met the cap
constexpr int64_t kWeightedDefaultAttempts = (int64_t)1 << 20;    // a cap, not a tuning knob
constexpr int64_t kWeightedAttemptLimit = (int64_t)1 << 31;       // attempts are 32-bit: a larger cap acts as this one
constexpr int kWeightedBatch = 8;                                 // attempts k_weighted_search makes per pass (four hashes a patient)

// gcre_mix64 of gcre_kernels.h, restated so that a program without HIP has it (tests/test_weighted_host.py holds it against
// the library's gcre_mix64)
GCRE_WT_HD inline uint64_t wt_mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
GCRE_WT_HD inline uint64_t wt_seed(uint64_t seed) { return wt_mix64(seed ^ kWeightedTag); }
GCRE_WT_HD inline uint64_t wt_key(uint64_t seed1, uint64_t r) { return wt_mix64(seed1 ^ (0x51ed270b7f3c9a1dull * (r + 1))); }
GCRE_WT_HD inline uint64_t wt_base(uint64_t key, uint32_t s) { return wt_mix64(key ^ (0xd1b54a32d192ed03ull * ((uint64_t)s + 1))); }
GCRE_WT_HD inline uint64_t wt_pair(uint64_t base, uint32_t j) { return wt_mix64(base + (uint64_t)j); }
// the two uniforms of patient column c under attempt pair j: high half for attempt 2j, low half for attempt 2j + 1
GCRE_WT_HD inline uint64_t wt_draw(uint64_t pair, uint32_t c) { return wt_mix64(pair + (uint64_t)c); }
GCRE_WT_HD inline bool wt_case(uint64_t u, uint32_t a, uint32_t thr) {
  return ((a & 1u) ? (uint32_t)u : (uint32_t)(u >> 32)) < thr;
}

// | sum thr_c / 2^32 - cases_s | stays below this for a stratum of `size` patients (derived above)
inline double weighted_sum_bound(uint32_t size) {
  const double z = (double)size;
  return z * (std::ldexp(1.0, -32) + std::ldexp(1.0, -44)) + z * z * std::ldexp(1.0, -52);
}

struct WeightedPlan {
  int ns = 0;
  std::vector<uint32_t> cases_in, size_of, npos;   // per stratum: cases (columns < n_cases), patients, patients with odds > 0
  std::vector<uint32_t> thr;                       // [n], by column
  std::vector<double> expected;                    // per stratum: sqrt(2 pi V), V = sum p (1 - p) over the thresholds; 1 at the least
};

// sqrt(2 pi V) of the thresholds as they are: the attempts one (r, s) takes on average
inline double expected_attempts(const uint32_t* thr, const int32_t* stratum, int32_t n, int s) {
  double V = 0;
  for (int32_t c = 0; c < n; c++)
    if ((stratum ? stratum[c] : 0) == s) {
      const double p = (double)thr[c] * std::ldexp(1.0, -32);
      V += p * (1.0 - p);
    }
  return std::max(1.0, std::sqrt(2.0 * 3.14159265358979323846 * V));
}

// The strata, the refusals and the thresholds.  GCRE_OK, or GCRE_ERR_ARG with `msg` naming the stratum.
inline int weighted_plan(int32_t n, int32_t n_cases, const double* odds, const int32_t* stratum, int n_strata, const std::string& who,
                         WeightedPlan& pl, std::string& msg) {
  if (!odds) { msg = who + ": NULL argument (odds)"; return GCRE_ERR_ARG; }
  if (n < 0 || n_cases < 0 || n_cases > n) { msg = who + ": n_cases outside 0 .. n"; return GCRE_ERR_ARG; }
  if (stratum && (n_strata < 1 || n_strata > kWeightedStrataMax)) {
    msg = who + ": n_strata = " + std::to_string(n_strata) + " outside 1 .. GCRE_STRATA_MAX = " + std::to_string(kWeightedStrataMax);
    return GCRE_ERR_ARG;
  }
  const int ns = stratum ? n_strata : 1;
  pl.ns = ns;
  pl.cases_in.assign((size_t)ns, 0u);
  pl.size_of.assign((size_t)ns, 0u);
  pl.npos.assign((size_t)ns, 0u);
  pl.thr.assign((size_t)n, 0u);
  pl.expected.assign((size_t)ns, 1.0);
  std::vector<double> wmax((size_t)ns, 0.0);
  for (int32_t c = 0; c < n; c++) {
    const int s = stratum ? stratum[c] : 0;
    if (s < 0 || s >= ns) {
      msg = who + ": stratum id " + std::to_string(s) + " of patient " + std::to_string(c) + " outside 0 .. " + std::to_string(ns - 1);
      return GCRE_ERR_ARG;
    }
    const double w = odds[c];
    if (!(w >= 0.0) || std::isinf(w)) {
      msg = who + ": the odds of patient " + std::to_string(c) + " (stratum " + std::to_string(s) + ") must be finite and >= 0, not " +
            std::to_string(w);
      return GCRE_ERR_ARG;
    }
    pl.size_of[(size_t)s]++;
    if (c < n_cases) pl.cases_in[(size_t)s]++;
    if (w > 0.0) pl.npos[(size_t)s]++;
    wmax[(size_t)s] = std::max(wmax[(size_t)s], w);
  }
  for (int s = 0; s < ns; s++)
    if (pl.npos[(size_t)s] < pl.cases_in[(size_t)s]) {
      msg = who + ": stratum " + std::to_string(s) + " has " + std::to_string(pl.npos[(size_t)s]) +
            " patients with positive odds, fewer than its " + std::to_string(pl.cases_in[(size_t)s]) + " cases";
      return GCRE_ERR_ARG;
    }
  std::vector<double> lw;   // log2 w_c of the stratum's patients with positive odds
  std::vector<int32_t> who_c;
  for (int s = 0; s < ns; s++) {
    const uint32_t m = pl.cases_in[(size_t)s], np = pl.npos[(size_t)s];
    if (m == 0) continue;   // every threshold 0
    lw.clear();
    who_c.clear();
    for (int32_t c = 0; c < n; c++)
      if ((stratum ? stratum[c] : 0) == s && odds[c] > 0.0) {
        who_c.push_back(c);
        lw.push_back(std::log2(odds[c] / wmax[(size_t)s]));   // <= 0
      }
    if (m == np) {
      for (int32_t c : who_c) pl.thr[(size_t)c] = 0xffffffffu;
    } else {
      // f(x) = sum 1 / (1 + 2^-(x + lw_c)) rises in x.  w <= 1: f <= np t / (1 + t), so t >= m / (np - m) is below the root;
      // w >= wmin: t <= m / ((np - m) wmin) is above it.
      auto f = [&](double x) {
        double sum = 0;
        for (double l : lw) {
          const double z = x + l;
          sum += z >= 0 ? 1.0 / (1.0 + std::exp2(-z)) : std::exp2(z) / (1.0 + std::exp2(z));
        }
        return sum;
      };
      const double lmin = *std::min_element(lw.begin(), lw.end());
      double lo = std::log2((double)m / (double)(np - m)) - 1.0, hi = lo + 2.0 - lmin;
      for (;;) {
        const double mid = lo + (hi - lo) * 0.5;
        if (!(mid > lo && mid < hi)) break;
        if (f(mid) < (double)m) lo = mid; else hi = mid;
      }
      for (size_t i = 0; i < lw.size(); i++) {
        const double z = lo + lw[i];
        const double p = z >= 0 ? 1.0 / (1.0 + std::exp2(-z)) : std::exp2(z) / (1.0 + std::exp2(z));
        const double q = std::floor(std::ldexp(p, 32));
        pl.thr[(size_t)who_c[i]] = q >= 4294967295.0 ? 0xffffffffu : (uint32_t)q;
      }
    }
    pl.expected[(size_t)s] = expected_attempts(pl.thr.data(), stratum, n, s);
  }
  return GCRE_OK;
}

// the cap as the kernels read it, or a refusal
inline int weighted_cap(int64_t max_attempts, const std::string& who, uint32_t& cap, std::string& msg) {
  if (max_attempts < 1) {
    msg = who + ": max_attempts = " + std::to_string(max_attempts) + " must be at least 1";
    return GCRE_ERR_ARG;
  }
  cap = (uint32_t)std::min(max_attempts, kWeightedAttemptLimit);
  return GCRE_OK;
}

// refused before any launch: a stratum whose estimate alone exceeds the cap
inline int weighted_plan_fits(const WeightedPlan& pl, uint32_t cap, const std::string& who, std::string& msg) {
  for (int s = 0; s < pl.ns; s++)
    if (pl.expected[(size_t)s] > (double)cap) {
      msg = who + ": stratum " + std::to_string(s) + " needs about " + std::to_string((long long)std::ceil(pl.expected[(size_t)s])) +
            " attempts per permutation, above max_attempts = " + std::to_string(cap);
      return GCRE_ERR_RANGE;
    }
  return GCRE_OK;
}

// the one refusal that comes after launches
inline std::string weighted_left_message(const std::string& who, long long left, long long perms, uint32_t cap) {
  return who + ": " + std::to_string(left) + " of " + std::to_string(perms) +
         " permutations were left over without an accepted attempt below max_attempts = " + std::to_string(cap) +
         ": the context's masks are unchanged";
}

// a*(r, s) on the host: the smallest accepted attempt below `cap`, or kWeightedNone.  cols: the columns of Z_s, any order.
inline uint32_t weighted_search(uint64_t seed, uint64_t r, uint32_t s, const int32_t* cols, size_t size, const uint32_t* thr,
                                uint32_t cases, uint32_t cap) {
  const uint64_t base = wt_base(wt_key(wt_seed(seed), r), s);
  for (uint32_t j = 0; 2 * (uint64_t)j < cap; j++) {
    const uint64_t pair = wt_pair(base, j);
    uint32_t even = 0, odd = 0;
    for (size_t i = 0; i < size; i++) {
      const uint64_t u = wt_draw(pair, (uint32_t)cols[i]);
      even += wt_case(u, 0, thr[cols[i]]) ? 1u : 0u;
      odd += wt_case(u, 1, thr[cols[i]]) ? 1u : 0u;
    }
    if (even == cases) return 2 * j;
    if (odd == cases && 2 * (uint64_t)j + 1 < cap) return 2 * j + 1;
  }
  return kWeightedNone;
}

// Mask r as packed dwords (bit c & 31 of words[c >> 5]) from the accepted attempts att[s]; `words` holds ceil(n / 32) dwords
inline void weighted_mask(uint64_t seed, uint64_t r, int32_t n, const int32_t* stratum, const uint32_t* thr, const uint32_t* att,
                          uint32_t* words) {
  const uint64_t key = wt_key(wt_seed(seed), r);
  for (int32_t k = 0; k < (n + 31) / 32; k++) words[k] = 0;
  for (int32_t c = 0; c < n; c++) {
    const uint32_t s = stratum ? (uint32_t)stratum[c] : 0u, a = att[s];
    if (wt_case(wt_draw(wt_pair(wt_base(key, s), a >> 1), (uint32_t)c), a, thr[c])) words[c >> 5] |= 1u << (c & 31);
  }
}

}  // namespace gcre_weighted

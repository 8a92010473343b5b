// weighted_main.cpp -- drives the host side of the covariate-adjusted masks (csrc/gcre_weighted.h) on one case read from a
// file, for tests/test_weighted_host.py: the refusals, the thresholds, the expected attempts, and the draw rule itself (the
// accepted attempts and the masks of the first permutations).  Plain C++: no GPU, no HIP.  The case file is a list of
// "key values..." lines:
//   n_cases C | n_ctrls T | seed S | max_attempts A | perms K
//   odds w0 w1 ...                          hexadecimal or decimal doubles ("nan", "inf" too); without the line the array is NULL
//   n_strata N | strata s0 s1 ...           without a `strata` line the array is NULL
//   left L                                  print the message of the refusal that follows a search that met the cap
// Output: "check CODE MESSAGE" first (the plan, then the cap, then whether the plan fits the cap); then, if it passed,
// "thr ...", "expected ..." (17 significant digits), "bound ..." (weighted_sum_bound of every stratum), and per permutation
// "perm R att a0 a1 ... mask w0 w1 ..." (accepted attempts per stratum, the mask as dwords); "left TEXT" lines last.  Every
// array has exactly the size the case gives it, so that a sanitizer sees any access beyond it.
#include "../../geneticscre_amd/csrc/gcre_weighted.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <sstream>

template <typename T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v, bool have) {
  std::unique_ptr<T[]> p(have ? new T[v.size()] : nullptr);
  if (have) std::copy(v.begin(), v.end(), p.get());
  return p;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line, key;
  int32_t n_cases = 1, n_ctrls = 1, n_strata = 0, perms = 0;
  uint64_t seed = 0;
  int64_t max_attempts = gcre_weighted::kWeightedDefaultAttempts;
  bool have_strata = false, have_odds = false;
  std::vector<int32_t> strata;
  std::vector<double> odds;
  std::vector<long long> lefts;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "n_cases") ls >> n_cases;
    else if (key == "n_ctrls") ls >> n_ctrls;
    else if (key == "seed") ls >> seed;
    else if (key == "max_attempts") ls >> max_attempts;
    else if (key == "perms") ls >> perms;
    else if (key == "n_strata") ls >> n_strata;
    else if (key == "strata") { have_strata = true; for (int32_t v; ls >> v;) strata.push_back(v); }
    else if (key == "odds") { have_odds = true; for (std::string v; ls >> v;) odds.push_back(std::strtod(v.c_str(), nullptr)); }
    else if (key == "left") { long long b = 0; ls >> b; lefts.push_back(b); }
    else return 2;
  }
  const int32_t n = n_cases + n_ctrls;
  if ((have_strata && (int32_t)strata.size() != n) || (have_odds && (int32_t)odds.size() != n)) return 2;
  const auto p_strata = exact(strata, have_strata);
  const auto p_odds = exact(odds, have_odds);

  const std::string who = "generate_weighted_masks";
  gcre_weighted::WeightedPlan pl;
  std::string msg;
  uint32_t cap = 0;
  int rc = gcre_weighted::weighted_plan(n, n_cases, p_odds.get(), p_strata.get(), n_strata, who, pl, msg);
  if (rc == GCRE_OK) rc = gcre_weighted::weighted_cap(max_attempts, who, cap, msg);
  if (rc == GCRE_OK) rc = gcre_weighted::weighted_plan_fits(pl, cap, who, msg);
  std::printf("check %d %s\n", rc, msg.c_str());
  if (rc == GCRE_OK) {
    std::string a = "thr";
    for (uint32_t v : pl.thr) a += " " + std::to_string(v);
    std::printf("%s\nexpected", a.c_str());
    for (double v : pl.expected) std::printf(" %.17g", v);
    std::printf("\nbound");
    for (uint32_t v : pl.size_of) std::printf(" %.17g", gcre_weighted::weighted_sum_bound(v));
    std::printf("\n");
    // the columns of every stratum, as the host stage lists them
    std::vector<std::vector<int32_t>> cols((size_t)pl.ns);
    for (int32_t c = 0; c < n; c++) cols[(size_t)(have_strata ? p_strata[c] : 0)].push_back(c);
    const size_t W = (size_t)(n + 31) / 32;
    const auto p_thr = exact(pl.thr, true);
    for (int32_t r = 0; r < perms; r++) {
      std::unique_ptr<uint32_t[]> att(new uint32_t[(size_t)pl.ns]);
      bool all = true;
      std::printf("perm %d att", r);
      for (int s = 0; s < pl.ns; s++) {
        const auto p_cols = exact(cols[(size_t)s], true);
        att[(size_t)s] = gcre_weighted::weighted_search(seed, (uint64_t)r, (uint32_t)s, p_cols.get(), cols[(size_t)s].size(), p_thr.get(),
                                                        pl.cases_in[(size_t)s], cap);
        all = all && att[(size_t)s] != gcre_weighted::kWeightedNone;
        std::printf(" %u", att[(size_t)s]);
      }
      std::printf(" mask");
      if (all) {
        std::unique_ptr<uint32_t[]> words(new uint32_t[W]);
        gcre_weighted::weighted_mask(seed, (uint64_t)r, n, p_strata.get(), p_thr.get(), att.get(), words.get());
        for (size_t k = 0; k < W; k++) std::printf(" %u", words[k]);
      }
      std::printf("\n");
    }
  }
  for (long long b : lefts) std::printf("left %s\n", gcre_weighted::weighted_left_message(who, b, perms, cap).c_str());
  return 0;
}

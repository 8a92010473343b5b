// seq_weighted_main.cpp -- drives the rule of the weighted sequential p-values (csrc/gcre_seq_weighted.h over gcre_weighted.h
// and gcre_sequential.h) on one case read from a file, for tests/test_seq_weighted_host.py: the up-front refusals, the batch
// loop of the host stage with its cut at the first left-over permutation -- the accepted attempts by weighted_search, the
// exceedances given by the caller as one bit string per set -- the launches it implies, the W32p + S batch accounting, and
// the hash chain at permutation indices no GPU test reaches.  Plain C++: no GPU, no HIP.  The case file is a list of
// "key values..." lines:
//   n_cases C | n_ctrls T | seed S | max_attempts A | n_strata N | strata s0 s1 ... | odds w0 w1 ...   as weighted_main.cpp
//   hits H | max_perms P | w32p W | max_mb M | cap_perms C | no_seq_out 1
//   set 0101...                             e[r] of one valid set, r = 0 .. max_perms - 1 ("set" alone: a set that never counts)
//   chain R S J C                           print wt_key / wt_base / wt_pair / wt_draw of permutation R (64-bit), stratum S,
//                                           attempt pair J, column C
// Output: "check CODE MESSAGE" first; then, if it passed, "dwords D", per batch "batch R0 NB FIRST KEEP ACTIVE" (FIRST -1:
// none), "launches L", "left_over R STRATUM" (-1 -1: none), "refused 0|1 MESSAGE", and per set "seq N_HIT N_PERM STOPPED";
// "chain KEY BASE PAIR DRAW" lines (hexadecimal) last, whatever the check said.
#include "../../geneticscre_amd/csrc/gcre_seq_weighted.h"

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

struct Chain { uint64_t r; uint32_t s, j, c; };

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line, key;
  int32_t n_cases = 1, n_ctrls = 1, n_strata = 0, W32p = 4;
  uint64_t seed = 0;
  int64_t max_attempts = gcre_weighted::kWeightedDefaultAttempts, h = 1, max_perms = 0, cap_perms = 0;
  double max_mb = 1024;
  bool have_strata = false, have_odds = false, have_seq_out = true;
  std::vector<int32_t> strata;
  std::vector<double> odds;
  std::vector<std::string> sets;
  std::vector<Chain> chains;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "n_cases") ls >> n_cases;
    else if (key == "n_ctrls") ls >> n_ctrls;
    else if (key == "seed") ls >> seed;
    else if (key == "max_attempts") ls >> max_attempts;
    else if (key == "n_strata") ls >> n_strata;
    else if (key == "hits") ls >> h;
    else if (key == "max_perms") ls >> max_perms;
    else if (key == "w32p") ls >> W32p;
    else if (key == "max_mb") ls >> max_mb;
    else if (key == "cap_perms") ls >> cap_perms;
    else if (key == "no_seq_out") have_seq_out = false;
    else if (key == "strata") { have_strata = true; for (int32_t v; ls >> v;) strata.push_back(v); }
    else if (key == "odds") { have_odds = true; for (std::string v; ls >> v;) odds.push_back(std::strtod(v.c_str(), nullptr)); }
    else if (key == "set") { std::string b; ls >> b; sets.push_back(b); }
    else if (key == "chain") { Chain c{}; ls >> c.r >> c.s >> c.j >> c.c; chains.push_back(c); }
    else return 2;
  }
  const int32_t n = n_cases + n_ctrls;
  if ((have_strata && (int32_t)strata.size() != n) || (have_odds && (int32_t)odds.size() != n)) return 2;
  for (const std::string& b : sets)
    if (!b.empty() && (int64_t)b.size() != max_perms) return 2;
  const auto p_strata = exact(strata, have_strata);
  const auto p_odds = exact(odds, have_odds);

  const std::string who = "score_sets_sequential_weighted";
  gcre_weighted::WeightedPlan pl;
  std::string msg;
  uint32_t cap = 0;
  int rc = gcre_sequential::check_sequential_args(h, max_perms, have_seq_out, who, msg);
  if (rc == GCRE_OK) rc = gcre_weighted::weighted_plan(n, n_cases, p_odds.get(), p_strata.get(), n_strata, who, pl, msg);
  if (rc == GCRE_OK) rc = gcre_weighted::weighted_cap(max_attempts, who, cap, msg);
  if (rc == GCRE_OK) rc = gcre_weighted::weighted_plan_fits(pl, cap, who, msg);
  std::printf("check %d %s\n", rc, msg.c_str());
  if (rc == GCRE_OK) {
    const int S = pl.ns;
    const int32_t dwords = gcre_seq_weighted::seq_weighted_dwords(W32p, S);
    std::printf("dwords %d\n", dwords);
    std::vector<std::vector<int32_t>> cols((size_t)S);
    for (int32_t c = 0; c < n; c++) cols[(size_t)(have_strata ? p_strata[c] : 0)].push_back(c);
    const auto p_thr = exact(pl.thr, true);
    const size_t V = sets.size();
    std::vector<int64_t> prior(V, 0), n_perm(V, 0);
    std::vector<size_t> act;
    for (size_t v = 0; v < V; v++) act.push_back(v);
    int64_t r0 = 0, batch = 0, left_over = -1, launches = 0;
    int left_stratum = -1;
    while (r0 < max_perms && !act.empty()) {
      batch = gcre_sequential::sequential_batch(batch, dwords, (int64_t)act.size(), max_mb, cap_perms);
      const int64_t nb = std::min(batch, max_perms - r0);
      // the search: att [S][nb], exactly so large; the first column with a stratum that met the cap
      std::unique_ptr<uint32_t[]> att(new uint32_t[(size_t)S * (size_t)nb]);
      uint32_t first = gcre_seq_weighted::kSeqWtNoColumn;
      for (int s = 0; s < S; s++) {
        const auto p_cols = exact(cols[(size_t)s], true);
        for (int64_t i = 0; i < nb; i++) {
          const uint32_t a = gcre_weighted::weighted_search(seed, (uint64_t)(r0 + i), (uint32_t)s, p_cols.get(), cols[(size_t)s].size(),
                                                            p_thr.get(), pl.cases_in[(size_t)s], cap);
          att[(size_t)s * (size_t)nb + (size_t)i] = a;
          if (a == gcre_weighted::kWeightedNone) first = std::min(first, (uint32_t)i);
        }
      }
      const gcre_seq_weighted::SeqWeightedCut cut = gcre_seq_weighted::seq_weighted_cut(r0, nb, first);
      launches += gcre_seq_weighted::seq_weighted_batch_launches(cut);
      if (cut.left_over >= 0) {
        left_over = cut.left_over;
        left_stratum = gcre_seq_weighted::seq_weighted_left_stratum(att.get(), S, (size_t)nb, (size_t)first);
      }
      // the bit rows of the columns that are scored, and the retirement
      std::vector<size_t> next;
      const size_t words = (size_t)(cut.keep + 63) / 64;
      for (size_t v : act) {
        std::unique_ptr<uint64_t[]> bits(new uint64_t[words ? words : 1]());
        for (int64_t i = 0; i < cut.keep; i++)
          if (!sets[v].empty() && sets[v][(size_t)(r0 + i)] == '1') bits[(size_t)i / 64] |= 1ull << (i & 63);
        const int64_t at = cut.keep > 0 ? gcre_sequential::sequential_find(bits.get(), cut.keep, prior[v], h) : -1;
        if (at >= 0) {
          n_perm[v] = r0 + at + 1;
        } else {
          for (size_t w = 0; w < words; w++) prior[v] += gcre_sequential::seq_popcount64(bits[w]);
          next.push_back(v);
        }
      }
      act.swap(next);
      std::printf("batch %lld %lld %lld %lld %zu\n", (long long)r0, (long long)nb,
                  first == gcre_seq_weighted::kSeqWtNoColumn ? -1ll : (long long)first, (long long)cut.keep, act.size());
      r0 += cut.keep;
      if (cut.left_over >= 0) break;
    }
    const bool refused = gcre_seq_weighted::seq_weighted_refused(left_over, (int64_t)act.size());
    std::printf("launches %lld\nleft_over %lld %d\n", (long long)launches, (long long)left_over, left_stratum);
    std::printf("refused %d %s\n", refused ? 1 : 0,
                refused ? gcre_seq_weighted::seq_weighted_message(who, left_over, left_stratum, cap, (int64_t)act.size(), max_perms).c_str() : "");
    for (size_t v = 0; v < V; v++) {
      const bool stopped = n_perm[v] != 0;
      std::printf("seq %lld %lld %d\n", (long long)(stopped ? h : prior[v]), (long long)(stopped ? n_perm[v] : (left_over >= 0 ? left_over : max_perms)),
                  stopped ? 1 : 0);
    }
  }
  for (const Chain& c : chains) {
    const uint64_t k = gcre_weighted::wt_key(gcre_weighted::wt_seed(seed), c.r), b = gcre_weighted::wt_base(k, c.s),
                   p = gcre_weighted::wt_pair(b, c.j), u = gcre_weighted::wt_draw(p, c.c);
    std::printf("chain %016llx %016llx %016llx %016llx\n", (unsigned long long)k, (unsigned long long)b, (unsigned long long)p,
                (unsigned long long)u);
  }
  return 0;
}

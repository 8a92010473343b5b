// compete_main.cpp -- drives the draw rule and the argument checks of gcre_score_sets_compete (csrc/gcre_compete.h) on one
// case read from a file, for tests/test_compete_host.py.  Plain C++: no GPU, no HIP.  The case file is a list of
// "key values..." lines:
//   n_rows R | n_bins NB | bin ...                      the pool; without a `bin` line the list is NULL (one bin)
//   n_sets S | set_off ... | members ...                the set list
//   draws D | have_n_ge 0/1 | want_null 0/1 | want_picks 0/1 | max_mb F     what the check is told
//   seed X | attempts A | pick S B                      print the picks of draw B of set S (any number of `pick` lines)
//   mix Z                                               print compete_mix64(Z) (any number)
// Output: "check CODE MESSAGE" first; then, if the check passed, one "picks S B r0 r1 ..." line per `pick` line; "mix Z V"
// lines last.  Every array has exactly the size the case gives it, so that a sanitizer sees any access beyond it.
#include "../../geneticscre_amd/csrc/gcre_compete.h"

#include <cstdio>
#include <fstream>
#include <memory>
#include <sstream>
#include <utility>

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line, key;
  gcre_set_input in{};
  int32_t n_bins = 1;
  int64_t draws = 0;
  int have_n_ge = 1, want_null = 0, want_picks = 0, attempts = gcre_compete::kCompeteAttempts;
  double max_mb = 1024;
  uint64_t seed = 0;
  bool have_bin = false;
  std::vector<int64_t> set_off;
  std::vector<int32_t> members, bin;
  std::vector<std::pair<int64_t, int64_t>> pick;
  std::vector<uint64_t> mix;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "n_rows") ls >> in.n_rows;
    else if (key == "n_sets") ls >> in.n_sets;
    else if (key == "n_bins") ls >> n_bins;
    else if (key == "draws") ls >> draws;
    else if (key == "have_n_ge") ls >> have_n_ge;
    else if (key == "want_null") ls >> want_null;
    else if (key == "want_picks") ls >> want_picks;
    else if (key == "max_mb") ls >> max_mb;
    else if (key == "seed") ls >> seed;
    else if (key == "attempts") ls >> attempts;
    else if (key == "set_off") { for (int64_t v; ls >> v;) set_off.push_back(v); }
    else if (key == "members") { for (int32_t v; ls >> v;) members.push_back(v); }
    else if (key == "bin") { have_bin = true; for (int32_t v; ls >> v;) bin.push_back(v); }
    else if (key == "pick") { int64_t s, b; ls >> s >> b; pick.push_back({s, b}); }
    else if (key == "mix") { uint64_t z; ls >> z; mix.push_back(z); }
    else return 2;
  }
  if (in.n_sets < 0 || set_off.size() != (size_t)in.n_sets + 1 || members.size() != (size_t)set_off.back()) return 2;
  if (have_bin && bin.size() != (size_t)in.n_rows) return 2;
  // heap arrays of exactly their size, never NULL where the list is present
  std::unique_ptr<int64_t[]> p_off(new int64_t[set_off.size()]);
  std::unique_ptr<int32_t[]> p_mem(new int32_t[members.size()]), p_bin(have_bin ? new int32_t[bin.size()] : nullptr);
  std::copy(set_off.begin(), set_off.end(), p_off.get());
  std::copy(members.begin(), members.end(), p_mem.get());
  if (have_bin) std::copy(bin.begin(), bin.end(), p_bin.get());
  in.set_off = p_off.get();
  in.members = p_mem.get();
  in.n_cols = 1;

  std::string msg;
  const int rc = gcre_compete::check_compete_args(&in, p_bin.get(), n_bins, draws, have_n_ge != 0, want_null != 0, want_picks != 0,
                                                  max_mb, "score_sets_compete", msg);
  std::printf("check %d %s\n", rc, msg.c_str());
  if (rc == GCRE_OK && !pick.empty()) {
    std::vector<int32_t> prow, poff;
    gcre_compete::compete_pool(p_bin.get(), in.n_rows, n_bins, prow, poff);
    std::vector<gcre_compete::CompeteMember> mem;
    gcre_compete::compete_members(&in, p_bin.get(), poff, mem);
    std::unique_ptr<int32_t[]> p_pool(new int32_t[prow.size()]);
    std::copy(prow.begin(), prow.end(), p_pool.get());
    for (const auto& sb : pick) {
      const int64_t s = sb.first;
      if (s < 0 || s >= in.n_sets) return 2;
      const int32_t k = (int32_t)(set_off[(size_t)s + 1] - set_off[(size_t)s]);
      std::unique_ptr<int32_t[]> out(new int32_t[(size_t)k]);
      std::unique_ptr<gcre_compete::CompeteMember[]> m(new gcre_compete::CompeteMember[(size_t)k]);
      std::copy(mem.begin() + set_off[(size_t)s], mem.begin() + set_off[(size_t)s + 1], m.get());
      gcre_compete::compete_draw(seed, s, sb.second, m.get(), k, p_pool.get(), attempts, out.get());
      std::printf("picks %lld %lld", (long long)s, (long long)sb.second);
      for (int32_t j = 0; j < k; j++) std::printf(" %d", out[(size_t)j]);
      std::printf("\n");
    }
  }
  for (uint64_t z : mix) std::printf("mix %llu %llu\n", (unsigned long long)z, (unsigned long long)gcre_compete::compete_mix64(z));
  return 0;
}

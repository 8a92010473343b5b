// dose_main.cpp -- drives the host plan of gcre_score_sets_dose (csrc/gcre_dose.h, with the slabs and the block table of
// csrc/gcre_prefix.h) on one case read from a file, for tests/test_dose_host.py.  Plain C++: no GPU, no HIP.  The case file is
// a list of "key values..." lines:
//   n_sets S | set_off ... | members ...                the set list
//   levels ...                                          the levels; without a `levels` line the pointer is NULL
//   n_levels N                                          what the call says their number is (default: as many as listed)
//   have_out 0/1 | iterations K | method M | w32p D | kpad P | want_null 0/1 | max_mb F | slab_sets N
// Output: "check CODE MESSAGE" first; then, if the check passed, "packed HEX" (the levels as the kernel takes them) and one
// "slab v0 nv rows" line per slab, each followed by "order ..." and "waves slot rows row0 ...".  Every array has exactly the
// size the case gives it, so that a sanitizer sees any access beyond it.
#include "../../geneticscre_amd/csrc/gcre_dose.h"

#include <cstdio>
#include <fstream>
#include <memory>
#include <sstream>

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line, key;
  gcre_set_input in{};
  int have_out = 1, iterations = 1, method = 1, w32p = 8, kpad = 2048, want_null = 0;
  long long n_levels = 0;
  bool have_n = false;
  double max_mb = 1024;
  int64_t slab_sets = 0;
  bool have_levels = false;
  std::vector<int64_t> set_off;
  std::vector<int32_t> members, levels;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "n_sets") ls >> in.n_sets;
    else if (key == "have_out") ls >> have_out;
    else if (key == "n_levels") { have_n = true; ls >> n_levels; }
    else if (key == "iterations") ls >> iterations;
    else if (key == "method") ls >> method;
    else if (key == "w32p") ls >> w32p;
    else if (key == "kpad") ls >> kpad;
    else if (key == "want_null") ls >> want_null;
    else if (key == "max_mb") ls >> max_mb;
    else if (key == "slab_sets") ls >> slab_sets;
    else if (key == "set_off") { for (int64_t v; ls >> v;) set_off.push_back(v); }
    else if (key == "members") { for (int32_t v; ls >> v;) members.push_back(v); }
    else if (key == "levels") { have_levels = true; for (int32_t v; ls >> v;) levels.push_back(v); }
    else return 2;
  }
  if (in.n_sets < 0 || set_off.size() != (size_t)in.n_sets + 1 || members.size() != (size_t)set_off.back()) return 2;
  if (!have_n) n_levels = (long long)levels.size();
  // the check reads levels[0 .. n_levels) only when n_levels is 1 .. 15: a case may say more levels than it lists only beyond that
  if (have_levels && n_levels >= 1 && n_levels <= gcre_dose::kDoseMaxLevel && (size_t)n_levels > levels.size()) return 2;
  // heap arrays of exactly their size
  std::unique_ptr<int64_t[]> p_off(new int64_t[set_off.size()]);
  std::unique_ptr<int32_t[]> p_mem(new int32_t[members.size()]);
  std::unique_ptr<int32_t[]> p_lev(have_levels ? new int32_t[levels.size()] : nullptr);
  std::copy(set_off.begin(), set_off.end(), p_off.get());
  std::copy(members.begin(), members.end(), p_mem.get());
  if (have_levels) std::copy(levels.begin(), levels.end(), p_lev.get());
  in.set_off = p_off.get();
  in.members = p_mem.get();
  in.n_cols = 1;

  std::string msg;
  const int rc = gcre_dose::check_dose_args(&in, p_lev.get(), (int32_t)n_levels, have_out != 0, iterations, method, w32p, kpad,
                                            want_null != 0, max_mb, "score_sets_dose", msg);
  std::printf("check %d %s\n", rc, msg.c_str());
  if (rc != GCRE_OK) return 0;
  std::printf("packed %llx\n", (unsigned long long)gcre_dose::pack_levels(p_lev.get(), (int32_t)n_levels));
  std::vector<int64_t> vsteps;
  for (int64_t s = 0; s < in.n_sets; s++)
    if (gcre_prefix::prefix_set_valid(&in, s)) vsteps.push_back(n_levels);
  std::vector<gcre_prefix::PrefixSlab> slabs;
  gcre_prefix::prefix_slabs(vsteps, method, w32p, kpad, want_null != 0, max_mb, slab_sets, slabs);
  for (const auto& sl : slabs) {
    std::printf("slab %lld %lld %lld\n", (long long)sl.v0, (long long)sl.nv, (long long)sl.steps);
    std::unique_ptr<int64_t[]> vs(new int64_t[(size_t)sl.nv]);   // exactly the slab's
    std::copy(vsteps.begin() + sl.v0, vsteps.begin() + sl.v0 + sl.nv, vs.get());
    std::vector<int32_t> order;
    std::vector<gcre_prefix::PrefixWave> waves;
    gcre_prefix::prefix_blocks(vs.get(), sl.nv, order, waves);
    std::printf("order");
    for (int32_t v : order) std::printf(" %d", v);
    std::printf("\nwaves");
    for (const auto& w : waves) std::printf(" %d %d %lld", w.slot, w.steps, (long long)w.row0);
    std::printf("\n");
  }
  return 0;
}

// seq_prefix_main.cpp -- drives the host plan of gcre_score_sets_prefix_sequential and gcre_score_sets_dose_sequential
// (csrc/gcre_seq_prefix.h) on one case read from a file, for tests/test_seq_prefix_host.py.  Plain C++: no GPU, no HIP.  The
// case file is a list of "key values..." lines:
//   n_sets S | set_off ... | members ...                the set list
//   cut ...                                             the cut flags; without a `cut` line the list is NULL (every member)
//   levels ...                                          the dose entry: its levels (then `cut` is not read)
//   have_out 0/1 | have_seq 0/1 | method M | w32p D | max_mb F | slab_sets N | hits H | max_perms P | weighted 0/1
//   nan ...                                             per valid set, in input order: 1 = its best observed score is NaN
//   loop LEFT_OVER STRATUM ACTIVE BATCHES               per slab, in order: what its batch loop left (LEFT_OVER -1: no R)
// Output: "check CODE MESSAGE" first; then, if the check passed, one "slab v0 nv steps" line per slab, each followed by
// "active ..." (its first active list, slots of the slab) and "launches N"; last "total REFUSED LEFT_OVER STRATUM ACTIVE".
// Every array has exactly the size the case gives it, so that a sanitizer sees any access beyond it.
#include "../../geneticscre_amd/csrc/gcre_seq_prefix.h"

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
  int have_out = 1, have_seq = 1, method = 1, w32p = 8, weighted = 0;
  double max_mb = 1024;
  int64_t slab_sets = 0, hits = 20, max_perms = 1000;
  bool have_cut = false, dose = false;
  std::vector<int64_t> set_off;
  std::vector<int32_t> members, levels;
  std::vector<int> cut, nan;
  struct Loop { int64_t left_over; int stratum; int64_t active, batches; };
  std::vector<Loop> loops;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "n_sets") ls >> in.n_sets;
    else if (key == "have_out") ls >> have_out;
    else if (key == "have_seq") ls >> have_seq;
    else if (key == "method") ls >> method;
    else if (key == "w32p") ls >> w32p;
    else if (key == "max_mb") ls >> max_mb;
    else if (key == "slab_sets") ls >> slab_sets;
    else if (key == "hits") ls >> hits;
    else if (key == "max_perms") ls >> max_perms;
    else if (key == "weighted") ls >> weighted;
    else if (key == "set_off") { for (int64_t v; ls >> v;) set_off.push_back(v); }
    else if (key == "members") { for (int32_t v; ls >> v;) members.push_back(v); }
    else if (key == "cut") { have_cut = true; for (int v; ls >> v;) cut.push_back(v); }
    else if (key == "levels") { dose = true; for (int32_t v; ls >> v;) levels.push_back(v); }
    else if (key == "nan") { for (int v; ls >> v;) nan.push_back(v); }
    else if (key == "loop") { Loop l{}; ls >> l.left_over >> l.stratum >> l.active >> l.batches; loops.push_back(l); }
    else return 2;
  }
  if (in.n_sets < 0 || set_off.size() != (size_t)in.n_sets + 1 || members.size() != (size_t)set_off.back()) return 2;
  if (have_cut && cut.size() != members.size()) return 2;
  // heap arrays of exactly their size
  std::unique_ptr<int64_t[]> p_off(new int64_t[set_off.size()]);
  std::unique_ptr<int32_t[]> p_mem(new int32_t[members.size()]);
  std::unique_ptr<uint8_t[]> p_cut(have_cut ? new uint8_t[cut.size()] : nullptr);
  std::unique_ptr<int32_t[]> p_lev(dose ? new int32_t[levels.size()] : nullptr);
  std::copy(set_off.begin(), set_off.end(), p_off.get());
  std::copy(members.begin(), members.end(), p_mem.get());
  for (size_t i = 0; have_cut && i < cut.size(); i++) p_cut[i] = (uint8_t)cut[i];
  for (size_t i = 0; dose && i < levels.size(); i++) p_lev[i] = levels[i];
  in.set_off = p_off.get();
  in.members = p_mem.get();
  in.n_cols = 1;

  gcre_prefix::PrefixSteps st;
  std::string msg;
  int rc;
  if (dose) {
    rc = gcre_seq_prefix::check_seq_dose_args(&in, p_lev.get(), (int32_t)levels.size(), have_out != 0, have_seq != 0, method, w32p, max_mb,
                                              hits, max_perms, "score_sets_dose_sequential", msg);
  } else {
    gcre_prefix::prefix_steps(&in, p_cut.get(), st);
    rc = gcre_seq_prefix::check_seq_prefix_args(&in, st, have_out != 0, have_seq != 0, method, w32p, max_mb, hits, max_perms,
                                                "score_sets_prefix_sequential", msg);
  }
  std::printf("check %d %s\n", rc, msg.c_str());
  if (rc != GCRE_OK) return 0;
  std::vector<int64_t> vsteps;
  for (int64_t s = 0; s < in.n_sets; s++)
    if (gcre_prefix::prefix_set_valid(&in, s)) vsteps.push_back(dose ? (int64_t)levels.size() : st.off[(size_t)s + 1] - st.off[(size_t)s]);
  if (nan.size() != vsteps.size()) return 2;
  std::vector<gcre_prefix::PrefixSlab> slabs;
  gcre_prefix::prefix_slabs(vsteps, method, w32p, 0, false, max_mb, slab_sets, slabs);
  if (!loops.empty() && loops.size() != slabs.size()) return 2;
  gcre_seq_prefix::SeqPrefixTotals totals;
  size_t at = 0;
  for (const auto& sl : slabs) {
    std::printf("slab %lld %lld %lld\n", (long long)sl.v0, (long long)sl.nv, (long long)sl.steps);
    std::unique_ptr<int64_t[]> vs(new int64_t[(size_t)sl.nv]);   // exactly the slab's
    std::unique_ptr<uint8_t[]> sn(new uint8_t[(size_t)sl.nv]);
    std::copy(vsteps.begin() + sl.v0, vsteps.begin() + sl.v0 + sl.nv, vs.get());
    for (int64_t e = 0; e < sl.nv; e++) sn[(size_t)e] = (uint8_t)nan[(size_t)(sl.v0 + e)];
    std::vector<uint32_t> act;
    gcre_seq_prefix::first_active(vs.get(), sl.nv, sn.get(), weighted != 0, act);
    std::printf("active");
    for (uint32_t v : act) std::printf(" %u", v);
    std::printf("\n");
    if (!loops.empty()) {
      const Loop& l = loops[at++];
      totals.add(l.left_over, l.stratum, l.active);
      std::printf("launches %lld\n", (long long)gcre_seq_prefix::seq_prefix_slab_launches(l.batches, weighted != 0));
    }
  }
  std::printf("total %d %lld %d %lld\n", totals.refused() ? 1 : 0, (long long)totals.left_over, totals.left_stratum, (long long)totals.n_active);
  return 0;
}

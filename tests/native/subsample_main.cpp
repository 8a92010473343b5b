// subsample_main.cpp -- drives the draw rule, the argument checks and the slab sizing of gcre_score_sets_subsample
// (csrc/gcre_subsample.h) on one case read from a file, for tests/test_subsample_host.py.  Plain C++: no GPU, no HIP.  The
// case file is a list of "key values..." lines:
//   n_cases C | n_ctrls T | m_cases A | m_ctrls B | draws D | seed X | n_sets S
//   table_a 0/1 NROW NCOL | table_b 0/1 NROW NCOL       whether the table is given, and its shape
//   n_cut J | cut ...                                   S x J values ("nan" is read); without a `cut` line the array is NULL
//   have_n_a 0/1 | have_n_b 0/1 | have_n_both 0/1 | want_a 0/1 | want_b 0/1 | max_mb F     what the check is told
//   mask B                                              print draw B as a string of 0 / 1 (any number of `mask` lines)
//   slab DRAWS W32P PER_DRAW_BYTES MAX_MB               print subsample_slab_draws of these (any number)
//   mix Z                                               print subsample_mix64(Z) (any number)
// Output: "check CODE MESSAGE" first; then, if the check passed, one "mask B bits" line per `mask` line; "slab N" and
// "mix Z V" lines last.  Every array has exactly the size the case gives it, so that a sanitizer sees any access beyond it.
#include "../../geneticscre_amd/csrc/gcre_subsample.h"

#include <cmath>
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
  gcre_subsample::SubsampleAsk q{};
  q.have_table_a = true;
  q.nrow_a = q.ncol_a = 1;
  q.have_n_a = true;
  double max_mb = 1024;
  uint64_t seed = 0;
  bool have_cut = false;
  std::vector<double> cut;
  std::vector<int64_t> mask;
  std::vector<uint64_t> mix;
  struct Slab { int64_t draws; int32_t w; double per, mb; };
  std::vector<Slab> slabs;
  auto flag = [](std::istringstream& ls) { int v = 0; ls >> v; return v != 0; };
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "n_cases") ls >> q.n_cases;
    else if (key == "n_ctrls") ls >> q.n_ctrls;
    else if (key == "m_cases") ls >> q.m_cases;
    else if (key == "m_ctrls") ls >> q.m_ctrls;
    else if (key == "draws") ls >> q.draws;
    else if (key == "seed") ls >> seed;
    else if (key == "n_sets") ls >> in.n_sets;
    else if (key == "table_a") { q.have_table_a = flag(ls); ls >> q.nrow_a >> q.ncol_a; }
    else if (key == "table_b") { q.have_table_b = flag(ls); ls >> q.nrow_b >> q.ncol_b; }
    else if (key == "n_cut") ls >> q.n_cut;
    else if (key == "cut") { have_cut = true; for (std::string v; ls >> v;) cut.push_back(v == "nan" ? std::nan("") : std::stod(v)); }
    else if (key == "have_n_a") q.have_n_a = flag(ls);
    else if (key == "have_n_b") q.have_n_b = flag(ls);
    else if (key == "have_n_both") q.have_n_both = flag(ls);
    else if (key == "want_a") q.want_scores_a = flag(ls);
    else if (key == "want_b") q.want_scores_b = flag(ls);
    else if (key == "max_mb") ls >> max_mb;
    else if (key == "mask") { int64_t b; ls >> b; mask.push_back(b); }
    else if (key == "slab") { Slab s{}; ls >> s.draws >> s.w >> s.per >> s.mb; slabs.push_back(s); }
    else if (key == "mix") { uint64_t z; ls >> z; mix.push_back(z); }
    else return 2;
  }
  if (in.n_sets < 0) return 2;
  if (have_cut && q.n_cut >= 0 && cut.size() != (size_t)in.n_sets * (size_t)q.n_cut) return 2;
  // a heap array of exactly its size, never NULL where the list is present
  std::unique_ptr<double[]> p_cut(have_cut ? new double[cut.size()] : nullptr);
  if (have_cut) std::copy(cut.begin(), cut.end(), p_cut.get());
  q.cut = p_cut.get();

  std::string msg;
  const int rc = gcre_subsample::check_subsample_args(&in, q, max_mb, "score_sets_subsample", msg);
  std::printf("check %d %s\n", rc, msg.c_str());
  if (rc == GCRE_OK && !mask.empty()) {
    const int32_t n = q.n_cases + q.n_ctrls;
    const size_t words = (size_t)(n + 31) / 32;
    std::unique_ptr<uint32_t[]> w(new uint32_t[words]);
    for (int64_t b : mask) {
      gcre_subsample::subsample_draw(seed, b, q.n_cases, q.n_ctrls, q.m_cases, q.m_ctrls, w.get());
      std::string bits((size_t)n, '0');
      for (int32_t c = 0; c < n; c++)
        if ((w[(size_t)c >> 5] >> (c & 31)) & 1u) bits[(size_t)c] = '1';
      std::printf("mask %lld %s\n", (long long)b, bits.c_str());
    }
  }
  for (const Slab& s : slabs) std::printf("slab %lld\n", (long long)gcre_subsample::subsample_slab_draws(s.draws, s.w, s.per, s.mb));
  for (uint64_t z : mix) std::printf("mix %llu %llu\n", (unsigned long long)z, (unsigned long long)gcre_subsample::subsample_mix64(z));
  return 0;
}

// sequential_main.cpp -- drives the mask rule, the bit-row search, the argument checks and the batch schedule of
// gcre_score_sets_sequential (csrc/gcre_sequential.h) on one case read from a file, for tests/test_sequential_host.py.  Plain
// C++: no GPU, no HIP.  The case file is a list of "key values..." lines:
//   n_cases C | n_ctrls T | seed X
//   n_strata N | strata s0 s1 ...                      what the caller passes; without a `strata` line the array is NULL
//   hits H | max_perms P | have_seq_out 0/1            what the check is told
//   mask R                                             print permutation R as a string of 0 / 1 (any number of `mask` lines)
//   find PRIOR H NBITS w0 w1 ...                       print sequential_find of the bit row w (hexadecimal words)
//   batch PREV DWORDS NACTIVE MAX_MB CAP               print sequential_batch of these
//   schedule DWORDS NACTIVE MAX_MB CAP MAX_PERMS       print the batches of a call whose active list never shrinks
//   mix Z                                              print seq_mix64(Z)
// Output: "check CODE MESSAGE" first (the argument check, then the strata); then, if it passed, one "mask R bits" line per
// `mask` line; "find I", "batch N", "schedule n1 n2 ..." and "mix Z V" lines last.  Every array has exactly the size the case
// gives it, so that a sanitizer sees any access beyond it.
#include "../../geneticscre_amd/csrc/gcre_sequential.h"

#include <cstdio>
#include <fstream>
#include <memory>
#include <sstream>

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line, key;
  int32_t n_cases = 1, n_ctrls = 1;
  int n_strata = 0;
  uint64_t seed = 0;
  int64_t hits = 1, max_perms = 0;
  bool have_seq_out = true, have_strata = false;
  std::vector<int32_t> strata;
  std::vector<uint64_t> mask, mix;
  struct Find { int64_t prior, h, n_bits; std::vector<uint64_t> w; };
  std::vector<Find> finds;
  struct Batch { int64_t prev; int32_t dwords; int64_t nactive; double mb; int64_t cap, max_perms; bool schedule; };
  std::vector<Batch> batches;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "n_cases") ls >> n_cases;
    else if (key == "n_ctrls") ls >> n_ctrls;
    else if (key == "seed") ls >> seed;
    else if (key == "n_strata") ls >> n_strata;
    else if (key == "strata") { have_strata = true; for (int32_t v; ls >> v;) strata.push_back(v); }
    else if (key == "hits") ls >> hits;
    else if (key == "max_perms") ls >> max_perms;
    else if (key == "have_seq_out") { int v = 0; ls >> v; have_seq_out = v != 0; }
    else if (key == "mask") { uint64_t r; ls >> r; mask.push_back(r); }
    else if (key == "find") {
      Find q{};
      ls >> q.prior >> q.h >> q.n_bits;
      for (std::string v; ls >> v;) q.w.push_back(std::stoull(v, nullptr, 16));
      if ((int64_t)q.w.size() != (q.n_bits + 63) / 64) return 2;
      finds.push_back(q);
    }
    else if (key == "batch") { Batch b{}; ls >> b.prev >> b.dwords >> b.nactive >> b.mb >> b.cap; batches.push_back(b); }
    else if (key == "schedule") { Batch b{}; b.schedule = true; ls >> b.dwords >> b.nactive >> b.mb >> b.cap >> b.max_perms; batches.push_back(b); }
    else if (key == "mix") { uint64_t z; ls >> z; mix.push_back(z); }
    else return 2;
  }
  const int32_t n = n_cases + n_ctrls;
  if (have_strata && (int32_t)strata.size() != n) return 2;
  // a heap array of exactly its size, never NULL where the list is present
  std::unique_ptr<int32_t[]> p_strata(have_strata ? new int32_t[strata.size()] : nullptr);
  if (have_strata) std::copy(strata.begin(), strata.end(), p_strata.get());

  const std::string who = "score_sets_sequential";
  std::string msg;
  std::vector<uint32_t> cases_in, size_of;
  int rc = gcre_sequential::check_sequential_args(hits, max_perms, have_seq_out, who, msg);
  if (rc == GCRE_OK) rc = gcre_sequential::strata_counts(n, n_cases, p_strata.get(), n_strata, cases_in, size_of, who, msg);
  std::printf("check %d %s\n", rc, msg.c_str());
  if (rc == GCRE_OK && !mask.empty()) {
    const size_t words = (size_t)(n + 31) / 32;
    std::unique_ptr<uint32_t[]> w(new uint32_t[words]);
    for (uint64_t r : mask) {
      gcre_sequential::sequential_mask(seed, r, n, p_strata.get(), cases_in, size_of, w.get());
      std::string bits((size_t)n, '0');
      for (int32_t c = 0; c < n; c++)
        if ((w[(size_t)c >> 5] >> (c & 31)) & 1u) bits[(size_t)c] = '1';
      std::printf("mask %llu %s\n", (unsigned long long)r, bits.c_str());
    }
  }
  for (const Find& q : finds) {
    std::unique_ptr<uint64_t[]> w(new uint64_t[q.w.size()]);
    std::copy(q.w.begin(), q.w.end(), w.get());
    std::printf("find %lld\n", (long long)gcre_sequential::sequential_find(w.get(), q.n_bits, q.prior, q.h));
  }
  for (const Batch& b : batches) {
    if (!b.schedule) {
      std::printf("batch %lld\n", (long long)gcre_sequential::sequential_batch(b.prev, b.dwords, b.nactive, b.mb, b.cap));
      continue;
    }
    // the host loop of the entry: r0 moves on by the batch every turn
    std::string out = "schedule";
    int64_t r0 = 0, batch = 0;
    for (int turns = 0; r0 < b.max_perms; turns++) {
      batch = gcre_sequential::sequential_batch(batch, b.dwords, b.nactive, b.mb, b.cap);
      if (batch <= 0 || batch % gcre_sequential::kSeqTile != 0 || turns > 1000000) return 3;
      const int64_t nb = std::min(batch, b.max_perms - r0);
      out += " " + std::to_string(nb);
      r0 += nb;
    }
    std::printf("%s\n", out.c_str());
  }
  for (uint64_t z : mix) std::printf("mix %llu %llu\n", (unsigned long long)z, (unsigned long long)gcre_sequential::seq_mix64(z));
  return 0;
}

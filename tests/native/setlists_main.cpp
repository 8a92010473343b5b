// setlists_main.cpp -- drives the set-list host stage of the library (csrc/gcre_setlists.h) on one case read from a file,
// for tests/test_setlists_host.py.  Plain C++: no GPU, no HIP.  The case file is a list of "key values..." lines:
//   method M | n N | n_cases C | stride WORDS | split 0/1 | who NAME       the context's side
//   n_cols N | n_rows R | n_sets S                                          what the caller declares (may be wrong)
//   rows HEX... | set_off ... | members ... | signs ...                     the arrays; a key that is absent is a NULL array
// Output: "check CODE MESSAGE", and if the checks pass, per set "set S valid V k K0 K1 K2 K3", "P HEX..." and (method 2)
// "N HEX...": the set's row of the destination, method x stride words, the (-) half at offset stride.  Every array has exactly
// the size the case gives it, so that a sanitizer sees any access beyond it.
#include "../../geneticscre_amd/csrc/gcre_setlists.h"

#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <sstream>

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  int method = 1, n = 0, n_cases = 0, split = 0;
  size_t stride = 0;
  std::string who = "score_sets", line, key;
  gcre_set_input in{};
  std::vector<uint64_t> rows;
  std::vector<int64_t> set_off;
  std::vector<int32_t> members, signs;
  bool have_rows = false, have_off = false, have_members = false, have_signs = false;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "method") ls >> method;
    else if (key == "n") ls >> n;
    else if (key == "n_cases") ls >> n_cases;
    else if (key == "stride") ls >> stride;
    else if (key == "split") ls >> split;
    else if (key == "who") ls >> who;
    else if (key == "n_cols") ls >> in.n_cols;
    else if (key == "n_rows") ls >> in.n_rows;
    else if (key == "n_sets") ls >> in.n_sets;
    else if (key == "rows") { have_rows = true; for (std::string h; ls >> h;) rows.push_back(std::stoull(h, nullptr, 16)); }
    else if (key == "set_off") { have_off = true; for (int64_t v; ls >> v;) set_off.push_back(v); }
    else if (key == "members") { have_members = true; for (int32_t v; ls >> v;) members.push_back(v); }
    else if (key == "signs") { have_signs = true; for (int32_t v; ls >> v;) signs.push_back(v); }
    else return 2;
  }
  const int W = (n + 63) / 64;
  if (n < 1 || n_cases < 0 || n_cases > n || stride < (size_t)W || (method != 1 && method != 2) || (split && method != 2))
    return 2;
  in.rows = have_rows ? rows.data() : nullptr;
  in.set_off = have_off ? set_off.data() : nullptr;
  in.members = have_members ? members.data() : nullptr;
  in.signs = have_signs ? signs.data() : nullptr;

  std::string msg;
  int rc = gcre_host::check_set_shape(&in, n, who, msg);
  if (rc == GCRE_OK) rc = gcre_host::check_set_members(&in, who, msg);
  std::printf("check %d %s\n", rc, msg.c_str());
  if (rc != GCRE_OK) return 0;

  const size_t RW = (size_t)method * stride;
  const gcre_host::SetUnion un(W, n, n_cases);
  std::vector<uint64_t> dst((size_t)in.n_sets * RW, 0);
  for (int64_t s = 0; s < in.n_sets; s++) {
    uint64_t* P = dst.data() + (size_t)s * RW;
    const bool valid = gcre_host::set_is_valid(&in, s);
    int32_t k[4] = {0, 0, 0, 0};
    if (valid) un.build(&in, s, P, stride, split != 0, k);
    std::printf("set %" PRId64 " valid %d k %d %d %d %d\n", s, valid ? 1 : 0, k[0], k[1], k[2], k[3]);
    for (int h = 0; h < method; h++) {
      std::printf(h ? "N" : "P");
      for (size_t w = 0; w < stride; w++) std::printf(" %" PRIx64, P[(size_t)h * stride + w]);
      std::printf("\n");
    }
  }
  return 0;
}

// given_main.cpp -- drives the index check of gcre_score_sets_given (check_given_index, csrc/gcre_setlists.h) on one case
// read from a file, for tests/test_given_host.py.  Plain C++: no GPU, no HIP.  The case file is a list of "key values..."
// lines:
//   n_rows R | n_sets S | set_off ... | members ...     the set list (the checks of the list itself are setlists_main's)
//   n_which E | cap C                                   what the caller declares (may be wrong)
//   which ... | given ...                               the index lists; a key that is absent is a NULL list
// Output: "check CODE MESSAGE".  Every array has exactly the size the case gives it, so that a sanitizer sees any access
// beyond it.
#include "../../geneticscre_amd/csrc/gcre_setlists.h"

#include <cstdio>
#include <algorithm>
#include <fstream>
#include <memory>
#include <sstream>

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line, key;
  gcre_set_input in{};
  int64_t n_which = 0, cap = 0;
  std::vector<int64_t> set_off, which, given;
  std::vector<int32_t> members;
  bool have_which = false, have_given = false;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "n_rows") ls >> in.n_rows;
    else if (key == "n_sets") ls >> in.n_sets;
    else if (key == "n_which") ls >> n_which;
    else if (key == "cap") ls >> cap;
    else if (key == "set_off") { for (int64_t v; ls >> v;) set_off.push_back(v); }
    else if (key == "members") { for (int32_t v; ls >> v;) members.push_back(v); }
    else if (key == "which") { have_which = true; for (int64_t v; ls >> v;) which.push_back(v); }
    else if (key == "given") { have_given = true; for (int64_t v; ls >> v;) given.push_back(v); }
    else return 2;
  }
  if (in.n_sets < 0 || set_off.size() != (size_t)in.n_sets + 1 || members.size() != (size_t)set_off.back()) return 2;
  // the lists are as long as the caller SAYS only where that is what the check relies on: a negative or mismatched length
  // is refused before an element is read
  if (have_which && n_which >= 0 && which.size() != (size_t)n_which) return 2;
  if (have_given && n_which >= 0 && given.size() != (size_t)n_which) return 2;
  in.set_off = set_off.data();
  in.members = members.data();
  in.n_cols = 1;

  // a list that is present is never NULL, even when it is empty: a heap array of exactly its size
  auto exact = [](const std::vector<int64_t>& v) {
    std::unique_ptr<int64_t[]> p(new int64_t[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
  };
  const std::unique_ptr<int64_t[]> pw = have_which ? exact(which) : nullptr, pg = have_given ? exact(given) : nullptr;
  std::string msg;
  const int rc = gcre_host::check_given_index(&in, pw.get(), pg.get(), n_which, cap, "score_sets_given", msg);
  std::printf("check %d %s\n", rc, msg.c_str());
  return 0;
}

// patients_main.cpp -- drives the argument check of gcre_set_patient_counts (check_patient_index, csrc/gcre_setlists.h) on one
// case read from a file, for tests/test_patients_host.py.  Plain C++: no GPU, no HIP.  The case file is a list of
// "key values..." lines:
//   n_rows R | n_sets S | n_cols C | set_off ... | members ...   the set list (its own checks are setlists_main's)
//   n_which E | n_groups G | by_sign B | counts 0/1 | max_mb X    what the caller declares (may be wrong)
//   which ... | group ...                                        the lists; a key that is absent is a NULL list
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
  in.n_cols = 1;
  int64_t n_which = 0;
  int32_t n_groups = 1;
  int by_sign = 0, have_counts = 1;
  double max_mb = 1024;
  std::vector<int64_t> set_off, which;
  std::vector<int32_t> members, group;
  bool have_which = false, have_group = false;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "n_rows") ls >> in.n_rows;
    else if (key == "n_sets") ls >> in.n_sets;
    else if (key == "n_cols") ls >> in.n_cols;
    else if (key == "n_which") ls >> n_which;
    else if (key == "n_groups") ls >> n_groups;
    else if (key == "by_sign") ls >> by_sign;
    else if (key == "counts") ls >> have_counts;
    else if (key == "max_mb") ls >> max_mb;
    else if (key == "set_off") { for (int64_t v; ls >> v;) set_off.push_back(v); }
    else if (key == "members") { for (int32_t v; ls >> v;) members.push_back(v); }
    else if (key == "which") { have_which = true; for (int64_t v; ls >> v;) which.push_back(v); }
    else if (key == "group") { have_group = true; for (int32_t v; ls >> v;) group.push_back(v); }
    else return 2;
  }
  if (in.n_sets < 0 || set_off.size() != (size_t)in.n_sets + 1 || members.size() != (size_t)set_off.back()) return 2;
  // the lists are as long as the caller SAYS only where that is what the check relies on: a length it refuses (negative,
  // mismatched, too large) is refused before an element is read
  const bool reads = n_which >= 0 && n_which < 0x7fffffff - 16;
  if (have_which && reads && which.size() != (size_t)n_which) return 2;
  if (have_group && reads && group.size() != (size_t)n_which) return 2;
  in.set_off = set_off.data();
  in.members = members.data();

  // a list that is present is never NULL, even when it is empty: a heap array of exactly its size
  auto exact = [](const auto& v) {
    typedef typename std::decay<decltype(v)>::type::value_type T;
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
  };
  const std::unique_ptr<int64_t[]> pw = have_which ? exact(which) : nullptr;
  const std::unique_ptr<int32_t[]> pg = have_group ? exact(group) : nullptr;
  std::string msg;
  const int rc = gcre_host::check_patient_index(&in, pw.get(), n_which, pg.get(), n_groups, by_sign, have_counts != 0, max_mb,
                                                "set_patient_counts", msg);
  std::printf("check %d %s\n", rc, msg.c_str());
  return 0;
}

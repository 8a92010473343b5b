// clump_main.cpp -- drives what gcre_clump_sets refuses before it launches anything (csrc/gcre_clumporder.h) on one case
// read from a file, for tests/test_clump_host.py.  Plain C++: no GPU, no HIP.  The case file is a list of "key values..."
// lines:
//   n_sets S | set_off ... | members ...      the set list (it has passed the checks of gcre_setlists.h)
//   order ...                                 the walk order; absent = a NULL array
//   n_order N                                 its declared length (default: the entries given)
//   r X | measure M | patients P              the rule (r is read by strtod: "nan" is a NaN)
//   row_bytes B | max_mb X                    the size check; max_mb absent = GCRE_CLUMP_MAX_MB of the environment
// Output: "rule CODE MESSAGE", "order CODE MESSAGE", "bytes CODE MESSAGE MAX_MB".  Every array has exactly the size the case
// gives it, so that a sanitizer sees any access beyond it.
#include "../../geneticscre_amd/csrc/gcre_clumporder.h"

#include <cstdio>
#include <fstream>
#include <sstream>

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  gcre_set_input in{};
  std::vector<int64_t> set_off, order;
  std::vector<int32_t> members;
  bool have_order = false, have_n_order = false, have_max = false;
  int64_t n_order = 0, row_bytes = 128;
  double r = 0.5, max_mb = 0;
  int measure = 0, patients = 0;
  std::string line, key;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "n_sets") ls >> in.n_sets;
    else if (key == "set_off") { for (int64_t v; ls >> v;) set_off.push_back(v); }
    else if (key == "members") { for (int32_t v; ls >> v;) members.push_back(v); }
    else if (key == "order") { have_order = true; for (int64_t v; ls >> v;) order.push_back(v); }
    else if (key == "n_order") { have_n_order = true; ls >> n_order; }
    else if (key == "r") { std::string x; ls >> x; r = std::strtod(x.c_str(), nullptr); }
    else if (key == "measure") ls >> measure;
    else if (key == "patients") ls >> patients;
    else if (key == "row_bytes") ls >> row_bytes;
    else if (key == "max_mb") { have_max = true; ls >> max_mb; }
    else return 2;
  }
  if (in.n_sets < 0 || set_off.size() != (size_t)in.n_sets + 1 || (size_t)set_off.back() != members.size()) return 2;
  in.set_off = set_off.data();
  in.members = members.data();
  if (!have_n_order) n_order = (int64_t)order.size();
  if (have_order && n_order > (int64_t)order.size()) return 2;

  std::string msg;
  int rc = gcre_host::check_clump_rule(r, measure, patients, msg);
  std::printf("rule %d %s\n", rc, msg.c_str());
  msg.clear();
  rc = gcre_host::check_clump_order(&in, have_order ? order.data() : nullptr, n_order, msg);
  std::printf("order %d %s\n", rc, msg.c_str());
  msg.clear();
  if (!have_max) max_mb = gcre_host::clump_max_mb();
  rc = gcre_host::check_clump_bytes(n_order, row_bytes, max_mb, msg);
  std::printf("bytes %d %s %.6g\n", rc, msg.c_str(), max_mb);
  return 0;
}

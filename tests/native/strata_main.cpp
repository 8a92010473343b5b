// strata_main.cpp -- drives the host plan of gcre_score_sets_strata (csrc/gcre_strata.h) on one case read from a file, for
// tests/test_strata_host.py: the stratum counts, the argument checks, the table offsets and the slab sizing.  Plain C++: no
// GPU, no HIP.  The case file is a list of "key values..." lines:
//   n_cases C | n_ctrls T | iterations K | kpad KP | n_sets S
//   n_strata N | strata s0 s1 ...          what the caller passes; without a `strata` line the array is NULL
//   tables HAVE | nrow r0 r1 ... | ncol c0 c1 ... | tab_off o0 o1 ...   without a line the array is NULL
//   have_px 0/1 | want_null 0/1 | max_mb X (default: the environment's GCRE_STRATA_MAX_MB, or 1024)
//   slab V NS M W32P KPAD WANT_NULL MAX_MB   print strata_slab_sets of these (GCRE_STRATA_SLAB_SETS from the environment)
//   message BAD                              print the message of the refusal of masks that do not keep the strata
// Output: "check CODE MESSAGE" first; then, if it passed, "cases ...", "sizes ..." and "offsets ..." (n_strata + 1 entries);
// "slab N" and "message TEXT" lines last.  Every array has exactly the size the case gives it, so that a sanitizer sees any
// access beyond it.
#include "../../geneticscre_amd/csrc/gcre_strata.h"

#include <cstdio>
#include <fstream>
#include <memory>
#include <sstream>

template <typename T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v, bool have) {
  std::unique_ptr<T[]> p(have ? new T[v.size()] : nullptr);
  if (have) std::copy(v.begin(), v.end(), p.get());
  return p;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line, key;
  int32_t n_cases = 1, n_ctrls = 1, iterations = 0, kpad = 0, n_strata = 0;
  int64_t n_sets = 0;
  bool have_strata = false, have_tables = true, have_nrow = false, have_ncol = false, have_off = false, have_px = true, want_null = false;
  double max_mb = gcre_strata::strata_max_mb();
  std::vector<int32_t> strata, nrow, ncol;
  std::vector<int64_t> tab_off;
  struct Slab { int64_t v; int ns, m; int32_t w32p, kpad; int want; double mb; };
  std::vector<Slab> slabs;
  std::vector<long long> messages;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "n_cases") ls >> n_cases;
    else if (key == "n_ctrls") ls >> n_ctrls;
    else if (key == "iterations") ls >> iterations;
    else if (key == "kpad") ls >> kpad;
    else if (key == "n_sets") ls >> n_sets;
    else if (key == "n_strata") ls >> n_strata;
    else if (key == "strata") { have_strata = true; for (int32_t v; ls >> v;) strata.push_back(v); }
    else if (key == "tables") { int v = 0; ls >> v; have_tables = v != 0; }
    else if (key == "nrow") { have_nrow = true; for (int32_t v; ls >> v;) nrow.push_back(v); }
    else if (key == "ncol") { have_ncol = true; for (int32_t v; ls >> v;) ncol.push_back(v); }
    else if (key == "tab_off") { have_off = true; for (int64_t v; ls >> v;) tab_off.push_back(v); }
    else if (key == "have_px") { int v = 0; ls >> v; have_px = v != 0; }
    else if (key == "want_null") { int v = 0; ls >> v; want_null = v != 0; }
    else if (key == "max_mb") ls >> max_mb;
    else if (key == "slab") { Slab s{}; ls >> s.v >> s.ns >> s.m >> s.w32p >> s.kpad >> s.want >> s.mb; slabs.push_back(s); }
    else if (key == "message") { long long b = 0; ls >> b; messages.push_back(b); }
    else return 2;
  }
  const int32_t n = n_cases + n_ctrls;
  if (have_strata && (int32_t)strata.size() != n) return 2;
  // the per-stratum arrays hold n_strata entries where that is a count an array can have
  const size_t ns = n_strata > 0 ? (size_t)n_strata : 0;
  if ((have_nrow && nrow.size() != ns) || (have_ncol && ncol.size() != ns) || (have_off && tab_off.size() != ns)) return 2;
  const auto p_strata = exact(strata, have_strata);
  const auto p_nrow = exact(nrow, have_nrow);
  const auto p_ncol = exact(ncol, have_ncol);
  const auto p_off = exact(tab_off, have_off);

  gcre_set_input in{};
  in.n_sets = n_sets;
  const gcre_strata::StrataAsk q{n, n_cases, iterations, kpad, p_strata.get(), n_strata, have_tables, p_nrow.get(), p_ncol.get(),
                                 p_off.get(), have_px, want_null, false};
  std::string msg;
  std::vector<uint32_t> cases_in, size_of;
  const int rc = gcre_strata::check_strata_args(&in, q, max_mb, "score_sets_strata", cases_in, size_of, msg);
  std::printf("check %d %s\n", rc, msg.c_str());
  if (rc == GCRE_OK) {
    std::vector<int64_t> doff;
    gcre_strata::strata_diag_offsets(size_of, doff);
    std::string a = "cases", b = "sizes", c = "offsets";
    for (uint32_t v : cases_in) a += " " + std::to_string(v);
    for (uint32_t v : size_of) b += " " + std::to_string(v);
    for (int64_t v : doff) c += " " + std::to_string(v);
    std::printf("%s\n%s\n%s\n", a.c_str(), b.c_str(), c.c_str());
  }
  for (const Slab& s : slabs)
    std::printf("slab %lld\n", (long long)gcre_strata::strata_slab_sets(s.v, s.ns, s.m, s.w32p, s.kpad, s.want != 0, s.mb,
                                                                       gcre_strata::strata_slab_sets_env()));
  for (long long b : messages) std::printf("message %s\n", gcre_strata::strata_mask_message("score_sets_strata", b).c_str());
  return 0;
}

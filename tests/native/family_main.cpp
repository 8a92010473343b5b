// family_main.cpp -- drives the host plans of gcre_score_sets_family (csrc/gcre_family.h) and gcre_score_sets_minp
// (csrc/gcre_minp.h) on the cases of a file, for tests/test_family_host.py and tests/test_minp_host.py.  Plain C++: no GPU, no
// HIP.  The file is a list of "key values..." lines; array lines describe the next case, a command line runs and clears it:
//   n_sets S | vset ...          the records to write, and the set of every valid set (V values)
//   obs ...                      the V observed scores of the valid sets ("nan" is read)
//   ge ...                       their V counts among the permutations (min-P)
//   sd ... | hist ...            what the device leaves the family finish: V counts, max(m, 1) bins
//   le ... | q ...               what the device leaves the min-P finish: V counts, K minima
//   family                       print the walk of `obs`; with `sd`, finish it and print the S records
//   minp                         print the walk of `obs` and `ge`; with `le`, finish it and print the S records
//   family_slab V K TILE MAX_MB SLAB_PERMS | minp_slab V K TILE MAX_MB SLAB_SETS     print the slab or the refusal
//   env                          print the four bounds as the environment gives them
//   thr X                        print f32_threshold(X)
// Every array has exactly the size the case gives it, so that a sanitizer sees any access beyond it; records start as the
// stage leaves them before the device runs (valid 0 / 0 / 0, invalid -1 / 0 / -1 and -1 / -1).
#include "../../geneticscre_amd/csrc/gcre_family.h"
#include "../../geneticscre_amd/csrc/gcre_minp.h"

#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>

namespace {

template <typename T>
std::vector<T> exact(const std::vector<T>& v) { return std::vector<T>(v.begin(), v.end()); }   // capacity == size

template <typename T>
void print(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (const T& x : v) std::printf(" %lld", (long long)x);
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line, key;
  int64_t n_sets = 0;
  std::vector<int64_t> vset;
  std::vector<double> obs;
  std::vector<unsigned long long> ge, hist;
  std::vector<uint32_t> sd, le, q;
  bool have_sd = false, have_le = false;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "n_sets") ls >> n_sets;
    else if (key == "vset") { for (int64_t v; ls >> v;) vset.push_back(v); }
    else if (key == "obs") { for (std::string v; ls >> v;) obs.push_back(v == "nan" ? std::nan("") : std::stod(v)); }
    else if (key == "ge") { for (unsigned long long v; ls >> v;) ge.push_back(v); }
    else if (key == "hist") { for (unsigned long long v; ls >> v;) hist.push_back(v); }
    else if (key == "sd") { have_sd = true; for (uint32_t v; ls >> v;) sd.push_back(v); }
    else if (key == "le") { have_le = true; for (uint32_t v; ls >> v;) le.push_back(v); }
    else if (key == "q") { for (uint32_t v; ls >> v;) q.push_back(v); }
    else if (key == "family" || key == "minp") {
      const bool fam = key == "family";
      const int64_t V = (int64_t)obs.size();
      if (n_sets < 0 || (int64_t)vset.size() != V) return 2;
      for (int64_t s : vset)
        if (s < 0 || s >= n_sets) return 2;
      const std::vector<double> o = exact(obs);
      const std::vector<int64_t> vs = exact(vset);
      std::vector<char> valid((size_t)n_sets, 0);
      for (int64_t s : vs) valid[(size_t)s] = 1;
      if (fam) {
        gcre_family::FamilyWalk w;
        gcre_family::family_walk(o.data(), V, w);
        std::printf("family %d\n", w.m);
        print("order", w.order);
        print("rank", w.rank);
        print("meta", w.meta);
        print("gstart", w.gstart);
        print("bin", w.bin);
        print("pat", w.pat);
        if (have_sd) {
          if ((int64_t)sd.size() != V || (int)hist.size() != std::max(w.m, 1)) return 2;
          std::vector<uint32_t> s = exact(sd);
          std::vector<unsigned long long> h = exact(hist);
          std::vector<gcre_family_score> rec((size_t)n_sets);
          for (int64_t i = 0; i < n_sets; i++) rec[(size_t)i] = {valid[(size_t)i] ? 0 : -1, 0, valid[(size_t)i] ? 0 : -1};
          gcre_family::family_finish(w, vs.data(), s.data(), h.data(), rec.data());
          std::printf("records");
          for (const auto& r : rec) std::printf(" %lld %llu %lld", (long long)r.n_ge_stepdown, (unsigned long long)r.exceed, (long long)r.observed);
          std::printf("\n");
        }
      } else {
        if ((int64_t)ge.size() != V) return 2;
        const std::vector<unsigned long long> g = exact(ge);
        gcre_minp::MinpWalk w;
        gcre_minp::minp_walk(o.data(), g.data(), V, w);
        std::printf("minp\n");
        print("order", w.order);
        print("meta", w.meta);
        if (have_le) {
          if ((int64_t)le.size() != V) return 2;
          std::vector<uint32_t> l = exact(le), qq = exact(q);
          std::vector<gcre_minp_score> rec((size_t)n_sets);
          for (int64_t i = 0; i < n_sets; i++) rec[(size_t)i] = {valid[(size_t)i] ? 0 : -1, valid[(size_t)i] ? 0 : -1};
          gcre_minp::minp_finish(w, o.data(), g.data(), vs.data(), l.data(), qq, rec.data());
          std::printf("records");
          for (const auto& r : rec) std::printf(" %lld %lld", (long long)r.n_le_minp, (long long)r.n_le_stepdown);
          std::printf("\n");
        }
      }
      n_sets = 0;
      vset.clear(); obs.clear(); ge.clear(); hist.clear(); sd.clear(); le.clear(); q.clear();
      have_sd = have_le = false;
    } else if (key == "family_slab" || key == "minp_slab") {
      int64_t V = 0, bound = 0, slab = -1;
      int K = 0, tile = 0;
      double mb = 0;
      ls >> V >> K >> tile >> mb >> bound;
      std::string msg;
      const int rc = key == "family_slab" ? gcre_family::family_slab(V, K, tile, mb, bound, "score_sets_family", slab, msg)
                                          : gcre_minp::minp_slab(V, K, tile, mb, bound, "score_sets_minp", slab, msg);
      std::printf("%s %d %lld %s\n", key.c_str(), rc, (long long)slab, msg.c_str());
    } else if (key == "env") {
      std::printf("env %.17g %lld %.17g %lld\n", gcre_family::family_max_mb(), (long long)gcre_family::family_slab_perms(),
                  gcre_minp::minp_max_mb(), (long long)gcre_minp::minp_slab_sets());
    } else if (key == "thr") {
      std::string v;
      ls >> v;
      std::printf("thr %u\n", gcre_family::f32_threshold(v == "nan" ? std::nan("") : std::stod(v)));
    } else {
      return 2;
    }
  }
  return 0;
}

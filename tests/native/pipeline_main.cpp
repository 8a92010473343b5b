// pipeline_main.cpp -- drives the plain-C++ parts of the one-call pipeline (csrc/gcre_pipeline.h) on one case read from a
// file, for tests/test_pipeline_host.py.  Plain C++: no GPU, no HIP.  The case file is a list of "key values..." lines; the
// first names the case:
//   case merge    | top_k K | cand SCORE PATH SRC TRG CASES CTRLS ...   (one line per candidate, in the order handed over)
//   case hints    | method M | counts ... | locations ... | signs ... | data_inds ... | l2_signs ...
//   case set_rows | path_length L | data1_rows R | data2_rows R | level I counts...   (I = 0..3)
//   case window   | kall K | perms ...
//   case shard    | total T | world W
//   case tags     | levels N | k0 ... | rounds N
//   case hub      | mode reduce|tag|timeout|fail
// Output: one line per answer, described at each case.  Every array has exactly the size the case gives it, so that a
// sanitizer sees any access beyond it.
#include "../../geneticscre_amd/csrc/gcre_pipeline.h"

#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <thread>

using namespace gcre_host;

namespace {

std::map<std::string, std::vector<std::string>> g_one;                 // key -> values, for keys that come once
std::vector<std::vector<std::string>> g_cands;                         // the `cand` lines
std::map<int, std::vector<std::string>> g_levels;                      // the `level I` lines

bool has(const std::string& k) { return g_one.count(k) != 0; }
int64_t num(const std::string& k, size_t i = 0) { return std::stoll(g_one.at(k).at(i)); }

// a heap array of exactly the values of a key (never NULL, even when empty)
template <typename T>
std::unique_ptr<T[]> exact(const std::vector<std::string>& v) {
  std::unique_ptr<T[]> p(new T[v.size()]);
  for (size_t i = 0; i < v.size(); i++) p[i] = (T)std::stoll(v[i]);
  return p;
}

// "row SCORE SRC TRG CASES CTRLS" per row of the merged table
int run_merge() {
  std::vector<Candidate> cands;
  for (const auto& c : g_cands)
    cands.push_back(Candidate{std::stod(c.at(0)), std::stoll(c.at(1)), (int32_t)std::stol(c.at(2)), (int32_t)std::stol(c.at(3)),
                              (int32_t)std::stol(c.at(4)), (int32_t)std::stol(c.at(5))});
  gcre_result out{};
  merge_candidates(cands, (int)num("top_k"), &out);
  for (int32_t i = 0; i < out.n; i++)
    std::printf("row %.17g %d %d %d %d\n", out.scores[i], out.src[i], out.trg[i], out.cases[i], out.ctrls[i]);
  for (void* p : {(void*)out.scores, (void*)out.src, (void*)out.trg, (void*)out.cases, (void*)out.ctrls}) std::free(p);
  return 0;
}

// "added ..." (level 4's hint over data_inds and level 2's signs) and "second ..." (level 5's over the level), as hex
int run_hints() {
  const int method = (int)num("method");
  const auto& counts = g_one.at("counts");
  const auto cnt = exact<int32_t>(counts);
  const auto loc = exact<int64_t>(g_one.at("locations"));
  const auto sg = exact<int32_t>(g_one.at("signs"));
  const auto inds = exact<int32_t>(g_one.at("data_inds"));
  const auto sg2 = exact<int32_t>(g_one.at("l2_signs"));
  if (g_one.at("locations").size() != counts.size()) return 2;
  const gcre_level l3{cnt.get(), loc.get(), (int64_t)counts.size(), sg.get(), (int64_t)g_one.at("signs").size()};
  const gcre_level l2{nullptr, nullptr, 0, sg2.get(), (int64_t)g_one.at("l2_signs").size()};
  std::printf("added");
  for (int32_t v : added_rows_hint(method, inds.get(), (int64_t)g_one.at("data_inds").size(), l2)) std::printf(" %08x", (unsigned)v);
  std::printf("\nsecond");
  for (int32_t v : second_relation_hint(method, l3)) std::printf(" %08x", (unsigned)v);
  std::printf("\n");
  return 0;
}

// "set_rows ..."
int run_set_rows() {
  gcre_pp_input in{};
  in.path_length = (int)num("path_length");
  in.data1_rows = num("data1_rows");
  in.data2_rows = num("data2_rows");
  std::unique_ptr<int32_t[]> held[6];
  for (const auto& kv : g_levels) {
    if (kv.first < 0 || kv.first > 5) return 2;
    held[kv.first] = exact<int32_t>(kv.second);
    in.level[kv.first].uid_count = held[kv.first].get();
    in.level[kv.first].n_uids = (int64_t)kv.second.size();
  }
  std::printf("set_rows");
  for (int64_t r : set_rows(&in)) std::printf(" %" PRId64, r);
  std::printf("\n");
  return 0;
}

// "window ..." one rounded window per entry of perms
int run_window() {
  std::printf("window");
  for (size_t i = 0; i < g_one.at("perms").size(); i++) std::printf(" %d", round_window_perms((int)num("perms", i), (int)num("kall")));
  std::printf("\n");
  return 0;
}

// "shard BEGIN END" per rank
int run_shard() {
  for (int r = 0; r < (int)num("world"); r++) {
    int64_t b = -1, e = -1;
    shard_bounds(num("total"), r, (int)num("world"), &b, &e);
    std::printf("shard %" PRId64 " %" PRId64 "\n", b, e);
  }
  return 0;
}

// "tag LEVEL K0 ROUND HEX" for every combination
int run_tags() {
  for (int lv = 0; lv < (int)num("levels"); lv++)
    for (size_t k = 0; k < g_one.at("k0").size(); k++)
      for (int r = 0; r < (int)num("rounds"); r++)
        std::printf("tag %d %d %d %016" PRIx64 "\n", lv, (int)num("k0", k), r, hub_tag(lv, (int)num("k0", k), r));
  return 0;
}

// "tT round R rc RC values..." per thread and round, then "failed F timed_out T"
int run_hub() {
  const std::string mode = g_one.at("mode").at(0);
  ExchangeHub hub;
  hub.n = 3;
  std::vector<std::string> said(3);
  auto bring = [&](int t, int rounds, bool odd_tag) {
    for (int r = 0; r < rounds; r++) {
      // (the largest value of round r comes from thread 2 - r; MAX over the threads: 2 -0.5 2 | 4 1.5 2 | 6 3.5 0)
      std::vector<float> v = {(float)((t + r) % 3 * (r + 1)), (float)(t * r) - 0.5f, (float)((t + 1) * (r + 1) % 3)};
      const int rc = hub.reduce(v, hub_tag(2, 0, r) + (odd_tag && r == 0 ? 1 : 0));
      std::ostringstream o;
      o << "t" << t << " round " << r << " rc " << rc;
      if (rc == 0) for (float x : v) o << " " << x;
      said[(size_t)t] += o.str() + "\n";
    }
  };
  std::vector<std::thread> th;
  if (mode == "reduce") {
    for (int t = 0; t < 3; t++) th.emplace_back(bring, t, 3, false);
  } else if (mode == "tag") {
    for (int t = 0; t < 3; t++) th.emplace_back(bring, t, 1, t == 2);
  } else if (mode == "timeout") {
    hub.timeout_s = 0.05;
    for (int t = 0; t < 2; t++) th.emplace_back(bring, t, 1, false);
  } else if (mode == "fail") {
    for (int t = 0; t < 2; t++) th.emplace_back(bring, t, 1, false);
    for (bool both = false; !both; std::this_thread::yield()) {   // both wait for the third, which gives up instead
      std::lock_guard<std::mutex> lk(hub.m);
      both = hub.arrived == 2;
    }
    hub.fail();
  } else {
    return 2;
  }
  for (auto& t : th) t.join();
  for (const auto& s : said) std::fputs(s.c_str(), stdout);
  std::printf("failed %d timed_out %d\n", (int)hub.failed, (int)hub.timed_out);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line, key;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    std::vector<std::string> vals;
    for (std::string v; ls >> v;) vals.push_back(v);
    if (key == "cand") {
      g_cands.push_back(vals);
    } else if (key == "level") {
      if (vals.empty()) return 2;
      g_levels[std::stoi(vals[0])] = std::vector<std::string>(vals.begin() + 1, vals.end());
    } else {
      g_one[key] = vals;
    }
  }
  if (!has("case")) return 2;
  const std::string name = g_one.at("case").at(0);
  if (name == "merge") return run_merge();
  if (name == "hints") return run_hints();
  if (name == "set_rows") return run_set_rows();
  if (name == "window") return run_window();
  if (name == "shard") return run_shard();
  if (name == "tags") return run_tags();
  if (name == "hub") return run_hub();
  return 2;
}

// steps_main.cpp -- drives the plain C++ that the variable-threshold and multi-hit stages share (csrc/gcre_steps.h: the two row
// variants, the first rows of a slab) and the readers of the budgets (csrc/gcre_env.h) on a machine without a GPU, under the
// sanitizers.  tests/test_seq_prefix_host.py holds what it prints against values written down by hand.
//   steps_main records   three sets -- one with an NA member, one whose pick is NaN, one ordinary with cuts 0 1 0 1 -- through
//                        defaults and write of both variants
//   steps_main env       GCRE_TEST_MB (default 1024, cap 65536) and GCRE_TEST_COUNT as the environment gives them
#include "../../geneticscre_amd/csrc/gcre_steps.h"

#include <cstdio>

namespace {

struct Pick {   // PrefixPick of gcre_kernels.h
  double score;
  int32_t best_step;
  int32_t cnt[4];
  int32_t pad;
};

const int64_t kOff[4] = {0, 3, 6, 10};
const int32_t kMembers[10] = {3, -1, 5, 1, 2, 9, 4, 6, 7, 8};
const uint8_t kCut[10] = {1, 1, 1, 0, 0, 0, 0, 1, 0, 1};
const double kNan = std::numeric_limits<double>::quiet_NaN();

void print_check(const char* tag, int rc, const std::string& msg) { printf("%s %d %s\n", tag, rc, msg.c_str()); }

void print_scores(const char* tag, const std::vector<double>& x) {
  printf("%s", tag);
  for (double v : x) printf(" %g", v);
  printf("\n");
}

void print_rows(const char* tag, const std::vector<int64_t>& x) {
  printf("%s", tag);
  for (int64_t v : x) printf(" %lld", (long long)v);
  printf("\n");
}

template <typename Variant>
void slabs(const Variant& v) {
  const std::vector<int64_t> vset = {1, 2};   // the valid sets
  std::vector<int64_t> vsteps, row0;
  v.vsteps(vset, vsteps);
  print_rows("vsteps", vsteps);
  gcre_steps::slab_row0(vsteps, 0, 2, row0);
  print_rows("row0", row0);
  gcre_steps::slab_row0(vsteps, 1, 1, row0);
  print_rows("row0", row0);
}

int records() {
  gcre_set_input in{};
  in.n_sets = 3;
  in.set_off = kOff;
  in.members = kMembers;
  gcre_set_score out[3] = {};
  out[1].valid = out[2].valid = 1;
  const Pick nan_pick = {kNan, -1, {0, 0, 0, 0}, 0};
  const double nan_rows[2] = {kNan, kNan};
  std::string msg;

  {
    gcre_prefix_score rec[3];
    std::memset(rec, 0x5a, sizeof rec);
    std::vector<double> scores(10, 7.0);
    gcre_steps::PrefixRows v{kCut, rec, scores.data()};
    gcre_set_input big{};
    big.n_sets = (int64_t)1 << 31;
    print_check("check", v.check(&big, 1, 1, 8, 64, false, 1024.0, "who", msg), msg);
    print_check("check_seq", v.check_seq(&big, true, 1, 8, 1024.0, 20, 100, "who", msg), msg);
    msg.clear();
    print_check("check", v.check(&in, 1, 1, 8, 64, false, 1024.0, "who", msg), msg);
    auto print = [&](const char* tag) {
      for (const auto& x : rec)
        printf("%s %g %lld %d %d %d %d %d %d %d\n", tag, x.score, (long long)x.n_ge, x.best_step, x.best_members, x.steps, x.cases_pos,
               x.ctrls_pos, x.cases_neg, x.ctrls_neg);
      print_scores("step_scores", scores);
    };
    v.defaults(&in, out);
    print("px");
    const Pick p = {2.5, 1, {5, 6, 7, 8}, 0};
    const double rows[2] = {1.5, 2.5};
    v.write(1, nan_pick, nan_rows);
    v.write(2, p, rows);
    print("px");
    slabs(v);
    gcre_steps::PrefixRows bare{nullptr, rec, nullptr};   // no cuts: every member ends a step; no step scores: no rows read
    print_check("check_seq", bare.check_seq(&in, true, 1, 8, 1024.0, 20, 100, "who", msg), msg);
    bare.defaults(&in, out);
    bare.write(2, p, nullptr);
    printf("bare %d %d %d\n", rec[2].best_step, rec[2].best_members, rec[2].steps);
  }
  {
    const int32_t levels[2] = {1, 3};
    gcre_dose_score rec[3];
    std::memset(rec, 0x5a, sizeof rec);
    std::vector<double> scores(6, 7.0);
    const gcre_steps::DoseRows v{levels, 2, rec, scores.data()};
    auto print = [&](const char* tag) {
      for (const auto& x : rec)
        printf("%s %g %lld %d %d %d %d %d %d %d %d\n", tag, x.score, (long long)x.n_ge, x.best_index, x.best_level, x.levels, x.cases_pos,
               x.ctrls_pos, x.cases_neg, x.ctrls_neg, x.pad);
      print_scores("level_scores", scores);
    };
    v.defaults(&in, out);
    print("ds");
    const Pick p = {4.0, 1, {1, 2, 3, 4}, 0};
    const double rows[2] = {3.0, 4.0};
    v.write(1, nan_pick, nan_rows);
    v.write(2, p, rows);
    print("ds");
    slabs(v);
  }
  return 0;
}

int env() {
  printf("mb %.17g\ncount %lld\n", gcre_env::env_mb("GCRE_TEST_MB", 1024, 65536.0), (long long)gcre_env::env_count("GCRE_TEST_COUNT"));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string what = argc == 2 ? argv[1] : "";
  if (what == "records") return records();
  if (what == "env") return env();
  fprintf(stderr, "usage: steps_main records|env\n");
  return 2;
}

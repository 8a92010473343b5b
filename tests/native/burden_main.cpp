// burden_main.cpp -- drives the argument check of gcre_patient_burden (check_burden_args, csrc/gcre_setlists.h) on one case
// read from a file, for tests/test_burden_host.py.  Plain C++: no GPU, no HIP.  The case file is a list of
// "key values..." lines:
//   n_rows R | n_cols C | weights ...           what the caller passes; without a `weights` line the pointer is NULL
//   n_patients N | iterations K | masks 0/1     the context: n_cases + n_ctrls, its permutations, whether masks are set
//   W32p D | Kpad P | out 0/1 | max_mb X        dwords per plane, padded permutations, whether `out` is there, the bound
// Output: "check CODE [planes ...] MESSAGE".  The weights array has exactly the size the case gives it, so that a
// sanitizer sees any access beyond it.
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
  int64_t n_rows = 0;
  int32_t n_cols = 1, n_patients = 1, iterations = 0, W32p = 8, Kpad = 0;
  int have_out = 1, have_masks = 1;
  double max_mb = 1024;
  std::vector<int32_t> weights;
  bool have_weights = false;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    if (!(ls >> key)) continue;
    if (key == "n_rows") ls >> n_rows;
    else if (key == "n_cols") ls >> n_cols;
    else if (key == "n_patients") ls >> n_patients;
    else if (key == "iterations") ls >> iterations;
    else if (key == "masks") ls >> have_masks;
    else if (key == "W32p") ls >> W32p;
    else if (key == "Kpad") ls >> Kpad;
    else if (key == "out") ls >> have_out;
    else if (key == "max_mb") ls >> max_mb;
    else if (key == "weights") { have_weights = true; for (int64_t v; ls >> v;) weights.push_back((int32_t)v); }
    else return 2;
  }
  // the array is as large as the caller SAYS only where the check reads it: a shape it refuses (a negative row count, a
  // column count that is not the context's) is refused before an element is read
  const bool reads = n_rows >= 0 && n_cols == n_patients && have_out && (iterations == 0 || have_masks);
  if (have_weights && reads && weights.size() != (size_t)n_rows * (size_t)n_cols) return 2;

  // a list that is present is never NULL, even when it is empty: a heap array of exactly its size
  std::unique_ptr<int32_t[]> pw;
  if (have_weights) {
    pw.reset(new int32_t[weights.size()]);
    std::copy(weights.begin(), weights.end(), pw.get());
  }
  std::string msg;
  std::vector<int32_t> planes;
  const int rc = gcre_host::check_burden_args(pw.get(), n_rows, n_cols, n_patients, have_out != 0, iterations, have_masks != 0, W32p,
                                              Kpad, max_mb, "patient_burden", planes, msg);
  std::printf("check %d [", rc);
  for (size_t i = 0; i < planes.size(); i++) std::printf(i ? " %d" : "%d", planes[i]);
  std::printf("] %s\n", msg.c_str());
  return 0;
}

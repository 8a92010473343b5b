// gcre_threshold.h -- how an observed score enters the device: as the f32 pattern null scores are compared with.  Plain C++17,
// no HIP: the set-score host files include it through gcre_set_stage.h, the family plan (gcre_family.h) on its own, and with
// it tests/native/family_main.cpp under plain g++.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

namespace gcre_host __attribute__((visibility("hidden"))) {

// The bit pattern of the smallest float x with (double)x >= score, among the non-negative floats null scores are: null
// score r counts (R/ProcessPaths.R:316) iff its bits are >= this -- 0 when every one counts, past +inf when none does (NaN).
inline uint32_t f32_threshold(double score) {
  if (score != score) return 0x7f800001u;
  if (score <= 0) return 0u;
  float f = (float)score;
  if ((double)f < score) f = std::nextafter(f, std::numeric_limits<float>::infinity());
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

}  // namespace gcre_host

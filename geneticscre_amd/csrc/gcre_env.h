// gcre_env.h -- the two readers of the environment variables that bound what a set stage holds on the device, defined once:
// every plan header's X_max_mb() and X_slab_...() is one call of these.  Nothing is cached: the variables are read per call
// (the tests change them between calls).  Plain C++17, no HIP.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace gcre_env __attribute__((visibility("hidden"))) {

// a budget in MB (tests set fractions): `default_mb` when unset, else the value clamped to [0, cap_mb]
inline double env_mb(const char* name, double default_mb, double cap_mb) {
  const char* e = std::getenv(name);
  return e ? std::min(std::max(std::atof(e), 0.0), cap_mb) : default_mb;
}

// a bound on the items of a slab (tests): 0 = unset, no bound; else at least 1
inline int64_t env_count(const char* name) {
  const char* e = std::getenv(name);
  return e ? std::max<int64_t>(std::atoll(e), 1) : 0;
}

}  // namespace gcre_env

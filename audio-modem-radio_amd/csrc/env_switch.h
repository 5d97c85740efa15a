// env_switch.h -- the one way the host layer reads an environment switch.
// No HIP dependency (tests/test_env_switch.py compiles it with the host
// compiler).  The helpers read the environment on every call; a call site
// that wants the value fixed for the process keeps it in a `static const`.
//
//   value          unset  ""   "0"  "1"  "2"
//   env_on           0     0    0    1    0     on only when it starts with '1'
//   env_not_off      1     1    0    1    1     off only when it starts with '0'
//   env_tri         -1     0    0    1    0     -1 unset, else env_on
//   (only the first character is read: "10" is on, "01" is off)
//   env_int(lo, hi, fb): atoll of the value when that is within [lo, hi],
//   else fb (unset, "" -> 0, text -> 0 and out-of-range values included)
#pragma once
#include <stdint.h>

#include <cstdlib>

namespace amr {
inline bool env_on(const char* name) {
  const char* e = std::getenv(name);
  return e && e[0] == '1';
}
inline bool env_not_off(const char* name) {
  const char* e = std::getenv(name);
  return !(e && e[0] == '0');
}
inline int env_tri(const char* name) { return std::getenv(name) ? (env_on(name) ? 1 : 0) : -1; }
inline int64_t env_int(const char* name, int64_t lo, int64_t hi, int64_t fallback) {
  const char* e = std::getenv(name);
  const int64_t v = e ? std::atoll(e) : fallback;
  return e && v >= lo && v <= hi ? v : fallback;
}
}  // namespace amr

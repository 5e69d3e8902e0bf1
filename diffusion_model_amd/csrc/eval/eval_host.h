// Argument checks and scratch memory that the host sides of the evaluation families (eval/*_host.cpp, cells/cell_host.cpp) share.
// Plain C++ beside host_logic, header only: it is also compiled into the CPU-only sanitizer library (make asan).
#pragma once
#include <stdlib.h>

#include "../host_logic.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set, naming the entry `who`; the caller gives the limit.  Inline, so
// that a program which compiles one family's *_host.cpp needs no further source file.
inline int atom_types_check(const char* who, int A, int most) {   // 1 <= A <= most
  if (A < 1 || A > most) { set_error("%s: %d atom types (1 <= A <= %d)", who, A, most); return EGNN_EINVAL; }
  return EGNN_OK;
}

inline int tiles_check(const char* who, const void* tiles, int n_tiles) {   // n_tiles >= 0 tiles given
  if (n_tiles < 0 || (n_tiles > 0 && !tiles)) { set_error("bad %s arguments (n_tiles >= 0 tiles given)", who); return EGNN_EINVAL; }
  return EGNN_OK;
}

// step `at` of the pointer list `list` over things called `noun` ("graph", "cell"): it does not decrease and spans at most `most` atoms
inline int ptr_step_check(const char* who, const char* list, const char* noun, const int32_t* ptr, int at, int most) {
  const long long n = (long long)ptr[at + 1] - ptr[at];
  if (n < 0) { set_error("%s: %s decreases at %s %d", who, list, noun, at); return EGNN_EINVAL; }
  if (n > most) { set_error("%s: %s %d has %lld atoms (at most %d)", who, noun, at, n, most); return EGNN_EINVAL; }
  return EGNN_OK;
}

inline int type_range_check(const char* who, const int32_t* type, int begin, int end, int A) {   // atoms [begin, end): a type in [0, A)
  for (int i = begin; i < end; ++i)
    if (type[i] < 0 || type[i] >= A) { set_error("%s: atom %d has type %d outside [0, %d)", who, i, type[i], A); return EGNN_EINVAL; }
  return EGNN_OK;
}

// scratch of a host statement, zeroed.  Not std::vector: a constructor or push_back the compiler does not inline is instantiated as
// a weak symbol with default visibility, and the library exports nothing but the header's functions (tests/test_cabi_and_host.py)
template <typename T>
struct Scratch {
  T* p;
  explicit Scratch(size_t n) : p(static_cast<T*>(calloc(n ? n : 1, sizeof(T)))) {}
  ~Scratch() { free(p); }
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  bool reset(size_t n) {
    free(p);
    p = static_cast<T*>(calloc(n ? n : 1, sizeof(T)));
    return p != nullptr;
  }
  T& operator[](size_t i) { return p[i]; }
};

}  // namespace egnn

// Host-only argument validation of the ring statistics (rings.hip) and of their host statement.  Plain C++ beside host_logic: it is
// also compiled into the CPU-only sanitizer library (make asan).
#pragma once
#include <stdint.h>

#include "../host_logic.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set; nothing is launched before they pass
int rings_common_check(const char* who, int N, const void* row_ptr, int E, const void* atom, const void* type, int A, int M,
                       const void* centre, const void* angle_ptr, int n_angles, int max_size, int max_sites, const void* size,
                       const void* count, const void* overflow);
// the lists, where they can be read on the host (each may be NULL: not checked)
int rings_lists_check(const char* who, int N, const int32_t* row_ptr, int E, const int32_t* atom, const int32_t* shift, int M,
                      const int32_t* centre);

}  // namespace egnn

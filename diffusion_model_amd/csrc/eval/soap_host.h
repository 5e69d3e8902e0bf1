// Host-only argument validation of the SOAP entries (soap.hip) and of their host statement.  Plain C++ beside host_logic: it is
// also compiled into the CPU-only sanitizer library (make asan).
#pragma once
#include <stdint.h>

#include "eval_host.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set; nothing is launched before they pass
int soap_descriptor_check(const char* who, int B, int N, int A, const void* pos, const void* type, const void* graph_ptr, int n_max,
                          int l_max, double neighbour_cut, const void* tables, int n_centres, const int32_t* centres, const void* desc);
int soap_rows_check(const char* who, int F, const void* a, int rows_a, const void* b, int rows_b);
int soap_nearest_check(const char* who, int T, int R, int S, int k, const void* target, const void* reference, const void* idx,
                       const void* mse);

}  // namespace egnn

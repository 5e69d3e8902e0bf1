// Host-only argument validation of the topological fingerprint (topo.hip) and of its host statement.  Plain C++ beside
// host_logic: it is also compiled into the CPU-only sanitizer library (make asan).
#pragma once
#include "eval_host.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set; nothing is launched before they pass
int topo_common_check(const char* who, int B, int A, const void* type, const void* graph_ptr, int max_atoms);
int topo_threshold_check(const char* who, int A, const double* thr);
int topo_length_check(const char* who, int L);

}  // namespace egnn

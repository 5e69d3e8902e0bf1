// Host-only argument validation of the whole-structure statistics (structure.hip) and their host statement.  Plain C++ beside
// host_logic: it is also compiled into the CPU-only sanitizer library (make asan).
#pragma once
#include "eval_host.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set; nothing is launched before they pass
int struct_pair_args_check(const char* who, int B, int A, const void* pos, const void* type, const void* graph_ptr, int max_atoms,
                           double dR, int nbins, const void* counts);
int struct_bond_args_check(const char* who, int B, int A, const void* pos, const void* type, const void* graph_ptr, int max_atoms,
                           float cutoff, double dtheta, int max_cn, const void* cn, const void* angles);
int struct_finish_args_check(int B, int A, const void* counts, const void* type, const void* graph_ptr, double R, double dR,
                             double sigma, int nbins, const void* out);

}  // namespace egnn

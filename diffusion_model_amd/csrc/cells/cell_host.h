// Host-only argument validation of the periodic-cell entries (cell_env.hip) and their host statement egnn_cell_env_host.  Plain C++
// beside host_logic: it is also compiled into the CPU-only sanitizer library (make asan).
#pragma once
#include "../eval/eval_host.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set; nothing is launched before they pass.
// cell_ptr and lattice are HOST arrays here: sizes, monotony, cutoff > 0, a singular lattice and a perpendicular width below the
// cutoff are refused, naming the cell.  lattice may be null where an entry reads no lattice (the environment count).
int cell_batch_check(const char* who, int C, int N, const int32_t* cell_ptr, const double* lattice, double cutoff);
int cell_env_params_check(const char* who, int M, int shells, int max_atoms, const void* centre_cell, const void* centre);

}  // namespace egnn

// Host-only argument validation of the reciprocal-space statistics (sq.hip) and their host statement.  Plain C++ beside
// host_logic: it is also compiled into the CPU-only sanitizer library (make asan).
#pragma once
#include "eval_host.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set; nothing is launched before they pass
int sq_debye_args_check(const char* who, int B, int A, const void* pos, const void* type, const void* graph_ptr, int max_atoms, int Q,
                        const double* q, double r_max, int window, const void* out);
int sq_tiles_args_check(const char* who, const void* tiles, int n_tiles, const void* tile_ptr, const void* partial);
// the cells of a call: sizes, lattices (singular -> EINVAL), q_max against the index limit; hkl_box int32 [C, 3] where given
int sq_cells_check(const char* who, int C, int A, const int32_t* cell_ptr, const double* lattice, double q_max, int32_t* hkl_box);
int sq_bins_check(const char* who, double q_max, double dq, int nbins);
// the host copy of plan ([C, 4] = {H, K, L, first row}) against the lattices; *max_rows = the most rows of one cell
int sq_plan_check(const char* who, int C, const double* lattice, double q_max, const int32_t* plan, int n_rows, int* max_rows);
int sq_vec_ptr_check(const char* who, int C, const int32_t* vec_ptr, int K);

}  // namespace egnn

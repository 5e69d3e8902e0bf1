// Host-only argument validation of the linked-cell entries (cell_grid.hip) and their host statement egnn_cell_grid_host.  Plain C++
// beside host_logic: it is also compiled into the CPU-only sanitizer library (make asan).
#pragma once
#include "cell_stats_host.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set; nothing is launched before they pass.
// radius positive and finite, 1 <= reach <= 3, min_width >= 0 and finite
int cell_grid_params_check(const char* who, double radius, int reach, double min_width);
// nb int32 [C, 3] (HOST): every cell either 0, 0, 0 (not gridded) or a grid the walk of (radius, reach) is complete on
// (cell_grid_valid: 2 reach + 1 <= nb_k <= floor(reach w_k / rho)); *n_bins = the bins of the batch, below 2^31
int cell_grid_dims_check(const char* who, int C, const double* lattice, const int32_t* nb, double radius, int reach, int64_t* n_bins);
// tiles int32 [n_tiles, 2] (HOST) = {cell, first centre}: every cell named lies in [0, C) and is gridded
int cell_grid_tiles_check(const char* who, int C, const int32_t* nb, const int32_t* tiles, int n_tiles);

}  // namespace egnn

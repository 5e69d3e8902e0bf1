// Host-only argument validation of the real-space statistics of periodic cells (cell_stats.hip) and their host statement
// egnn_cell_stats_host.  Plain C++ beside cell_host: it is also compiled into the CPU-only sanitizer library (make asan).
#pragma once
#include "cell_host.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set; nothing is launched before they pass.  lattice is a HOST array.
// pair part: dR > 0 and finite, nbins >= 1, A A nbins bins within the LDS histogram, every cell regular and within 16 images per axis
int cell_stat_pair_check(const char* who, int C, int A, const double* lattice, double dR, int nbins);
// bond part: dtheta in [0.5, 180], 1 <= max_cn <= 64, former and bridge two different types below A
int cell_stat_bond_check(const char* who, int A, double dtheta, int max_cn, int former, int bridge);

}  // namespace egnn

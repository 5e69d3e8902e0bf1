// Host-only argument validation of the periodic-cell SOAP entries (cell_soap.hip) and of their host statements.  Plain C++ beside
// host_logic: it is also compiled into the CPU-only sanitizer library (make asan).
#pragma once
#include "cell_host.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set; nothing is launched before they pass.
// the batch of an entry over the sites of every image: cell_batch_core_check (cell_host.h) and, where cut > 0, a perpendicular
// width <= cut / 4 (the image box would pass 4) refused, naming the cell and its widths.  cut = 0: the entry reads no cut.
int cell_soap_batch_check(const char* who, int C, int N, const int32_t* cell_ptr, const double* lattice, double cut);
int cell_soap_basis_check(const char* who, int A, int n_max, int l_max, const void* tables);

}  // namespace egnn

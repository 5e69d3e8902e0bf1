// Host-only argument validation of egnn_assign / egnn_assign_prealign (assign.hip).  Plain C++ beside host_logic: it is also
// compiled into the CPU-only sanitizer library (make asan), where tests/test_assign_host.py calls it without a GPU.
#pragma once
#include "../host_logic.h"

namespace egnn {

constexpr int kPrealignMinAtoms = 5;   // smallest min_atoms of the pre-alignment: atom 0 and four neighbours

int assign_args_check(int B, const void* P, const void* Q, const void* graph_ptr, int max_atoms, const void* col, const void* cost,
                      const void* solved);
int assign_prealign_args_check(int B, const void* orig, const void* gen, const void* graph_ptr, int min_atoms, const void* R,
                               const void* prealigned);

}  // namespace egnn

// Host-only logic of the assignment entry points (see assign_host.h).  Plain C++: no HIP call, no device code.
#include "assign_host.h"

namespace egnn {

int assign_args_check(int B, const void* P, const void* Q, const void* graph_ptr, int max_atoms, const void* col, const void* cost,
                      const void* solved) {
  if (B < 1 || !P || !Q || !graph_ptr || !col || !cost || !solved || max_atoms < 1 || max_atoms > EGNN_ASSIGN_MAX_ATOMS) {
    set_error("bad egnn_assign arguments (B >= 1, 1 <= max_atoms <= %d)", EGNN_ASSIGN_MAX_ATOMS);
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

int assign_prealign_args_check(int B, const void* orig, const void* gen, const void* graph_ptr, int min_atoms, const void* R,
                               const void* prealigned) {
  if (B < 1 || !orig || !gen || !graph_ptr || !R || !prealigned || min_atoms < kPrealignMinAtoms) {
    set_error("bad egnn_assign_prealign arguments (B >= 1, min_atoms >= %d: atom 0 and four neighbours)", kPrealignMinAtoms);
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

}  // namespace egnn

// Test-only C entry points of the sanitizer build, as in host_logic.cpp.  Not exported by libegnn_amd.so.
#ifdef EGNN_HOST_TEST_API
extern "C" {
int egnn_host_assign_args_check(int B, const void* P, const void* Q, const void* graph_ptr, int max_atoms, const void* col,
                                const void* cost, const void* solved) {
  return egnn::assign_args_check(B, P, Q, graph_ptr, max_atoms, col, cost, solved);
}
int egnn_host_assign_prealign_args_check(int B, const void* orig, const void* gen, const void* graph_ptr, int min_atoms, const void* R,
                                         const void* prealigned) {
  return egnn::assign_prealign_args_check(B, orig, gen, graph_ptr, min_atoms, R, prealigned);
}
}
#endif

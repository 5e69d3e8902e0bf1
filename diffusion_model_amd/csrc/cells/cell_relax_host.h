// Host-only argument validation of the relaxation entries (cell_relax.hip) and of their host statements.  Plain C++ beside
// host_logic: it is also compiled into the CPU-only sanitizer library (make asan).
#pragma once
#include "cell_ewald_host.h"
#include "cell_relax_math.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set; nothing is launched before they pass.
// The FIRE parameters of a call: dt_max, f_inc, f_dec, a_start, f_a, max_step, f_max and skin positive and finite, f_dec < 1 <= f_inc,
// a_start <= 1, f_a <= 1, n_min >= 0, max_steps >= 0, max_step <= skin / 2.
int cell_relax_fire_check(const char* who, double dt_max, int n_min, double f_inc, double f_dec, double a_start, double f_a, double max_step,
                          double f_max, int max_steps, double skin, FireModel* model);
// the batch of a step: the host copy of cell_ptr runs from 0 to N in steps of at most kCellMaxAtoms atoms, no lattice is singular
int cell_relax_batch_check(const char* who, int C, int N, const int32_t* cell_ptr, const double* lattice);
// one step of cell c on host arrays (the order of cell_relax_math.h); coincident: whether the evaluation flagged the cell
void cell_relax_step_cell(const FireModel& M, int c, int C, const int32_t* cell_ptr, const double* lattice, const double* force, double energy,
                          bool coincident, double* frac, double* velocity, double* since, double* moved, double* scalars, int32_t* counters,
                          int32_t* done, int32_t* rebuild, double* energy_trace, double* force_trace);

}  // namespace egnn

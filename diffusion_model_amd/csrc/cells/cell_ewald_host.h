// Host-only argument validation of the lattice-energy entries (cell_ewald.hip) and of their host statement.  Plain C++ beside
// host_logic: it is also compiled into the CPU-only sanitizer library (make asan).
#pragma once
#include "../eval/sq_host.h"
#include "cell_ewald_math.h"
#include "cell_soap_host.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set; nothing is launched before they pass.
// The model of a call from its HOST arguments: charges double [A]; pot double [4, A, A] = the tables A, b, C, D (null: Coulomb
// only), symmetric and finite; 1 <= n <= kEwaldMaxPower; kappa, alpha, r_cut, k_max positive and finite, 0 < short_cut <= r_cut.
// u_cut = u_ab(short_cut) where `shift` is set: computed here, once, for the kernels and the host statement alike.
int cell_ewald_model_check(const char* who, int A, const double* charges, const double* pot, int n, int shift, double kappa, double alpha,
                           double r_cut, double short_cut, double k_max, int forces, EwaldModel* model);
// the batch of an entry: the image box of r_cut within 4 (cell_soap_batch_check) and the index need of k_max within the limit of
// sq_index_need (sq_cells_check)
int cell_ewald_batch_check(const char* who, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, double r_cut, double k_max);
// the vector table of cell c for the host statements (egnn_cell_ewald_host, egnn_cell_ewald_virial_host): the half-space vectors
// below P.k_max in ascending (h, k, l) and (k_x, k_y, k_z, g S^c, g S^s) of each, the amplitudes over the na atoms (wrapped
// coordinates w [na, 3], types type [na]) in ascending order; none where every charge is 0.  EGNN_EINVAL above kSqMaxVectors.
int cell_ewald_vector_table(const char* who, int c, const EwaldModel& P, const double* L, const double* w, const int32_t* type, int na,
                            int64_t* n_vectors, Scratch<int32_t>* hkl, Scratch<double>* table);
inline bool cell_ewald_charged(const EwaldModel& P) {
  for (int a = 0; a < P.A; ++a)
    if (P.charge[a] != 0.0) return true;
  return false;
}

}  // namespace egnn

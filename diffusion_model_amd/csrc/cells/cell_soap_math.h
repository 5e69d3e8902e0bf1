// Definitions of the SOAP descriptors of periodic cells (cell_soap.hip, cell_soap_host.cpp): the sites of every image about a
// centre and the descriptor over them.  Plain C++ behind the host/device macro, so that the kernels and the host statement read the
// same text.  dscribe's SOAP(periodic=True) is the behaviour restated, from its description: not pinned by execution.
//
//  * cut: the neighbour cut, r_cut + sigma sqrt(2 ln 1000) by default (soap_math.h).
//  * sites of centre i of a cell: every (j, s), s in Z^3, with cell_norm2(r) < cut * cut in fp64, r = cell_site_vector on the
//    wrapped coordinates (cell_math.h: the text the bond kernels compile).  The centre itself, (i, 0), is a site at r = 0 exactly;
//    its own images (i, s != 0) are ordinary sites.
//  * image box: b_k = floor(cut / w_k) + 1, w the perpendicular widths (cell_widths).  It is never below the complete bound:
//    |d_k| w_k <= |r| < cut and |w_j - w_i| < 1 give |s_k| < cut / w_k + 1.  A larger box cannot change membership: only the
//    distance test decides.  b_k <= 4 is required, so that cell_shift_code holds every site: a cell with a width <= cut / 4 or a
//    singular lattice is refused.
//  * candidates of a centre: q = j nbox + t, j the atom inside its cell, nbox = prod (2 b_k + 1), t the shifts of the box ascending
//    in (s_x, s_y, s_z), which is ascending shift code: ascending q is ascending key atom * 729 + code.
//  * order: the centre first, then every other site by ascending key (the rows of an EnvironmentBatch).  Every sum over sites runs
//    in this order.
//  * site list: CSR rows in the format of a bond-list row (atom as index into the batch, shift code), ascending, (i, 0) left out.
//  * descriptor: exactly soap_math.h -- soap_solid_column, soap_radial, beta over n, soap_power_entry, the same tables -- fed r and
//    d2 = cell_norm2(r) in fp64.  Nothing is rounded to float32.
//  * mean over a cell: the rows of its centres added in ascending centre order into one running fp64 sum, divided once by their
//    number; a cell without a centre has a row of zeros.
#pragma once
#include "../eval/soap_math.h"
#include "cell_math.h"

namespace egnn {

constexpr int kCellSoapMaxBox = 4;      // b_k: what the shift code holds
constexpr int kCellSiteWaves = 4;       // site tile: centres, one wavefront each

// the image box of one cell; false for a singular lattice (w untouched) or a box beyond 4 (w written: the message names them)
EGNN_HD bool cell_soap_box(const double* L, double cut, int* b, double* w) {
  w[0] = w[1] = w[2] = 0.0;
  if (!cell_widths(L, w)) return false;
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    const double q = floor(cut / w[k]) + 1.0;
    if (!(q <= (double)kCellSoapMaxBox)) { ok = false; b[k] = 0; continue; }
    b[k] = (int)q;
  }
  return ok;
}

EGNN_HD int cell_soap_box_count(const int* b) { return ((2 * b[0] + 1) * (2 * b[1] + 1)) * (2 * b[2] + 1); }

// shift t of the box, ascending in (s_x, s_y, s_z)
EGNN_HD void cell_soap_box_shift(int t, const int* b, int* s) {
  const int n1 = 2 * b[1] + 1, n2 = 2 * b[2] + 1;
  s[0] = t / (n1 * n2) - b[0];
  s[1] = t / n2 % n1 - b[1];
  s[2] = t % n2 - b[2];
}

// whether image s of the atom at wrapped wj is a site of the centre at wrapped wi; r is its vector either way
EGNN_HD bool cell_soap_site(const double* wj, const double* wi, const int* s, const double* L, double cut2, double* r) {
  cell_site_vector(wj, wi, s, L, r);
  return cell_norm2(r) < cut2;
}

}  // namespace egnn

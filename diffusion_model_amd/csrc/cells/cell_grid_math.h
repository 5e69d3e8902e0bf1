// Definitions of the linked-cell grid of periodic cells (cell_grid.hip, cell_grid_host.cpp): the bins of a cell, the sorted order of
// its atoms and the candidate sites of a centre.  Plain C++ behind the host/device macro, so that the kernels and the host statement
// read the same text.  An extension (no file of the reference bins a cell); the site vector, the wrap and the widths are those of
// cell_math.h, the pair bin and its cull those of cell_stats_math.h.  Nothing is restated here: the grid only chooses WHICH sites
// (j, s) are handed to the existing text, so a bond list or a pair histogram found through it holds the bits of the direct walk.
//
//  * grid of a cell for a search radius `radius` and a reach m >= 1 (bins walked to each side): rho = radius (1 + 1e-6), the margin
//    of cell_bond_kernel and cell_stat_axis_reach; nb_k = floor(m w_k / max(rho, m min_width)), at most 256, with the perpendicular
//    widths w of cell_widths.  min_width >= 0 asks for bins at least that thick; a coarser grid is always valid.  The cell is
//    griddable iff nb_k >= 2 m + 1 on all three axes; there are no mixed axes.
//  * bin of an atom: b_k = min(nb_k - 1, (int)floor(cell_wrap(f_k) nb_k)), flat (b_0 nb_1 + b_1) nb_2 + b_2.
//  * sorted order: the atoms of a cell ascending by (flat bin, atom index).
//  * candidates of centre i: for every offset in [-m, m]^3, raw_k = b_k(i) + offset_k, s_k = floor_div(raw_k, nb_k) in {-1, 0, 1},
//    bin raw_k - s_k nb_k; every atom j of that bin is the candidate site (j, s).  nb_k >= 2 m + 1 makes the (2 m + 1)^3 bins
//    distinct: a site is visited at most once.  A bin is at least rho / m thick, so a site with |r| < radius, |d_k| w_k <= |r|, lies
//    fewer than m (1 - 1e-6) + 1 bins away: it is among the candidates, with a margin ten orders above the rounding of w nb_k.
//  * whether a candidate counts is decided by cell_site_vector with exactly that s and cell_norm2(r) < cutoff^2 (a bond) or
//    cell_stat_bin (a pair), (i, 0) excluded: the text of the direct kernels.
#pragma once
#include "cell_stats_math.h"

namespace egnn {

constexpr int kCellGridMaxBins = 256;       // nb_k
constexpr int kCellGridMaxReach = 3;        // m
constexpr int kCellGridMaxOffsets = 343;    // (2 m + 1)^3
constexpr int kCellGridRowKeys = 128;       // fill pass of the bond list: keys of a row staged per wavefront; a longer row is ranked in pieces

// nb[3] of one cell; false for a singular lattice.  nb = 0, 0, 0 where the cell is not griddable.
EGNN_HD bool cell_grid_dims(const double* L, double radius, int reach, double min_width, int* nb) {
  double w[3];
  if (!cell_widths(L, w)) return false;
  const double rho = radius * (1.0 + 1e-6);
  const double thick = (double)reach * min_width;
  const double per = rho > thick ? rho : thick;
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    const double q = floor((double)reach * w[k] / per);
    nb[k] = q < (double)kCellGridMaxBins ? (q > 0.0 ? (int)q : 0) : kCellGridMaxBins;
    ok = ok && nb[k] >= 2 * reach + 1;
  }
  if (!ok) nb[0] = nb[1] = nb[2] = 0;
  return true;
}

// the finest grid the walk of (radius, reach) is complete on: nb_k <= floor(reach w_k / rho).  `nb` may be coarser, never finer,
// and needs 2 reach + 1 bins per axis.
EGNN_HD bool cell_grid_valid(const double* L, double radius, int reach, const int* nb) {
  int most[3];
  if (!cell_grid_dims(L, radius, reach, 0.0, most)) return false;
  for (int k = 0; k < 3; ++k)
    if (nb[k] < 2 * reach + 1 || nb[k] > most[k]) return false;
  return true;
}

EGNN_HD int cell_grid_axis_bin(double f, int nb) {
  const int b = (int)floor(cell_wrap(f) * (double)nb);
  return b < nb - 1 ? b : nb - 1;
}
EGNN_HD int cell_grid_flat(const int* b, const int* nb) { return (b[0] * nb[1] + b[1]) * nb[2] + b[2]; }
EGNN_HD int cell_grid_bin(const double* f, const int* nb) {
  const int b[3] = {cell_grid_axis_bin(f[0], nb[0]), cell_grid_axis_bin(f[1], nb[1]), cell_grid_axis_bin(f[2], nb[2])};
  return cell_grid_flat(b, nb);
}
EGNN_HD void cell_grid_unflat(int flat, const int* nb, int* b) {
  b[2] = flat % nb[2];
  b[1] = flat / nb[2] % nb[1];
  b[0] = flat / (nb[2] * nb[1]);
}

// offset `t` of the (2 m + 1)^3, ascending (x, y, z), about the centre's bin b: the candidate bin (flat) and the shift of its atoms
EGNN_HD int cell_grid_candidate(const int* b, const int* nb, int reach, int t, int* s) {
  const int span = 2 * reach + 1;
  const int off[3] = {t / (span * span) - reach, t / span % span - reach, t % span - reach};
  int cb[3];
  for (int k = 0; k < 3; ++k) {
    const int raw = b[k] + off[k];
    s[k] = raw < 0 ? -1 : (raw >= nb[k] ? 1 : 0);
    cb[k] = raw - s[k] * nb[k];
  }
  return cell_grid_flat(cb, nb);
}

}  // namespace egnn

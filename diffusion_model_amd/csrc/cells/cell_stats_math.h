// Definitions of the real-space statistics of periodic cells (cell_stats.hip, cell_stats_host.cpp): partial pair counts over every
// centre and every image, coordination numbers, bond angles and the Q^n speciation of the network formers.  Plain C++ behind the
// host/device macro, so that the kernels and the host statement read the same text.  They extend evaluate_RDF.py:39-60,
// evaluate_Si-O-Si.py:23-41 and CN2_evaluate.py:12-16 (one cluster, atom 0) to the INFINITE lattice of a cell; no file of the
// reference computes them for a cell (an extension, like the rings and S(q)).  The site vector, the wrap and the widths are those of
// cell_math.h; the angle bin and the smoothing filter those of eval/structure_math.h.  Nothing is restated here.
//
//  * pair: an ordered (i, (j, s)), s in Z^3, (j, s) != (i, 0).  An atom pairs with its own images (j = i, s != 0).  Its vector is
//    cell_site_vector (fp64, one fixed order; the library is built with -ffp-contract=off), r2 = cell_norm2(r), r = sqrt(r2).
//  * radial bin: k = floor(r / dR) and the pair counts iff k < nbins: bin k is [k dR, (k + 1) dR), the spelling of the shell bin of
//    eval/sq_math.h.  The caller takes nbins = floor(R / dR + 0.5); the effective radius is nbins dR.  NOT the reference's bin set
//    (dR + k dR, dR + (k + 1) dR) that stats.rdf and stats.pair_counts keep for clusters.
//  * image box: the wrapped fractional differences lie in (-1, 1) and |r| >= |d_k| w_k with the perpendicular widths w of
//    cell_widths, so |s_k| <= S_k = ceil(nbins dR / w_k) holds every pair that counts.  S_k <= 16.
//  * whether a pair counts is decided by the one fp64 comparison of cell_stat_bin and by nothing else; a kernel may skip a pair
//    only where cell_stat_axis_reach or cell_stat_r2_limit say, with margins a billion roundings wide, that it cannot count.
//  * swapping the two atoms of a pair negates d, and every product and sum of cell_cartesian with it, exactly: r2 is the same
//    bits, so c[a][b][k] == c[b][a][k].
//  * bonds are those of the periodic bond list (cell_math.h: r2 < cutoff^2, rows ascending by (atom, shift code)).
//    coordination[i][b] = bonds of atom i to type b; cn[a][b][m] = atoms of type a with m bonds to type b, the last bin max_cn or more.
//  * angles: bond vectors by cell_site_vector, pairs p < q in row order, struct_angle_bin; the first kMaxNeighbours = 64 bonds of a
//    row at most: a centre with more counts in cn and coordination, gives no angle and is reported per cell.
//  * Q^n of atom i of type `former`: its bonds to atoms j of type `bridge` with coordination[j][former] >= 2 (a bridging oxygen),
//    counted per bond; -1 for every other atom.  The histogram has max_cn + 1 bins, the last saturating.
#pragma once
#include "../eval/structure_math.h"
#include "cell_math.h"

namespace egnn {

constexpr int kCellStatMaxImages = 16;           // S_k
constexpr int kCellStatMaxHist = 16384;          // A A nbins: 64 KiB of int32 bins in LDS
constexpr int kCellStatCentreBlock = 64;         // pair tile: centres
constexpr int kCellStatChunk = 1024;             // pair tile: neighbour atoms staged in LDS
constexpr int kCellStatBondCentres = 8;          // bond tile: centres, two per wavefront

// the bin of distance r, -1 where the pair does not count (k >= nbins, or r not finite)
EGNN_HD int cell_stat_bin(double r, double dR, int nbins) {
  const double k = floor(r / dR);
  return k < (double)nbins ? (int)k : -1;
}

// S_k = ceil(nbins dR / w_k); false for a singular lattice.  A value beyond the limit is returned as kCellStatMaxImages + 1.
EGNN_HD bool cell_stat_image_box(const double* L, double dR, int nbins, int* S) {
  double w[3];
  if (!cell_widths(L, w)) return false;
  for (int k = 0; k < 3; ++k) {
    const double s = ceil((double)nbins * dR / w[k]);
    S[k] = s <= (double)kCellStatMaxImages ? (int)s : kCellStatMaxImages + 1;
  }
  return true;
}

// conservative culls: |d_k| >= reach_k or r2 >= limit cannot count (|r| >= |d_k| w_k; floor(r / dR) >= nbins).  The margin of
// 1e-6 is ten orders above the roundings of d_k, r2 and the quotient.
EGNN_HD double cell_stat_axis_reach(double dR, int nbins, double width) { return (double)nbins * dR * (1.0 + 1e-6) / width; }
EGNN_HD double cell_stat_r2_limit(double dR, int nbins) {
  const double r = (double)nbins * dR * (1.0 + 1e-6);
  return r * r;
}

// piece `piece` of `pieces` of the first shift component's values -S .. S: [lo, hi) as offsets 0 .. 2S + 1
EGNN_HD void cell_stat_piece(int S, int piece, int pieces, int* lo, int* hi) {
  const int span = 2 * S + 1;
  *lo = (int)((long long)piece * span / pieces);
  *hi = (int)((long long)(piece + 1) * span / pieces);
}

}  // namespace egnn

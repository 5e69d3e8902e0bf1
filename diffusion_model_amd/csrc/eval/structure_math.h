// Definitions of the whole-structure statistics (structure.hip, structure_host.cpp): partial pair counts, coordination numbers and
// bond angles of EVERY centre of a graph.  Plain C++ behind a host/device macro (the pattern of kabsch_math.h), so that the kernels
// and the host statement read the same text.  They generalise evaluate_RDF.py:39-60 (RDF about atom 0 -> every centre, by type),
// evaluate_Si-O-Si.py:23-41 (the bond rule `norm < cutoff` about atom 0 -> every centre) and CN2_evaluate.py:12-16 (the angle).
//
//  * distance: float32, in exactly this order: dx = q.x - p.x (float32), d = sqrtf((dx*dx + dy*dy) + dz*dz).  The library is built
//    with -ffp-contract=off and sqrtf is correctly rounded on host and device, so a numpy float32 restatement that keeps this order
//    (tests/_struct_util.py) is bitwise equal.  It is the order of rdf_kernel and sio_si_kernel (graph_stats.hip).
//  * radial bin: rdf_kernel's rule unchanged: bin k < nbins holds d iff (float)(dR + k*dR) < d < (float)(dR + k*dR + dR), the
//    edges computed in double and rounded to float32 afterwards; a distance on an edge, or below dR, is in no bin.
//  * bond: j != i is a bond of centre i iff d_ij < cutoff (float32, the comparison of sio_si_kernel).
//  * angle at centre i between bonds j < k: fp64 from the float32 positions, v = (double)p_j - (double)p_i, w likewise,
//    c = v.w / (sqrt(v.v) * sqrt(w.w)) clamped to [-1, 1], theta = acos(c) * 180/pi, bin floor(theta/dtheta + 0.5): bins CENTRED on
//    the multiples of dtheta, so 90, 109.47, 120 and 180 degrees of a perfect lattice stay away from bin edges.  A zero-length
//    bond vector has no angle.
//  * smoothing: scipy's gaussian_filter1d(sigma) as rdf_kernel spells it (reflect boundary, truncation at 4 sigma).
#pragma once
#include "eval_math.h"

namespace egnn {

constexpr int kStructMaxTypes = 4;          // A
constexpr int kStructMaxBins = 1024;        // nbins, as egnn_rdf
constexpr int kStructMaxAngleBins = 361;    // dtheta >= 0.5 degrees
constexpr int kStructMaxAtoms = 32768;      // n (n - 1) ordered pairs of one graph stay inside int32
constexpr int kStructMaxCn = 64;            // max_cn
constexpr int kMaxNeighbours = 64;          // bonds of one centre whose angles are taken
constexpr int kStructCentreBlock = 64;      // pair tile: centres
constexpr int kStructChunk = 1024;          // pair tile: neighbour atoms
constexpr int kStructBondCentres = 8;       // bond tile: centres

EGNN_HD float struct_distance(float px, float py, float pz, float qx, float qy, float qz) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// a bin index within one of the bin (if any) that holds d, from float32 arithmetic: d * inv_dR is within 1e-3 of d / dR for every
// d below (nbins + 2) dR, and the bin that holds d is floor(d / dR) - 1 or its lower neighbour, so the caller tests guess - 1,
// guess and guess + 1 with struct_in_bin.  Distances beyond the last bin (and NaN) return nbins + 2: no candidate is a bin.
EGNN_HD int struct_bin_guess(float d, float inv_dR, int nbins) {
  const float t = d * inv_dR;
  if (!(t < (float)(nbins + 2))) return nbins + 2;
  return (int)t - 1;
}

EGNN_HD bool struct_in_bin(float d, int k, double dR) {
  const double rk = dR + (double)k * dR;
  return (float)rk < d && d < (float)(rk + dR);
}

EGNN_HD int struct_angle_bins(double dtheta) { return (int)floor(180.0 / dtheta + 0.5) + 1; }

// angle bin of the bond vectors v and w, -1 where one of them has no length
EGNN_HD int struct_angle_bin(const double* v, const double* w, double dtheta, int nth) {
  const double vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  const double ww = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  if (!(vv > 0.0) || !(ww > 0.0)) return -1;
  const double vw = (v[0] * w[0] + v[1] * w[1]) + v[2] * w[2];
  double c = vw / (sqrt(vv) * sqrt(ww));
  c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
  const double theta = acos(c) * (180.0 / M_PI);
  const int k = (int)floor(theta / dtheta + 0.5);
  return k < nth ? k : nth - 1;
}

// ---- Gaussian smoothing of a curve of nbins values, as rdf_kernel's ----
EGNN_HD int struct_smooth_half_width(double sigma) { return (int)(4.0 * sigma + 0.5); }
EGNN_HD double struct_smooth_weight(int t, double sigma) { return exp(-0.5 * (double)t * t / (sigma * sigma)); }
EGNN_HD int struct_reflect(int idx, int nbins) {   // 'reflect': (d c b a | a b c d | d c b a)
  const int period = 2 * nbins;
  idx %= period;
  if (idx < 0) idx += period;
  if (idx >= nbins) idx = period - 1 - idx;
  return idx;
}
EGNN_HD double struct_smooth_at(const double* raw, int nbins, int k, double sigma, int lw, double wsum) {
  double acc = 0.0;
  for (int t = -lw; t <= lw; ++t) acc += raw[struct_reflect(k + t, nbins)] * struct_smooth_weight(t, sigma);
  return acc / wsum;
}

}  // namespace egnn

// Definitions of the strain derivative of the lattice energy of periodic cells (cell_stress.hip, cell_stress_host.cpp): the Ewald
// virial, the stress tensor and the pressure.  On top of cell_ewald_math.h: the same sites, the same vector table, the same
// amplitudes.  Plain C++ behind the host/device macro, so that the kernels and the host statement compile the same text.  An
// extension: no file of the reference computes a stress.
//
// A homogeneous strain eps acts as L -> L (1 + eps) with the fractional coordinates held: a site vector d -> d (1 + eps), the
// phases h . w do not move, k -> k (1 - eps) and V -> V (1 + tr eps) to first order.  alpha, r_cut, short_cut, k_max and the
// membership of sites and vectors are held, as they are for the forces.  D_xy = dE / d eps_xy (eV) is symmetric and stored as six
// numbers in Voigt order xx, yy, zz, yz, xz, xy (kVoigtX, kVoigtY); it is split per atom and per component as the energy is.
//
//  * force factors of a site at r2 > 0 (ewald_site_factors): r = sqrt(r2), ar = alpha * r, ec = erfc(ar) / r;
//    f_real = (-(kappa * q_i)) * ((q_j * (ec + ((2 / sqrt pi) * alpha) * exp(-(ar * ar)))) / r2), the Coulomb part of the f of
//    ewald_site to the bit; f_short = u'_ab(r) / r where a potential is given and r < short_cut (ewald_pair), else 0.  The shift
//    constant u_cut does not depend on the strain.
//  * virial term of a site, component v = (x, y): f * (d_x * d_y), once with f_real and once with f_short (ewald_virial_add: twelve
//    running sums).  Per atom: D_real = 0.5 * (sum of the real terms), D_short = 0.5 * (sum of the short terms).
//  * reciprocal part, per vector m from the stored k (ewald_recip_B): k2 = cell_norm2(k), c = 2 * (1 / k2 + 1 / ((4 alpha) alpha)),
//    B_v = (k_x * k_y) * c - delta_xy: dg / d eps_xy = 2 k_x k_y g (1 / k^2 + 1 / (4 alpha^2)) and d(1 / V) / d eps_xy =
//    -delta_xy / V.  Per atom: D_rec,v = (((4 pi * kappa) / V) * q_i) * sum_m term_im * B_m,v, term_im the energy term of
//    cell_ewald_math.h (ewald_recip_energy_term) and the prefactor that of ewald_recip_energy.
//  * self: 0.  Background: D_v = -e_background,i on the diagonal (v < 3), 0 off it.
//  * per atom: D_v = (((real + reciprocal) + self) + background) + short (ewald_atom_energy on the five numbers of component v).
//    Per cell: each component and the total summed over the cell's atoms in ascending order, one running sum each.
//  * stress_v = D_v / V (eV / A^3, tension positive); pressure = -(((s_xx + s_yy) + s_zz) / 3).
//
// Orders of the sums: those of cell_ewald_math.h.  The host statement adds the sites and the vectors of an atom in ascending order
// into one running sum each; the kernels give lane l the entries l, l + 64, .. and add the 64 lane sums by the butterfly wave_sum.
#pragma once
#include "cell_ewald_math.h"

namespace egnn {

constexpr int kVoigt = 6;   // xx, yy, zz, yz, xz, xy

EGNN_HD int voigt_x(int v) { return v < 3 ? v : (v == 3 ? 1 : 0); }
EGNN_HD int voigt_y(int v) { return v < 3 ? v : (v == 5 ? 1 : 2); }

// the two force factors of one site at r2 > 0: fr (Coulomb, the first term of the f of ewald_site) and fs (pair potential)
EGNN_HD void ewald_site_factors(const EwaldModel& P, int ti, int tj, double r2, double* fr, double* fs) {
  const double r = sqrt(r2), ar = P.alpha * r, ec = erfc(ar) / r, qj = P.charge[tj];
  *fr = (-(P.kappa * P.charge[ti])) * ((qj * (ec + (kEwaldTwoOverSqrtPi * P.alpha) * exp(-(ar * ar)))) / r2);
  *fs = 0.0;
  if (P.has_potential && r < P.short_cut) {
    double u, du;
    ewald_pair(P, ti * P.A + tj, r2, r, &u, &du);
    *fs = du / r;
  }
}

// sum[v] += fr * (d_x d_y), sum[6 + v] += fs * (d_x d_y)
EGNN_HD void ewald_virial_add(double fr, double fs, const double* d, double* sum) {
  for (int v = 0; v < kVoigt; ++v) {
    const double dd = d[voigt_x(v)] * d[voigt_y(v)];
    sum[v] += fr * dd;
    sum[kVoigt + v] += fs * dd;
  }
}
EGNN_HD double ewald_virial_site_sum(double sum) { return 0.5 * sum; }

// B_m of a vector from its stored k
EGNN_HD void ewald_recip_B(const double* kv, double alpha, double* B) {
  const double k2 = cell_norm2(kv), c = 2.0 * (1.0 / k2 + 1.0 / ((4.0 * alpha) * alpha));
  for (int v = 0; v < kVoigt; ++v) B[v] = (kv[voigt_x(v)] * kv[voigt_y(v)]) * c - (v < 3 ? 1.0 : 0.0);
}

EGNN_HD double ewald_virial_background(double e_background, int v) { return v < 3 ? -e_background : 0.0; }
EGNN_HD double ewald_pressure(const double* stress) { return -(((stress[0] + stress[1]) + stress[2]) / 3.0); }

}  // namespace egnn

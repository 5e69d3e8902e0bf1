// Definitions of the lattice energy of periodic cells (cell_ewald.hip, cell_ewald_host.cpp): the Ewald sum of point charges plus a
// short-range pair potential (Buckingham with an optional D / r^n repulsion: BKS), per-atom energies and forces.  Plain C++ behind
// the host/device macro, so that the kernels and the host statement compile the same text.  An extension: no file of the reference
// computes an energy.
//
// Units: Angstrom and eV.  Charges are per TYPE, q_i = charge[type_i]; kappa is the Coulomb constant (eV A); V = |det L|, the
// determinant in the order of cell_widths, (a_0 bc_0 + a_1 bc_1) + a_2 bc_2.
//
//  * sites of centre i: the rows of egnn_cell_sites_* at cut = r_cut (cell_soap_math.h: every image, cell_norm2(d) < r_cut^2 in
//    fp64, (i, 0) left out, ascending (atom, shift code)); d = cell_site_vector, r2 = cell_norm2(d), r = sqrt(r2).  A site with
//    r2 == 0 (coincident atoms) contributes nothing and flags its cell: the caller refuses the cell.
//  * real term of a site (ewald_site): ar = alpha * r, ec = erfc(ar) / r; energy term q_j * ec; force factor
//    f = (-(kappa * q_i)) * ((q_j * (ec + ((2 / sqrt pi) * alpha) * exp(-(ar * ar)))) / r2).
//  * short term of a site, where a potential is given and r < short_cut: u_ab(r) = (A exp(-(b r)) - C / r6) + D / rn, r6 = (r2 r2) r2,
//    rn = r^n by ewald_ipow (binary powers, one fixed order), the D term skipped where D == 0; energy term u_ab(r) - u_cut[ab], u_cut
//    = u_ab(short_cut) where `shift` is set and 0 otherwise, computed ONCE on the host for both statements; f += u'_ab(r) / r,
//    u' = ((-(A b)) exp(-(b r)) + (6 C) / (r6 r)) - (n D) / (rn r).  ab = type_i * A + type_j; the tables are symmetric.
//  * per atom: e_real = ((0.5 * kappa) * q_i) * (sum of the real terms), e_short = 0.5 * (sum of the short terms),
//    F_x = sum of f * d_x: F = -dE/dr_i.
//  * vectors of a cell: m = (h, k, l) with sq_is_vector(m, Bm, k_max) (sq_math.h: the half space, k2 < k_max^2), ascending (h, k, l),
//    inside the index box of sq_index_need / sq_index_box.  k_m by ewald_kvec (the expression of sq_k2), g_m = exp(-(k2 / ((4 alpha)
//    alpha))) / k2.
//  * structure amplitude: S^c_m = sum_j q_j cos phi_jm, S^s_m = sum_j q_j sin phi_jm over the atoms of the cell in ascending order,
//    phi = 2 pi t, t = sq_phase (the phase (h w_0 + k w_1) + l w_2 on the wrapped coordinates, mod 1), the sine and cosine by
//    sq_phase_sincos.  Stored per vector: (k_x, k_y, k_z, g_m S^c_m, g_m S^s_m).
//  * reciprocal part of atom i: term_m = cos phi_im * (g S^c)_m + sin phi_im * (g S^s)_m, e_rec = (((4 pi * kappa) / V) * q_i) * sum;
//    force term_m = sin phi_im * (g S^c)_m - cos phi_im * (g S^s)_m, F_x += (((8 pi * kappa) / V) * q_i) * sum_m k_x term_m.  The
//    factor 2 for -m is in the 4 pi.
//  * self: -(((kappa * alpha) * (q_i q_i)) * (1 / sqrt pi)).  Background: -((((kappa * pi) * q_i) * Q) / ((2 (alpha alpha)) * V)),
//    Q = sum over the types a ascending of (double)n_a * charge[a], n_a the atoms of type a in the cell: a charged cell is served.
//  * per atom: components (real, reciprocal, self, background, short); energy = (((real + reciprocal) + self) + background) + short;
//    force = the real-space sum + the reciprocal sum.  Per cell: each component and the energy summed over its atoms in ascending
//    order, one running sum each.
//
// Orders of the sums.  The host statement adds the sites of an atom, and the vectors of an atom, in ascending order into one
// running sum.  The kernels give lane l of a wavefront the entries l, l + 64, .. in ascending order (one running sum a lane) and
// add the 64 lane sums by the butterfly wave_sum (offsets 32 .. 1): a fixed pattern that depends on the row alone.  S_m and the
// per-cell sums are ascending running sums on both sides.  erfc, exp, sin and cos are the platform's.  Host and device therefore
// agree bitwise on membership (sites, vectors: +, *, /, sqrt, floor of fp64 under -ffp-contract=off) and on values to rounding
// only: the situation of the SOAP descriptors and of S(q), not of q_l.
#pragma once
#include "../eval/sq_math.h"
#include "cell_soap_math.h"

namespace egnn {

constexpr int kEwaldWaves = 4;              // rows of a workgroup, one wavefront each
constexpr int kEwaldVectorBlock = kSqVectorBlock;   // vectors of one workgroup of the amplitude kernel, one per thread: the tiles of sq.hip
constexpr int kEwaldAtomChunk = 1024;       // atoms of a cell staged in LDS at a time (w and q: 32 KiB)
constexpr int kEwaldMaxPower = 64;          // n of D / r^n
constexpr int kEwaldComponents = 5;         // real, reciprocal, self, background, short
constexpr int kEwaldReal = 0, kEwaldRecip = 1, kEwaldSelf = 2, kEwaldBackground = 3, kEwaldShort = 4;
constexpr double kEwaldPi = 3.14159265358979323846;
constexpr double kEwaldFourPi = 12.566370614359172;          // 4 pi rounded to fp64
constexpr double kEwaldEightPi = 25.132741228718345;         // 8 pi
constexpr double kEwaldTwoOverSqrtPi = 1.1283791670955126;   // 2 / sqrt pi
constexpr double kEwaldOneOverSqrtPi = 0.5641895835477563;   // 1 / sqrt pi

// what one call computes with: passed to the kernels by value
struct EwaldModel {
  int A, n, has_potential, forces;
  double kappa, alpha, r_cut, short_cut, k_max;
  double charge[kCellMaxTypes];
  double pa[kCellMaxTypes * kCellMaxTypes], pb[kCellMaxTypes * kCellMaxTypes], pc[kCellMaxTypes * kCellMaxTypes],
      pd[kCellMaxTypes * kCellMaxTypes], u_cut[kCellMaxTypes * kCellMaxTypes];   // [type_i * A + type_j]
};

EGNN_HD double ewald_volume(const double* L) {
  const double* a = L;
  const double* b = L + 3;
  const double* c = L + 6;
  const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
  return fabs((a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2]);
}

// r^n, n >= 1, by binary powers: the squares r, r^2, r^4, .. and the product of those n selects, lowest first
EGNN_HD double ewald_ipow(double r, int n) {
  double p = 1.0, s = r;
  bool first = true;
  for (int e = n; e > 0; e >>= 1) {
    if (e & 1) { p = first ? s : p * s; first = false; }
    s = s * s;
  }
  return p;
}

// u_ab(r) and u'_ab(r) of pair ab
EGNN_HD void ewald_pair(const EwaldModel& P, int ab, double r2, double r, double* u, double* du) {
  const double ex = exp(-(P.pb[ab] * r)), r6 = (r2 * r2) * r2;
  double v = P.pa[ab] * ex - P.pc[ab] / r6, dv = (-(P.pa[ab] * P.pb[ab])) * ex + (6.0 * P.pc[ab]) / (r6 * r);
  if (P.pd[ab] != 0.0) {
    const double rn = ewald_ipow(r, P.n);
    v = v + P.pd[ab] / rn;
    dv = dv - ((double)P.n * P.pd[ab]) / (rn * r);
  }
  *u = v;
  *du = dv;
}

// the three terms of one site at r2 > 0: er (real energy), es (short energy), f (force factor: F += f * d)
EGNN_HD void ewald_site(const EwaldModel& P, int ti, int tj, double r2, double* er, double* es, double* f) {
  const double r = sqrt(r2), ar = P.alpha * r, ec = erfc(ar) / r, qj = P.charge[tj];
  *er = qj * ec;
  *es = 0.0;
  double fs = (-(P.kappa * P.charge[ti])) * ((qj * (ec + (kEwaldTwoOverSqrtPi * P.alpha) * exp(-(ar * ar)))) / r2);
  if (P.has_potential && r < P.short_cut) {
    const int ab = ti * P.A + tj;
    double u, du;
    ewald_pair(P, ab, r2, r, &u, &du);
    *es = u - P.u_cut[ab];
    fs = fs + du / r;
  }
  *f = fs;
}

EGNN_HD double ewald_real_energy(const EwaldModel& P, int ti, double sum) { return ((0.5 * P.kappa) * P.charge[ti]) * sum; }
EGNN_HD double ewald_short_energy(double sum) { return 0.5 * sum; }

EGNN_HD void ewald_kvec(int h, int k, int l, const double* Bm, double* kv) {
  for (int x = 0; x < 3; ++x) kv[x] = ((double)h * Bm[x] + (double)k * Bm[3 + x]) + (double)l * Bm[6 + x];
}
EGNN_HD double ewald_g(double k2, double alpha) { return exp(-(k2 / ((4.0 * alpha) * alpha))) / k2; }

// the energy and force terms of vector m at atom i: sn, cs of phi_im, (gc, gs) = g (S^c, S^s)
EGNN_HD double ewald_recip_energy_term(double sn, double cs, double gc, double gs) { return cs * gc + sn * gs; }
EGNN_HD double ewald_recip_force_term(double sn, double cs, double gc, double gs) { return sn * gc - cs * gs; }
EGNN_HD double ewald_recip_energy(const EwaldModel& P, double V, double qi, double sum) { return (((kEwaldFourPi * P.kappa) / V) * qi) * sum; }
EGNN_HD double ewald_recip_force(const EwaldModel& P, double V, double qi, double sum) { return (((kEwaldEightPi * P.kappa) / V) * qi) * sum; }

EGNN_HD double ewald_self(const EwaldModel& P, double qi) { return -(((P.kappa * P.alpha) * (qi * qi)) * kEwaldOneOverSqrtPi); }
EGNN_HD double ewald_background(const EwaldModel& P, double V, double qi, double Q) {
  return -((((P.kappa * kEwaldPi) * qi) * Q) / ((2.0 * (P.alpha * P.alpha)) * V));
}
// Q of a cell from its atoms per type
EGNN_HD double ewald_cell_charge(const EwaldModel& P, const int* n_type) {
  double Q = 0.0;
  for (int a = 0; a < P.A; ++a) Q += (double)n_type[a] * P.charge[a];
  return Q;
}
EGNN_HD double ewald_atom_energy(const double* comp) {
  return (((comp[kEwaldReal] + comp[kEwaldRecip]) + comp[kEwaldSelf]) + comp[kEwaldBackground]) + comp[kEwaldShort];
}

}  // namespace egnn

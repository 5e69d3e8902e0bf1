// Host side of the lattice-energy entries: the argument checks of the device entries (cell_ewald.hip) and the host statement
// egnn_cell_ewald_host -- the walk of the image box and of the index box, the Ewald sum and the pair potential computed on the CPU
// through cell_ewald_math.h, the text the kernels compile, every sum one ascending running sum.  No HIP call, no device code:
// checked (and run under the sanitizers) on a machine without a GPU.
#include <math.h>
#include <string.h>

#include "cell_ewald_host.h"

namespace egnn {

namespace {
bool positive_finite(double v) { return v > 0.0 && v < 1e300; }
}  // namespace

int cell_ewald_model_check(const char* who, int A, const double* charges, const double* pot, int n, int shift, double kappa, double alpha,
                           double r_cut, double short_cut, double k_max, int forces, EwaldModel* model) {
  if (int rc = atom_types_check(who, A, kCellMaxTypes)) return rc;
  if (!charges) { set_error("bad %s arguments (the host copy of the charges given)", who); return EGNN_EINVAL; }
  if (!positive_finite(kappa) || !positive_finite(alpha) || !positive_finite(r_cut) || !positive_finite(k_max)) {
    set_error("%s: kappa, alpha, r_cut and k_max must be positive and finite", who);
    return EGNN_EINVAL;
  }
  if (!positive_finite(short_cut) || short_cut > r_cut) {
    set_error("%s: short_cut %g (0 < short_cut <= r_cut = %g)", who, short_cut, r_cut);
    return EGNN_EINVAL;
  }
  if (n < 1 || n > kEwaldMaxPower) { set_error("%s: power n = %d of D / r^n (1 <= n <= %d)", who, n, kEwaldMaxPower); return EGNN_EINVAL; }
  EwaldModel& P = *model;
  memset(&P, 0, sizeof(P));
  P.A = A; P.n = n; P.has_potential = pot ? 1 : 0; P.forces = forces ? 1 : 0;
  P.kappa = kappa; P.alpha = alpha; P.r_cut = r_cut; P.short_cut = short_cut; P.k_max = k_max;
  for (int a = 0; a < A; ++a) {
    if (!(fabs(charges[a]) < 1e300)) { set_error("%s: the charge of type %d is not finite", who, a); return EGNN_EINVAL; }
    P.charge[a] = charges[a];
  }
  if (!pot) return EGNN_OK;
  const int AA = A * A;
  for (int a = 0; a < A; ++a)
    for (int b = 0; b < A; ++b) {
      const int ab = a * A + b, ba = b * A + a;
      for (int t = 0; t < 4; ++t) {
        if (!(fabs(pot[t * AA + ab]) < 1e300)) { set_error("%s: pair table %d is not finite at (%d, %d)", who, t, a, b); return EGNN_EINVAL; }
        if (pot[t * AA + ab] != pot[t * AA + ba]) { set_error("%s: pair table %d is not symmetric at (%d, %d)", who, t, a, b); return EGNN_EINVAL; }
      }
      P.pa[ab] = pot[ab]; P.pb[ab] = pot[AA + ab]; P.pc[ab] = pot[2 * AA + ab]; P.pd[ab] = pot[3 * AA + ab];
    }
  if (shift)
    for (int ab = 0; ab < AA; ++ab) {
      double du;
      ewald_pair(P, ab, short_cut * short_cut, short_cut, &P.u_cut[ab], &du);
    }
  return EGNN_OK;
}

int cell_ewald_batch_check(const char* who, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, double r_cut, double k_max) {
  if (int rc = cell_soap_batch_check(who, C, N, cell_ptr, lattice, r_cut)) return rc;
  return sq_cells_check(who, C, A, cell_ptr, lattice, k_max, nullptr);
}

int cell_ewald_vector_table(const char* who, int c, const EwaldModel& P, const double* L, const double* w, const int32_t* type, int na,
                            int64_t* n_vectors, Scratch<int32_t>* hkl_out, Scratch<double>* tab_out) {
  const bool charged = cell_ewald_charged(P);
  int64_t nv = 0;
  double Bm[9];
  int need[3];
  sq_reciprocal(L, Bm);
  sq_index_need(L, P.k_max, need);
  const int H = sq_index_box(need[0]), Kb = sq_index_box(need[1]), Lb = sq_index_box(need[2]);
  if (charged)
    for (int h = 0; h <= H; ++h)
      for (int k = -Kb; k <= Kb; ++k) nv += sq_row_vectors(h, k, Lb, Bm, P.k_max, [](int, int, double) {});
  if (nv > kSqMaxVectors) {
    set_error("%s: cell %d has %lld vectors below k_max (at most %d; lower k_max)", who, c, (long long)nv, kSqMaxVectors);
    return EGNN_EINVAL;
  }
  *n_vectors = nv;
  Scratch<int32_t>& hkl = *hkl_out;
  Scratch<double>& tab = *tab_out;
  if (!hkl.reset(3 * (size_t)nv) || !tab.reset(5 * (size_t)nv)) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
  if (charged) {
    size_t v = 0;
    for (int h = 0; h <= H; ++h)
      for (int k = -Kb; k <= Kb; ++k)
        sq_row_vectors(h, k, Lb, Bm, P.k_max, [&](int, int l, double k2) {
          double sc = 0.0, ss = 0.0;
          for (int j = 0; j < na; ++j) {
            double sn, cs;
            sq_phase_sincos(sq_phase(h, k, l, w + 3 * (size_t)j), &sn, &cs);
            const double qj = P.charge[type[j]];
            sc += qj * cs;
            ss += qj * sn;
          }
          const double g = ewald_g(k2, P.alpha);
          hkl[3 * v] = h; hkl[3 * v + 1] = k; hkl[3 * v + 2] = l;
          ewald_kvec(h, k, l, Bm, tab.p + 5 * v);
          tab[5 * v + 3] = g * sc;
          tab[5 * v + 4] = g * ss;
          ++v;
        });
  }
  return EGNN_OK;
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_ewald_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type,
                         const double* charges, const double* pot, int n, int shift, double kappa, double alpha, double r_cut, double short_cut,
                         double k_max, int forces, double* energy, double* components, double* energy_per_atom, double* atom_components,
                         double* force, int32_t* n_sites, int64_t* n_vectors, int32_t* coincident) {
  const char* who = "egnn_cell_ewald_host";
  if (C < 1 || !cell_ptr || !energy || !components || !energy_per_atom || !n_vectors || !coincident || (forces && !force)) {
    set_error("bad %s arguments (C >= 1; cell_ptr, energy, components, energy_per_atom, n_vectors and coincident given; force with forces)", who);
    return EGNN_EINVAL;
  }
  EwaldModel P;
  if (int rc = cell_ewald_model_check(who, A, charges, pot, n, shift, kappa, alpha, r_cut, short_cut, k_max, forces, &P)) return rc;
  const int N = cell_ptr[C];
  if (int rc = cell_ewald_batch_check(who, C, N, A, cell_ptr, lattice, r_cut, k_max)) return rc;
  if (N > 0 && (!frac || !type)) { set_error("bad %s arguments (frac and type given)", who); return EGNN_EINVAL; }
  if (int rc = cell_inputs_check(who, N, frac, type, A, 0, nullptr)) return rc;
  const double cut2 = r_cut * r_cut;
  for (int c = 0; c < C; ++c) {
    const int lo = cell_ptr[c], hi = cell_ptr[c + 1], na = hi - lo;
    const double* L = lattice + 9 * (size_t)c;
    const double V = ewald_volume(L);
    Scratch<double> w(3 * (size_t)na);
    if (!w.p) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
    for (int t = 0; t < 3 * na; ++t) w[t] = cell_wrap(frac[3 * (size_t)lo + t]);
    int n_type[kCellMaxTypes] = {0, 0, 0, 0};
    for (int i = lo; i < hi; ++i) ++n_type[type[i]];
    const double Q = ewald_cell_charge(P, n_type);
    // the vectors of the cell and their amplitudes
    int64_t nv = 0;
    Scratch<int32_t> hkl(0);
    Scratch<double> tab(0);
    if (int rc = cell_ewald_vector_table(who, c, P, L, w.p, type + lo, na, &nv, &hkl, &tab)) return rc;
    n_vectors[c] = nv;
    int box[3];
    double width[3];
    cell_soap_box(L, r_cut, box, width);
    const int nbox = cell_soap_box_count(box);
    double cell_sum[kEwaldComponents + 1] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    coincident[c] = 0;
    for (int i = lo; i < hi; ++i) {
      const double* wi = w.p + 3 * (size_t)(i - lo);
      const int ti = type[i];
      const double qi = P.charge[ti];
      double er = 0.0, es = 0.0, F[3] = {0.0, 0.0, 0.0};
      int sites = 0;
      for (int j = lo; j < hi; ++j) {
        const double* wj = w.p + 3 * (size_t)(j - lo);
        for (int t = 0; t < nbox; ++t) {
          int s[3];
          double d[3];
          cell_soap_box_shift(t, box, s);
          if (j == i && s[0] == 0 && s[1] == 0 && s[2] == 0) continue;
          if (!cell_soap_site(wj, wi, s, L, cut2, d)) continue;
          ++sites;
          const double r2 = cell_norm2(d);
          if (r2 == 0.0) { coincident[c] = 1; continue; }
          double a, b, f;
          ewald_site(P, ti, type[j], r2, &a, &b, &f);
          er += a;
          es += b;
          if (forces)
            for (int x = 0; x < 3; ++x) F[x] += f * d[x];
        }
      }
      double rec = 0.0, R[3] = {0.0, 0.0, 0.0};
      for (int64_t v = 0; v < nv; ++v) {
        double sn, cs;
        sq_phase_sincos(sq_phase(hkl[3 * v], hkl[3 * v + 1], hkl[3 * v + 2], wi), &sn, &cs);
        const double* tv = tab.p + 5 * v;
        rec += ewald_recip_energy_term(sn, cs, tv[3], tv[4]);
        if (forces) {
          const double ft = ewald_recip_force_term(sn, cs, tv[3], tv[4]);
          for (int x = 0; x < 3; ++x) R[x] += tv[x] * ft;
        }
      }
      double comp[kEwaldComponents];
      comp[kEwaldReal] = ewald_real_energy(P, ti, er);
      comp[kEwaldRecip] = ewald_recip_energy(P, V, qi, rec);
      comp[kEwaldSelf] = ewald_self(P, qi);
      comp[kEwaldBackground] = ewald_background(P, V, qi, Q);
      comp[kEwaldShort] = ewald_short_energy(es);
      const double e = ewald_atom_energy(comp);
      energy_per_atom[i] = e;
      for (int k = 0; k < kEwaldComponents; ++k) {
        if (atom_components) atom_components[(size_t)i * kEwaldComponents + k] = comp[k];
        cell_sum[k] += comp[k];
      }
      cell_sum[kEwaldComponents] += e;
      if (forces)
        for (int x = 0; x < 3; ++x) force[3 * (size_t)i + x] = F[x] + ewald_recip_force(P, V, qi, R[x]);
      if (n_sites) n_sites[i] = sites;
    }
    for (int k = 0; k < kEwaldComponents; ++k) components[(size_t)c * kEwaldComponents + k] = cell_sum[k];
    energy[c] = cell_sum[kEwaldComponents];
  }
  return EGNN_OK;
}

}  // extern "C"

// Host statement of the strain derivative of the lattice energy, egnn_cell_ewald_virial_host: the walk of the image box and of the
// vector table of egnn_cell_ewald_host, the virial terms computed on the CPU through cell_stress_math.h, the text the kernels
// compile, every sum one ascending running sum.  No HIP call, no device code: checked (and run under the sanitizers) on a machine
// without a GPU.
#include <math.h>

#include "cell_ewald_host.h"
#include "cell_stress_math.h"

using namespace egnn;

extern "C" {

int egnn_cell_ewald_virial_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type,
                                const double* charges, const double* pot, int n, int shift, double kappa, double alpha, double r_cut,
                                double short_cut, double k_max, double* strain, double* components, double* per_atom, double* atom_components,
                                double* stress, double* pressure, int64_t* n_vectors, int32_t* coincident) {
  const char* who = "egnn_cell_ewald_virial_host";
  if (C < 1 || !cell_ptr || !strain || !components || !per_atom || !stress || !pressure || !n_vectors || !coincident) {
    set_error("bad %s arguments (C >= 1; cell_ptr, strain, components, per_atom, stress, pressure, n_vectors and coincident given)", who);
    return EGNN_EINVAL;
  }
  EwaldModel P;
  if (int rc = cell_ewald_model_check(who, A, charges, pot, n, shift, kappa, alpha, r_cut, short_cut, k_max, 0, &P)) return rc;
  const int N = cell_ptr[C];
  if (int rc = cell_ewald_batch_check(who, C, N, A, cell_ptr, lattice, r_cut, k_max)) return rc;
  if (N > 0 && (!frac || !type)) { set_error("bad %s arguments (frac and type given)", who); return EGNN_EINVAL; }
  if (int rc = cell_inputs_check(who, N, frac, type, A, 0, nullptr)) return rc;
  constexpr int kParts = kEwaldComponents * kVoigt;
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
    int64_t nv = 0;
    Scratch<int32_t> hkl(0);
    Scratch<double> tab(0);
    if (int rc = cell_ewald_vector_table(who, c, P, L, w.p, type + lo, na, &nv, &hkl, &tab)) return rc;
    n_vectors[c] = nv;
    int box[3];
    double width[3];
    cell_soap_box(L, r_cut, box, width);
    const int nbox = cell_soap_box_count(box);
    double cell_sum[kParts + kVoigt];
    for (int t = 0; t < kParts + kVoigt; ++t) cell_sum[t] = 0.0;
    coincident[c] = 0;
    for (int i = lo; i < hi; ++i) {
      const double* wi = w.p + 3 * (size_t)(i - lo);
      const int ti = type[i];
      const double qi = P.charge[ti];
      double site[2 * kVoigt], rec[kVoigt];
      for (int v = 0; v < 2 * kVoigt; ++v) site[v] = 0.0;
      for (int v = 0; v < kVoigt; ++v) rec[v] = 0.0;
      for (int j = lo; j < hi; ++j) {
        const double* wj = w.p + 3 * (size_t)(j - lo);
        for (int t = 0; t < nbox; ++t) {
          int s[3];
          double d[3];
          cell_soap_box_shift(t, box, s);
          if (j == i && s[0] == 0 && s[1] == 0 && s[2] == 0) continue;
          if (!cell_soap_site(wj, wi, s, L, cut2, d)) continue;
          const double r2 = cell_norm2(d);
          if (r2 == 0.0) { coincident[c] = 1; continue; }
          double fr, fs;
          ewald_site_factors(P, ti, type[j], r2, &fr, &fs);
          ewald_virial_add(fr, fs, d, site);
        }
      }
      for (int64_t v = 0; v < nv; ++v) {
        double sn, cs, B[kVoigt];
        sq_phase_sincos(sq_phase(hkl[3 * v], hkl[3 * v + 1], hkl[3 * v + 2], wi), &sn, &cs);
        const double* tv = tab.p + 5 * v;
        const double term = ewald_recip_energy_term(sn, cs, tv[3], tv[4]);
        ewald_recip_B(tv, P.alpha, B);
        for (int x = 0; x < kVoigt; ++x) rec[x] += term * B[x];
      }
      const double e_bg = ewald_background(P, V, qi, Q);
      for (int v = 0; v < kVoigt; ++v) {
        double comp[kEwaldComponents];
        comp[kEwaldReal] = ewald_virial_site_sum(site[v]);
        comp[kEwaldRecip] = ewald_recip_energy(P, V, qi, rec[v]);
        comp[kEwaldSelf] = 0.0;
        comp[kEwaldBackground] = ewald_virial_background(e_bg, v);
        comp[kEwaldShort] = ewald_virial_site_sum(site[kVoigt + v]);
        const double d_v = ewald_atom_energy(comp);
        per_atom[(size_t)i * kVoigt + v] = d_v;
        for (int k = 0; k < kEwaldComponents; ++k) {
          if (atom_components) atom_components[((size_t)i * kEwaldComponents + k) * kVoigt + v] = comp[k];
          cell_sum[k * kVoigt + v] += comp[k];
        }
        cell_sum[kParts + v] += d_v;
      }
    }
    for (int t = 0; t < kParts; ++t) components[(size_t)c * kParts + t] = cell_sum[t];
    for (int v = 0; v < kVoigt; ++v) {
      strain[(size_t)c * kVoigt + v] = cell_sum[kParts + v];
      stress[(size_t)c * kVoigt + v] = cell_sum[kParts + v] / V;
    }
    pressure[c] = ewald_pressure(stress + (size_t)c * kVoigt);
  }
  return EGNN_OK;
}

}  // extern "C"

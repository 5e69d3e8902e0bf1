// Host side of the relaxation entries: the argument checks of the device entries (cell_relax.hip) and the host statements
// egnn_cell_relax_step_host (the step alone) and egnn_cell_relax_host (the whole loop: held lists, freeze rule and rebuilds, the
// evaluation through cell_ewald_math.h over a held row, every sum of an evaluation one ascending running sum).  The definitions and
// the order of every sum: cell_relax_math.h, the text the kernels compile.  No HIP call, no device code: checked (and run under the
// sanitizers) on a machine without a GPU.
#include <math.h>
#include <string.h>

#include "cell_relax_host.h"

namespace egnn {

namespace {

bool positive_finite(double v) { return v > 0.0 && v < 1e300; }

// the held rows of a cell: the sites of every atom inside list_cut on the wrapped reference coordinates w, ascending (atom, code)
struct HeldList {
  Scratch<int32_t> row_ptr, atom, code;
  HeldList() : row_ptr(0), atom(0), code(0) {}
};

int held_build(const char* who, const double* L, const double* w, int lo, int na, double list_cut, HeldList* H) {
  int box[3];
  double width[3];
  cell_soap_box(L, list_cut, box, width);
  const int nbox = cell_soap_box_count(box);
  const double cut2 = list_cut * list_cut;
  if (!H->row_ptr.reset((size_t)na + 1)) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
  for (int pass = 0; pass < 2; ++pass) {
    int64_t total = 0;
    for (int i = 0; i < na; ++i) {
      H->row_ptr[i] = (int32_t)total;
      for (int j = 0; j < na; ++j)
        for (int t = 0; t < nbox; ++t) {
          int s[3];
          double d[3];
          cell_soap_box_shift(t, box, s);
          if (j == i && s[0] == 0 && s[1] == 0 && s[2] == 0) continue;
          if (!cell_soap_site(w + 3 * (size_t)j, w + 3 * (size_t)i, s, L, cut2, d)) continue;
          if (pass) {
            H->atom[total] = lo + j;
            H->code[total] = cell_shift_code(s[0], s[1], s[2]);
          }
          ++total;
        }
    }
    if (total > 0x7fffffff) { set_error("%s: more than 2^31 - 1 held sites in one cell", who); return EGNN_EINVAL; }
    H->row_ptr[na] = (int32_t)total;
    if (!pass && (!H->atom.reset((size_t)total) || !H->code.reset((size_t)total))) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
  }
  return EGNN_OK;
}

// one evaluation of cell c at the unwrapped coordinates u (whole batch array) over its held rows: force (whole batch array) and the
// cell's energy; the statement of egnn_cell_ewald_host with the real part read from the held row
int held_evaluate(const char* who, int c, const EwaldModel& P, const double* L, const double* u, const int32_t* type, int lo, int na,
                  const HeldList& H, double* force, double* energy, bool* coincident) {
  const double V = ewald_volume(L), cut2 = P.r_cut * P.r_cut;
  Scratch<double> w(3 * (size_t)na);
  if (!w.p) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
  for (int t = 0; t < 3 * na; ++t) w[t] = cell_wrap(u[3 * (size_t)lo + t]);
  int n_type[kCellMaxTypes] = {0, 0, 0, 0};
  for (int i = lo; i < lo + na; ++i) ++n_type[type[i]];
  const double Q = ewald_cell_charge(P, n_type);
  int64_t nv = 0;
  Scratch<int32_t> hkl(0);
  Scratch<double> tab(0);
  if (int rc = cell_ewald_vector_table(who, c, P, L, w.p, type + lo, na, &nv, &hkl, &tab)) return rc;
  double total = 0.0;
  *coincident = false;
  for (int i = lo; i < lo + na; ++i) {
    const double* ui = u + 3 * (size_t)i;
    const double* wi = w.p + 3 * (size_t)(i - lo);
    const int ti = type[i];
    const double qi = P.charge[ti];
    double er = 0.0, es = 0.0, F[3] = {0.0, 0.0, 0.0};
    for (int e = H.row_ptr.p[i - lo]; e < H.row_ptr.p[i - lo + 1]; ++e) {
      double d[3];
      if (!relax_held_site(u, L, lo, lo + na, ui, H.atom.p[e], H.code.p[e], cut2, d)) continue;
      const double r2 = cell_norm2(d);
      if (r2 == 0.0) { *coincident = true; continue; }
      double a, b, f;
      ewald_site(P, ti, type[H.atom.p[e]], r2, &a, &b, &f);
      er += a;
      es += b;
      for (int x = 0; x < 3; ++x) F[x] += f * d[x];
    }
    double rec = 0.0, R[3] = {0.0, 0.0, 0.0};
    for (int64_t v = 0; v < nv; ++v) {
      double sn, cs;
      sq_phase_sincos(sq_phase(hkl[3 * v], hkl[3 * v + 1], hkl[3 * v + 2], wi), &sn, &cs);
      const double* tv = tab.p + 5 * v;
      rec += ewald_recip_energy_term(sn, cs, tv[3], tv[4]);
      const double ft = ewald_recip_force_term(sn, cs, tv[3], tv[4]);
      for (int x = 0; x < 3; ++x) R[x] += tv[x] * ft;
    }
    double comp[kEwaldComponents];
    comp[kEwaldReal] = ewald_real_energy(P, ti, er);
    comp[kEwaldRecip] = ewald_recip_energy(P, V, qi, rec);
    comp[kEwaldSelf] = ewald_self(P, qi);
    comp[kEwaldBackground] = ewald_background(P, V, qi, Q);
    comp[kEwaldShort] = ewald_short_energy(es);
    total += ewald_atom_energy(comp);
    for (int x = 0; x < 3; ++x) force[3 * (size_t)i + x] = F[x] + ewald_recip_force(P, V, qi, R[x]);
  }
  *energy = total;
  return EGNN_OK;
}

}  // namespace

int cell_relax_fire_check(const char* who, double dt_max, int n_min, double f_inc, double f_dec, double a_start, double f_a, double max_step,
                          double f_max, int max_steps, double skin, FireModel* model) {
  if (!positive_finite(dt_max) || !positive_finite(f_inc) || !positive_finite(f_dec) || !positive_finite(a_start) || !positive_finite(f_a) ||
      f_inc < 1.0 || f_dec >= 1.0 || a_start > 1.0 || f_a > 1.0 || n_min < 0) {
    set_error("%s: FIRE needs dt_max > 0, f_inc >= 1, 0 < f_dec < 1, 0 < a_start <= 1, 0 < f_a <= 1 and n_min >= 0", who);
    return EGNN_EINVAL;
  }
  if (!positive_finite(f_max)) { set_error("%s: f_max = %g must be positive and finite", who, f_max); return EGNN_EINVAL; }
  if (max_steps < 0) { set_error("%s: max_steps = %d must not be negative", who, max_steps); return EGNN_EINVAL; }
  if (!positive_finite(skin)) { set_error("%s: skin = %g must be positive and finite", who, skin); return EGNN_EINVAL; }
  if (!positive_finite(max_step) || max_step > 0.5 * skin) {
    set_error("%s: max_step = %g must be positive and at most skin / 2 = %g (skin = %g)", who, max_step, 0.5 * skin, skin);
    return EGNN_EINVAL;
  }
  FireModel& M = *model;
  M.dt_max = dt_max; M.f_inc = f_inc; M.f_dec = f_dec; M.a_start = a_start; M.f_a = f_a; M.max_step = max_step; M.f_max = f_max; M.skin = skin;
  M.n_min = n_min; M.max_steps = max_steps;
  return EGNN_OK;
}

int cell_relax_batch_check(const char* who, int C, int N, const int32_t* cell_ptr, const double* lattice) {
  if (C < 1 || C > 65535 || N < 0 || !cell_ptr || !lattice) {
    set_error("bad %s arguments (1 <= C <= 65535 cells; N >= 0; the host copies of cell_ptr and the lattices given)", who);
    return EGNN_EINVAL;
  }
  if (cell_ptr[0] != 0 || cell_ptr[C] != N) { set_error("%s: the host copy of cell_ptr must run from 0 to N = %d", who, N); return EGNN_EINVAL; }
  for (int c = 0; c < C; ++c) {
    if (int rc = ptr_step_check(who, "cell_ptr", "cell", cell_ptr, c, kCellMaxAtoms)) return rc;
    double w[3];
    if (!cell_widths(lattice + 9 * (size_t)c, w)) { set_error("%s: cell %d has a singular lattice", who, c); return EGNN_EINVAL; }
  }
  return EGNN_OK;
}

void cell_relax_step_cell(const FireModel& M, int c, int C, const int32_t* cell_ptr, const double* lattice, const double* force, double energy,
                          bool coincident, double* frac, double* velocity, double* since, double* moved, double* scalars, int32_t* counters,
                          int32_t* done, int32_t* rebuild, double* energy_trace, double* force_trace) {
  if (done[c] || rebuild[c]) return;
  const int lo = cell_ptr[c], n = cell_ptr[c + 1] - lo;
  double* sc = scalars + (size_t)c * kRelaxScalars;
  int32_t* ct = counters + (size_t)c * kRelaxCounters;
  if (coincident) { ct[kRelaxStatus] = kRelaxCoincident; done[c] = 1; return; }
  const double* F = force + 3 * (size_t)lo;
  double* u = frac + 3 * (size_t)lo;
  double* v = velocity + 3 * (size_t)lo;
  double* s = since + 3 * (size_t)lo;
  double* mv = moved + 3 * (size_t)lo;
  double part[4][kRelaxThreads], sums[4];
  for (int t = 0; t < kRelaxThreads; ++t) {
    double four[4];
    relax_thread_sums(t, n, F, v, four);
    for (int k = 0; k < 4; ++k) part[k][t] = four[k];
  }
  for (int k = 0; k < 4; ++k) sums[k] = relax_tree_host(part[k], k == 3);
  const int steps = ct[kRelaxSteps];
  const RelaxPlan R = relax_plan(M, sc[kRelaxDt], sc[kRelaxA], ct[kRelaxNPos], steps, sums);
  if (R.status == kRelaxNotFinite) { ct[kRelaxStatus] = R.status; done[c] = 1; return; }
  const double fm = sqrt(sums[3]);
  sc[kRelaxEnergy] = energy;
  sc[kRelaxMaxForce] = fm;
  if (steps == 0) sc[kRelaxInitial] = energy;
  if (energy_trace && relax_in_trace(M, steps)) energy_trace[(size_t)steps * C + c] = energy;
  if (force_trace && relax_in_trace(M, steps)) force_trace[(size_t)steps * C + c] = fm;
  if (R.status != kRelaxRunning) { ct[kRelaxStatus] = R.status; done[c] = 1; return; }
  for (int t = 0; t < kRelaxThreads; ++t) part[0][t] = relax_thread_move(t, n, R, F, v);
  const double scale = relax_cap(M, relax_tree_host(part[0], true));
  for (int t = 0; t < kRelaxThreads; ++t) {
    double two[2];
    relax_thread_reach(t, n, R, scale, F, v, s, two);
    part[0][t] = two[0];
    part[1][t] = two[1];
  }
  const double reach2 = relax_tree_host(part[0], true), held2 = relax_tree_host(part[1], true);
  if (relax_frozen(M, reach2, held2)) {
    if (relax_stuck(ct[kRelaxFrozen], steps)) { ct[kRelaxStatus] = kRelaxStuck; done[c] = 1; return; }
    ct[kRelaxFrozen] = steps + 1;
    rebuild[c] = 1;
    return;
  }
  double K[9];
  relax_inverse(lattice + 9 * (size_t)c, K);
  for (int t = 0; t < kRelaxThreads; ++t) relax_thread_commit(t, n, R, scale, K, F, u, v, s, mv);
  sc[kRelaxDt] = R.dt;
  sc[kRelaxA] = R.a;
  ct[kRelaxNPos] = R.n_pos;
  ct[kRelaxSteps] = steps + 1;
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_relax_step_host(int C, int N, const int32_t* cell_ptr, const double* lattice, const double* force, const double* energy,
                              const int32_t* coincident, double dt_max, int n_min, double f_inc, double f_dec, double a_start, double f_a,
                              double max_step, double f_max, int max_steps, double skin, double* frac, double* velocity, double* since,
                              double* moved, double* scalars, int32_t* counters, int32_t* done, int32_t* rebuild, double* energy_trace,
                              double* force_trace) {
  const char* who = "egnn_cell_relax_step_host";
  FireModel M;
  if (int rc = cell_relax_fire_check(who, dt_max, n_min, f_inc, f_dec, a_start, f_a, max_step, f_max, max_steps, skin, &M)) return rc;
  if (int rc = cell_relax_batch_check(who, C, N, cell_ptr, lattice)) return rc;
  if (!energy || !coincident || !scalars || !counters || !done || !rebuild || (N > 0 && (!force || !frac || !velocity || !since || !moved))) {
    set_error("bad %s arguments (force, energy, coincident, the state arrays, the counters and the two flag arrays given)", who);
    return EGNN_EINVAL;
  }
  for (int c = 0; c < C; ++c)
    cell_relax_step_cell(M, c, C, cell_ptr, lattice, force, energy[c], coincident[c] != 0, frac, velocity, since, moved, scalars, counters, done,
                         rebuild, energy_trace, force_trace);
  return EGNN_OK;
}

int egnn_cell_relax_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type,
                         const double* charges, const double* pot, int n, int shift, double kappa, double alpha, double r_cut, double short_cut,
                         double k_max, double dt, double dt_max, int n_min, double f_inc, double f_dec, double a_start, double f_a, double max_step,
                         double f_max, int max_steps, double skin, double* frac_out, double* energy, double* initial_energy, double* force,
                         double* max_force, int32_t* steps, int32_t* status, double* moved, int32_t* n_rebuilds, double* energy_trace,
                         double* force_trace, double* frac_trace) {
  const char* who = "egnn_cell_relax_host";
  if (C < 1 || !cell_ptr || !energy || !initial_energy || !max_force || !steps || !status || !n_rebuilds) {
    set_error("bad %s arguments (C >= 1; cell_ptr, energy, initial_energy, max_force, steps, status and n_rebuilds given)", who);
    return EGNN_EINVAL;
  }
  EwaldModel P;
  if (int rc = cell_ewald_model_check(who, A, charges, pot, n, shift, kappa, alpha, r_cut, short_cut, k_max, 1, &P)) return rc;
  FireModel M;
  if (int rc = cell_relax_fire_check(who, dt_max, n_min, f_inc, f_dec, a_start, f_a, max_step, f_max, max_steps, skin, &M)) return rc;
  if (!positive_finite(dt)) { set_error("%s: dt = %g must be positive and finite", who, dt); return EGNN_EINVAL; }
  const int N = cell_ptr[C];
  if (int rc = cell_ewald_batch_check(who, C, N, A, cell_ptr, lattice, r_cut, k_max)) return rc;
  if (int rc = cell_soap_batch_check(who, C, N, cell_ptr, lattice, r_cut + skin)) return rc;   // the held lists: the image box of r_cut + skin
  if (N > 0 && (!frac || !type || !frac_out || !force || !moved)) {
    set_error("bad %s arguments (frac, type, frac_out, force and moved given)", who);
    return EGNN_EINVAL;
  }
  if (int rc = cell_inputs_check(who, N, frac, type, A, 0, nullptr)) return rc;
  Scratch<double> velocity(3 * (size_t)N), since(3 * (size_t)N), scalars((size_t)C * kRelaxScalars), cell_energy((size_t)C);
  Scratch<int32_t> counters((size_t)C * kRelaxCounters), done((size_t)C), rebuild((size_t)C);
  if (!velocity.p || !since.p || !scalars.p || !cell_energy.p || !counters.p || !done.p || !rebuild.p) {
    set_error("%s: out of memory", who);
    return EGNN_ENOMEM;
  }
  const size_t rows = (size_t)max_steps + 1;
  const double nan = NAN;
  if (energy_trace) for (size_t t = 0; t < rows * C; ++t) energy_trace[t] = nan;
  if (force_trace) for (size_t t = 0; t < rows * C; ++t) force_trace[t] = nan;
  if (frac_trace) for (size_t t = 0; t < rows * 3 * (size_t)N; ++t) frac_trace[t] = nan;
  for (size_t t = 0; t < 3 * (size_t)N; ++t) { frac_out[t] = frac[t]; moved[t] = 0.0; force[t] = 0.0; }
  for (int c = 0; c < C; ++c) {
    const int lo = cell_ptr[c], na = cell_ptr[c + 1] - lo;
    const double* L = lattice + 9 * (size_t)c;
    scalars[(size_t)c * kRelaxScalars + kRelaxDt] = dt;
    scalars[(size_t)c * kRelaxScalars + kRelaxA] = a_start;
    n_rebuilds[c] = 0;
    HeldList H;
    Scratch<double> ref(3 * (size_t)na);
    if (!ref.p) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
    bool first = true;
    rebuild[c] = 1;
    while (!done[c]) {
      if (rebuild[c]) {   // u <- wrap(u): the reference of the new list
        for (int t = 0; t < 3 * na; ++t) {
          ref[t] = frac_out[3 * (size_t)lo + t] = cell_wrap(frac_out[3 * (size_t)lo + t]);
          since[3 * (size_t)lo + t] = 0.0;
        }
        if (int rc = held_build(who, L, ref.p, lo, na, r_cut + skin, &H)) return rc;
        rebuild[c] = 0;
        if (!first) ++n_rebuilds[c];
        first = false;
      }
      bool coincident = false;
      if (int rc = held_evaluate(who, c, P, L, frac_out, type, lo, na, H, force, &cell_energy[c], &coincident)) return rc;
      if (frac_trace && relax_in_trace(M, counters[(size_t)c * kRelaxCounters + kRelaxSteps]))
        memcpy(frac_trace + ((size_t)counters[(size_t)c * kRelaxCounters + kRelaxSteps] * N + lo) * 3, frac_out + 3 * (size_t)lo,
                             sizeof(double) * 3 * (size_t)na);
      cell_relax_step_cell(M, c, C, cell_ptr, lattice, force, cell_energy[c], coincident, frac_out, velocity.p, since.p, moved, scalars.p,
                           counters.p, done.p, rebuild.p, energy_trace, force_trace);
    }
    energy[c] = scalars[(size_t)c * kRelaxScalars + kRelaxEnergy];
    initial_energy[c] = scalars[(size_t)c * kRelaxScalars + kRelaxInitial];
    max_force[c] = scalars[(size_t)c * kRelaxScalars + kRelaxMaxForce];
    steps[c] = counters[(size_t)c * kRelaxCounters + kRelaxSteps];
    status[c] = counters[(size_t)c * kRelaxCounters + kRelaxStatus];
  }
  return EGNN_OK;
}

}  // extern "C"

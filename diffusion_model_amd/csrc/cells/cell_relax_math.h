// Definitions of the relaxation of periodic cells (cell_relax.hip, cell_relax_host.cpp): the FIRE minimiser (Bitzek et al., Phys.
// Rev. Lett. 97, 170201 (2006)) over the lattice energy of cell_ewald_math.h, the atoms moving in a fixed cell, the real-space sites
// read from lists that are held over many evaluations.  Plain C++ behind the host/device macro, so that the kernels and the host
// statement compile the same text.  An extension: no file of the reference relaxes a structure.  The parameters of FIRE are stated
// from the publication, not pinned by execution.
//
// State of a cell, independent of every other cell of a batch: u [n, 3] unwrapped fractional coordinates; v [n, 3] velocities (unit
// mass 1); since [n, 3] the Cartesian move of every atom since the cell's list was built; moved [n, 3] its net move since the start
// (never folded into the cell); dt, a, n_pos, steps, frozen; status (kRelaxRunning .. kRelaxStuck); the flags done and rebuild.
//
//  * held list: the rows of egnn_cell_sites_* at cut = r_cut + skin on the REFERENCE coordinates, the wrapped u at the moment of the
//    build (ascending (atom, shift code), (i, 0) left out).  An evaluation reads site (j, s) of centre i at d = cell_site_vector(u_j,
//    u_i, s, L) on the UNWRAPPED u, in exactly the operation order of the search, and keeps it iff cell_norm2(d) < r_cut * r_cut
//    (relax_held_site): the expression of cell_soap_site.  At the moment of a build u is the reference, so the kept sites are those
//    of egnn_cell_sites_* at cut = r_cut, bit for bit and in the same order.  After the test the terms are ewald_site, unchanged.  A
//    site at r2 == 0 contributes nothing and flags its cell.
//  * completeness: a site inside r_cut now was inside r_cut + |since_i| + |since_j| at the build; the freeze rule keeps every
//    |since| <= skin / 2, so the held row misses none.  With max_step == skin / 2 the first capped move after a build may exceed
//    skin / 2 by the rounding of the cap (a few ulp of max_step); it is made all the same (step 6), so the bound on |since| holds to
//    that rounding, which is also the rounding of the distances the argument compares.
//  * evaluation: the real part per atom over its held row; amplitudes, reciprocal part, self, background and the finish by the text
//    of cell_ewald_math.h on cell_wrap(u) (the lattice-energy kernels, unchanged: they wrap on read).  F [n, 3], E of the cell.
//  * step of a cell at an evaluation (F, E), in this order:
//      0. done or rebuild set: nothing changes.  A coincident site: status = coincident, done.
//      1. sums: P = sum_i dot(F_i, v_i), FF = sum_i dot(F_i, F_i), vv = sum_i dot(v_i, v_i), fm2 = max_i dot(F_i, F_i);
//         dot(a, b) = (a_0 b_0 + a_1 b_1) + a_2 b_2.  FF not finite: status = not finite, done.
//      2. records: energy = E, max_force = sqrt(fm2); at steps == 0 initial_energy = E; trace row `steps` = (E, sqrt(fm2)).
//      3. fm2 < f_max * f_max: status = converged, done.  Else steps == max_steps: status = step limit, done.
//      4. FIRE (relax_plan).  P > 0: c = (a * sqrt(vv)) / sqrt(FF), v' = (1 - a) * v + c * F; if n_pos > n_min: dt' = min(dt * f_inc,
//         dt_max), a' = a * f_a; n_pos' = n_pos + 1.  Else v' = 0, a' = a_start, dt' = dt * f_dec, n_pos' = 0.
//         Then v'' = v' + dt' * F (for P <= 0 exactly dt' * F) and dr = dt' * v'' (relax_velocity).
//      5. cap: m2 = max_i dot(dr_i, dr_i), m = sqrt(m2); scale = max_step / m where m > max_step, else 1; dr_i = scale * dr_i: one
//         factor per cell that bounds the move of every ATOM, not the norm of the whole vector.
//      6. freeze: reach2 = max_i |since_i + dr_i|^2, held2 = max_i |since_i|^2; where sqrt(reach2) > skin / 2 AND held2 > 0 the cell
//         sets rebuild and NOTHING else changes (v, dt, a, n_pos, steps, u): it repeats this evaluation until its list has been
//         rebuilt.  A cell whose list has just been built (since == 0 exactly, held2 == 0) always moves: its move is capped at
//         max_step <= skin / 2, and a capped move that rounds to a few ulp above skin / 2 must not freeze it again -- the rebuild
//         would change nothing and the cell would ask for ever.  As a guard the counter `frozen` holds steps + 1 of the last freeze:
//         a cell that freezes twice at the same step count has not moved in between; status = stuck, done.
//      7. commit: v = v'', dt = dt', a = a', n_pos = n_pos', u_i += dr_i L^-1 (relax_to_fractional), since_i += dr_i,
//         moved_i += dr_i, steps += 1.
//  * rebuild of a cell (the caller's): u <- cell_wrap(u), reference <- u, since <- 0, its rows searched again, rebuild cleared.
//    v, dt, a, n_pos, steps and moved stay.  A cell that did not ask keeps its reference and therefore its rows bit for bit.
//
// Orders of the sums.  Real part of an atom: the host statement adds the kept sites of the held row in ascending order into one
// running sum; the kernel gives lane l the entries l, l + 64, .. and adds the 64 lane sums by the butterfly wave_sum, as
// cell_ewald_real_kernel.  Everything else of an evaluation: cell_ewald_math.h.  The three sums of the step (P, FF, vv) run in ONE
// order on host and device, which depends on the atom count n of the cell alone: partial t of kRelaxThreads = 256 adds the atoms t,
// t + 256, .. in ascending order into one running sum from 0 (relax_thread_sums), then the tree s[t] += s[t + off], off = 128, 64,
// .. 1, t < off (relax_tree_host; the kernel runs the same tree in LDS).  The maxima (fm2, m2, reach2, held2) go through the same
// partials and tree with max in place of +: a maximum does not depend on its order.  sqrt, +, *, / of fp64 under -ffp-contract=off: the step
// is bitwise the same on host and device; the forces agree to rounding (erfc, exp, sin and cos are the platform's).
#pragma once
#include "cell_ewald_math.h"

namespace egnn {

constexpr int kRelaxThreads = 256;   // partial sums of a cell's reductions: the threads of the step kernel's workgroup
constexpr int kRelaxRunning = 0, kRelaxConverged = 1, kRelaxStepLimit = 2, kRelaxCoincident = 3, kRelaxNotFinite = 4;   // status
constexpr int kRelaxStuck = 5;       // status: froze twice without a move in between (the guard of step 6)
constexpr int kRelaxScalars = 5;     // scalars [C, 5]: dt, a, energy, initial energy, max force
constexpr int kRelaxDt = 0, kRelaxA = 1, kRelaxEnergy = 2, kRelaxInitial = 3, kRelaxMaxForce = 4;
constexpr int kRelaxCounters = 4;    // counters [C, 4]: n_pos, steps, status, frozen (steps + 1 of the last freeze, 0: none yet)
constexpr int kRelaxNPos = 0, kRelaxSteps = 1, kRelaxStatus = 2, kRelaxFrozen = 3;

// what one call steps with: passed to the kernel by value
struct FireModel {
  double dt_max, f_inc, f_dec, a_start, f_a, max_step, f_max, skin;
  int n_min, max_steps;
};

EGNN_HD double relax_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
EGNN_HD double relax_max(double a, double b) { return b > a ? b : a; }

// site (j, code) of a held row about the centre at unwrapped ui: false where the entry names no site of the cell [lo, hi) or the
// site lies outside cut2 = r_cut * r_cut now; d is its vector where true
EGNN_HD bool relax_held_site(const double* frac, const double* L, int lo, int hi, const double* ui, int j, int code, double cut2, double* d) {
  if (!cell_site_listed(lo, hi, j, code)) return false;
  int s[3];
  cell_shift_decode(code, s);
  cell_site_vector(frac + 3 * (size_t)j, ui, s, L, d);
  return cell_norm2(d) < cut2;
}

// K [k][x] = (the cross product of the two other lattice rows)_x / det L: f_k = dot(r, K_k) are the fractional coordinates of r
EGNN_HD void relax_inverse(const double* L, double* K) {
  const double* a = L;
  const double* b = L + 3;
  const double* c = L + 6;
  const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
  const double ca[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
  const double ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double det = (a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2];
  for (int x = 0; x < 3; ++x) {
    K[x] = bc[x] / det;
    K[3 + x] = ca[x] / det;
    K[6 + x] = ab[x] / det;
  }
}
EGNN_HD void relax_to_fractional(const double* K, const double* r, double* f) {
  for (int k = 0; k < 3; ++k) f[k] = relax_dot(r, K + 3 * k);
}

// partial t of the sums of step 1 over the n atoms of a cell (F, v: the cell's first atom): out = (P, FF, vv, fm2)
EGNN_HD void relax_thread_sums(int t, int n, const double* F, const double* v, double* out) {
  double P = 0.0, FF = 0.0, vv = 0.0, fm2 = 0.0;
  for (int i = t; i < n; i += kRelaxThreads) {
    const double* Fi = F + 3 * (size_t)i;
    const double* vi = v + 3 * (size_t)i;
    const double ff = relax_dot(Fi, Fi);
    P += relax_dot(Fi, vi);
    FF += ff;
    vv += relax_dot(vi, vi);
    fm2 = relax_max(fm2, ff);
  }
  out[0] = P; out[1] = FF; out[2] = vv; out[3] = fm2;
}

// the decision of steps 3 and 4 from the state and the four sums
struct RelaxPlan {
  int status;        // kRelaxRunning: a move is planned
  int positive;      // P > 0
  int n_pos;
  double keep, c;    // v' = keep * v + c * F where positive
  double dt, a;      // dt', a'
};

EGNN_HD RelaxPlan relax_plan(const FireModel& M, double dt, double a, int n_pos, int steps, const double* sums) {
  RelaxPlan R;
  R.status = kRelaxRunning; R.positive = 0; R.n_pos = n_pos; R.keep = 0.0; R.c = 0.0; R.dt = dt; R.a = a;
  const double P = sums[0], FF = sums[1], vv = sums[2], fm2 = sums[3];
  if (!(FF < 1e300)) { R.status = kRelaxNotFinite; return R; }
  if (fm2 < M.f_max * M.f_max) { R.status = kRelaxConverged; return R; }
  if (steps >= M.max_steps) { R.status = kRelaxStepLimit; return R; }
  if (P > 0.0) {
    R.positive = 1;
    R.keep = 1.0 - a;
    R.c = (a * sqrt(vv)) / sqrt(FF);
    if (n_pos > M.n_min) {
      const double grown = dt * M.f_inc;
      R.dt = grown < M.dt_max ? grown : M.dt_max;
      R.a = a * M.f_a;
    }
    R.n_pos = n_pos + 1;
  } else {
    R.a = M.a_start;
    R.dt = dt * M.f_dec;
    R.n_pos = 0;
  }
  return R;
}

// v'' and the uncapped dr of one atom
EGNN_HD void relax_velocity(const RelaxPlan& R, const double* v, const double* F, double* vn, double* dr) {
  for (int k = 0; k < 3; ++k) {
    vn[k] = R.positive ? (R.keep * v[k] + R.c * F[k]) + R.dt * F[k] : R.dt * F[k];
    dr[k] = R.dt * vn[k];
  }
}

// partial t of m2 = max |dr_i|^2
EGNN_HD double relax_thread_move(int t, int n, const RelaxPlan& R, const double* F, const double* v) {
  double m2 = 0.0;
  for (int i = t; i < n; i += kRelaxThreads) {
    double vn[3], dr[3];
    relax_velocity(R, v + 3 * (size_t)i, F + 3 * (size_t)i, vn, dr);
    m2 = relax_max(m2, relax_dot(dr, dr));
  }
  return m2;
}

EGNN_HD double relax_cap(const FireModel& M, double m2) {
  const double m = sqrt(m2);
  return m > M.max_step ? M.max_step / m : 1.0;
}

// the capped move of one atom and what `since` becomes with it
EGNN_HD void relax_capped(const RelaxPlan& R, double scale, const double* v, const double* F, const double* since, double* vn, double* dr,
                          double* reach) {
  relax_velocity(R, v, F, vn, dr);
  for (int k = 0; k < 3; ++k) {
    dr[k] = scale * dr[k];
    reach[k] = since[k] + dr[k];
  }
}

// partial t of reach2 = max |since_i + dr_i|^2 and of held2 = max |since_i|^2: out = (reach2, held2)
EGNN_HD void relax_thread_reach(int t, int n, const RelaxPlan& R, double scale, const double* F, const double* v, const double* since,
                                double* out) {
  double r2 = 0.0, h2 = 0.0;
  for (int i = t; i < n; i += kRelaxThreads) {
    double vn[3], dr[3], reach[3];
    const double* si = since + 3 * (size_t)i;
    relax_capped(R, scale, v + 3 * (size_t)i, F + 3 * (size_t)i, si, vn, dr, reach);
    r2 = relax_max(r2, relax_dot(reach, reach));
    h2 = relax_max(h2, relax_dot(si, si));
  }
  out[0] = r2; out[1] = h2;
}

// a cell whose list has just been built (held2 == 0) is never frozen: see step 6
EGNN_HD bool relax_frozen(const FireModel& M, double reach2, double held2) { return held2 > 0.0 && sqrt(reach2) > 0.5 * M.skin; }
// whether a freeze at `steps` repeats the last one (`frozen` = steps + 1 of it): the cell has not moved in between
EGNN_HD bool relax_stuck(int frozen, int steps) { return frozen == steps + 1; }
// whether row `steps` lies inside the traces [max_steps + 1, C]
EGNN_HD bool relax_in_trace(const FireModel& M, int steps) { return steps >= 0 && steps <= M.max_steps; }

// step 7 for the atoms t, t + 256, .. of a cell
EGNN_HD void relax_thread_commit(int t, int n, const RelaxPlan& R, double scale, const double* K, const double* F, double* u, double* v,
                                 double* since, double* moved) {
  for (int i = t; i < n; i += kRelaxThreads) {
    double vn[3], dr[3], reach[3], du[3];
    relax_capped(R, scale, v + 3 * (size_t)i, F + 3 * (size_t)i, since + 3 * (size_t)i, vn, dr, reach);
    relax_to_fractional(K, dr, du);
    for (int k = 0; k < 3; ++k) {
      const size_t at = 3 * (size_t)i + k;
      v[at] = vn[k];
      u[at] = u[at] + du[k];
      since[at] = reach[k];
      moved[at] = moved[at] + dr[k];
    }
  }
}

// the tree over the kRelaxThreads partials on the host: s[t] (+ or max)= s[t + off], off = 128 .. 1; the result is s[0]
inline double relax_tree_host(double* s, bool is_max) {
  for (int off = kRelaxThreads / 2; off > 0; off >>= 1)
    for (int t = 0; t < off; ++t) s[t] = is_max ? relax_max(s[t], s[t + off]) : s[t] + s[t + off];
  return s[0];
}

}  // namespace egnn

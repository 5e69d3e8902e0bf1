// Host side of the bond-orientational-order entries: the argument checks of the device entries (cell_boo.hip) and the host
// statement egnn_cell_boo_host -- the box walk of egnn_cell_sites_host, q_lm of every atom and the invariants of the listed centres
// computed on the CPU through cell_boo_math.h, the text the kernels compile, in the orders it states.  No HIP call, no device code:
// checked (and run under the sanitizers) on a machine without a GPU.
#include <math.h>
#include <string.h>

#include "cell_boo_host.h"
#include "cell_boo_math.h"

namespace egnn {

int cell_boo_config_check(const char* who, int A, int l_max, int l_solid, unsigned select) {
  if (int rc = atom_types_check(who, A, kCellMaxTypes)) return rc;
  if (l_max < 0 || l_max > kBooMaxL) { set_error("%s: l_max %d (0 <= l_max <= %d)", who, l_max, kBooMaxL); return EGNN_EINVAL; }
  if (l_solid != -1 && (l_solid < 0 || l_solid > l_max)) { set_error("%s: l_solid %d (0 <= l_solid <= l_max = %d)", who, l_solid, l_max); return EGNN_EINVAL; }
  if (select >> (A * A)) { set_error("%s: select 0x%x has a bit beyond the %d x %d type pairs", who, select, A, A); return EGNN_EINVAL; }
  return EGNN_OK;
}

int cell_boo_table_check(const char* who, int l_max, int E, const int32_t* g_off) {
  if (E < 0 || !g_off) { set_error("bad %s arguments (E >= 0 entries of G; the host copy of g_off given)", who); return EGNN_EINVAL; }
  if (g_off[0] != 0 || g_off[l_max + 1] != E) { set_error("%s: g_off must run from 0 to E = %d", who, E); return EGNN_EINVAL; }
  for (int l = 0; l <= l_max; ++l)
    if (g_off[l + 1] < g_off[l]) { set_error("%s: g_off decreases at l = %d", who, l); return EGNN_EINVAL; }
  return EGNN_OK;
}

namespace {

struct BooCells {
  int C, A, l_max;
  unsigned select;
  double cut;
  const int32_t* cell_ptr;
  const double* lattice;
  const double* frac;
  const int32_t* type;
  const double* norm;
};

// the kept sites of atom i in ascending (atom, shift code): f(atom, unit vector)
template <typename F>
void boo_walk(const BooCells& b, int i, F f) {
  const int c = cell_of_atom_host(b.cell_ptr, b.C, i);
  const int lo = b.cell_ptr[c], hi = b.cell_ptr[c + 1];
  const double* L = b.lattice + 9 * (size_t)c;
  int box[3];
  double width[3];
  cell_soap_box(L, b.cut, box, width);
  const int nbox = cell_soap_box_count(box);
  const double cut2 = b.cut * b.cut;
  double wi[3], wj[3];
  cell_wrapped_read(b.frac, i, wi);
  for (int j = lo; j < hi; ++j) {
    cell_wrapped_read(b.frac, j, wj);
    for (int t = 0; t < nbox; ++t) {
      int s[3];
      double r[3], u[3];
      cell_soap_box_shift(t, box, s);
      if (j == i && s[0] == 0 && s[1] == 0 && s[2] == 0) continue;
      if (!cell_soap_site(wj, wi, s, L, cut2, r)) continue;
      if (boo_site(b.frac, b.type, L, lo, hi, b.A, b.select, i, j, cell_shift_code(s[0], s[1], s[2]), u)) f(j, u);
    }
  }
}

}  // namespace
}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_boo_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type, double cutoff,
                       unsigned select, int l_max, const double* norm, int E, const int32_t* g_off, const int32_t* g_idx, const double* g_val,
                       int l_solid, double threshold, int averaged, int M, const int32_t* centre_atom, double* out, int32_t* n,
                       int32_t* n_solid, double* qlm) {
  const char* who = "egnn_cell_boo_host";
  if (C < 1 || !cell_ptr || M < 0 || (M > 0 && (!centre_atom || !out || !n || !n_solid)) || !norm || (E > 0 && (!g_idx || !g_val))) {
    set_error("bad %s arguments (C >= 1; cell_ptr, norm and the G tables given; M >= 0 centres with out, n and n_solid)", who);
    return EGNN_EINVAL;
  }
  const int N = cell_ptr[C];
  if (l_solid < 0) { set_error("%s: l_solid %d (0 <= l_solid <= l_max)", who, l_solid); return EGNN_EINVAL; }
  if (int rc = cell_boo_config_check(who, A, l_max, l_solid, select)) return rc;
  if (int rc = cell_boo_table_check(who, l_max, E, g_off)) return rc;
  if (cutoff == 0.0) { set_error("%s: cutoff must be positive and finite", who); return EGNN_EINVAL; }
  if (int rc = cell_soap_batch_check(who, C, N, cell_ptr, lattice, cutoff)) return rc;
  if (N > 0 && (!frac || !type)) { set_error("bad %s arguments (frac and type given)", who); return EGNN_EINVAL; }
  if (int rc = cell_inputs_check(who, N, frac, type, A, M, centre_atom)) return rc;
  const int L1 = l_max + 1, LM = soap_lm_count(l_max), blocks = averaged ? 6 : 3;
  Scratch<double> all((size_t)N * LM), col((size_t)LM), acc((size_t)LM);
  if (!all.p || !col.p || !acc.p) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
  const BooCells b = {C, A, l_max, select, cutoff, cell_ptr, lattice, frac, type, norm};
  for (int i = 0; i < N; ++i) {   // pass 1: q_lm of every atom
    double* row = all.p + (size_t)i * LM;
    int kept = 0;
    boo_walk(b, i, [&](int, const double* u) {
      const double uu = cell_norm2(u);
      for (int m = 0; m <= l_max; ++m) soap_solid_column(u[0], u[1], u[2], uu, m, l_max, norm, col.p);
      for (int lm = 0; lm < LM; ++lm) row[lm] += col[lm];
      ++kept;
    });
    for (int lm = 0; lm < LM; ++lm) row[lm] = kept > 0 ? row[lm] / (double)kept : 0.0;
  }
  for (int m = 0; m < M; ++m) {   // pass 2: the invariants of the listed centres
    const int i = centre_atom[m];
    const double* own = all.p + (size_t)i * LM;
    double* o = out + (size_t)m * blocks * L1;
    for (int l = 0; l <= l_max; ++l) boo_invariants(own, l, l_max, E, g_off, g_idx, g_val, o);
    for (int lm = 0; lm < LM; ++lm) acc[lm] = own[lm];
    int kept = 0, solid = 0;
    boo_walk(b, i, [&](int j, const double*) {
      const double* other = all.p + (size_t)j * LM;
      if (averaged)
        for (int lm = 0; lm < LM; ++lm) acc[lm] += other[lm];
      solid += boo_solid(own, other, l_solid) > threshold;
      ++kept;
    });
    n[m] = kept;
    n_solid[m] = solid;
    if (averaged) {
      for (int lm = 0; lm < LM; ++lm) acc[lm] = acc[lm] / (double)(1 + kept);
      for (int l = 0; l <= l_max; ++l) boo_invariants(acc.p, l, l_max, E, g_off, g_idx, g_val, o + 3 * L1);
    }
    if (qlm) memcpy(qlm + (size_t)m * LM, own, sizeof(double) * LM);
  }
  return EGNN_OK;
}

}  // extern "C"

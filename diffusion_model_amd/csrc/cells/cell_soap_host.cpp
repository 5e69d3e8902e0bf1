// Host side of the periodic-cell SOAP entries: the argument checks of the device entries (cell_soap.hip) and the host statements
// egnn_cell_sites_host, egnn_cell_soap_host and egnn_cell_soap_mean_host -- the box walk without a cull, the descriptor and the
// per-cell mean computed on the CPU through cell_soap_math.h and soap_math.h, the text the kernels compile.  No HIP call, no device
// code: checked (and run under the sanitizers) on a machine without a GPU.
#include <math.h>
#include <string.h>

#include "cell_soap_host.h"
#include "cell_soap_math.h"

namespace egnn {

// the shift code holds the sites of a cell whose image box stays within 4 (cell_soap_math.h)
static int cell_widths_box_rule(const char* who, int c, const double* L, const double* w, double cut) {
  int b[3];
  double w_box[3];
  if (cell_soap_box(L, cut, b, w_box)) return EGNN_OK;
  set_error("%s: cell %d has perpendicular widths %.6g, %.6g, %.6g and one is at most cut / 4 = %.6g (an image box beyond %d)", who, c, w[0],
            w[1], w[2], cut / 4.0, kCellSoapMaxBox);
  return EGNN_EINVAL;
}

int cell_soap_batch_check(const char* who, int C, int N, const int32_t* cell_ptr, const double* lattice, double cut) {
  if (C < 1 || N < 0 || !cell_ptr || !lattice) {
    set_error("bad %s arguments (C >= 1, N >= 0, the host copies of cell_ptr and lattice given)", who);
    return EGNN_EINVAL;
  }
  if (cut != 0.0 && (!soap_cut_ok(cut) || !(cut < 1e30))) { set_error("%s: cut must be positive and finite", who); return EGNN_EINVAL; }
  return cell_batch_core_check(who, C, N, cell_ptr, lattice, cut == 0.0 ? nullptr : cell_widths_box_rule, cut);
}

int cell_soap_basis_check(const char* who, int A, int n_max, int l_max, const void* tables) {
  if (int rc = atom_types_check(who, A, kSoapMaxTypes)) return rc;
  if (n_max < 1 || n_max > kSoapMaxN) { set_error("%s: n_max %d (1 <= n_max <= %d)", who, n_max, kSoapMaxN); return EGNN_EINVAL; }
  if (l_max < 0 || l_max > kSoapMaxL) { set_error("%s: l_max %d (0 <= l_max <= %d)", who, l_max, kSoapMaxL); return EGNN_EINVAL; }
  if (!tables) { set_error("bad %s arguments (tables given)", who); return EGNN_EINVAL; }
  return EGNN_OK;
}

// what the two host statements ask of their inputs beyond the batch check: finite coordinates, centres inside the batch
static int cell_soap_inputs_check(const char* who, int N, const double* frac, int M, const int32_t* centre_atom) {
  if (M < 0 || (M > 0 && !centre_atom) || (N > 0 && !frac)) { set_error("bad %s arguments (M >= 0 centres and frac given)", who); return EGNN_EINVAL; }
  return cell_inputs_check(who, N, frac, nullptr, 0, M, centre_atom);
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_cell_sites_host(int C, const int32_t* cell_ptr, const double* lattice, const double* frac, double cut, int M,
                         const int32_t* centre_atom, int32_t* row_ptr, int64_t site_cap, int32_t* site_atom, int32_t* site_shift) {
  const char* who = "egnn_cell_sites_host";
  if (C < 1 || !cell_ptr || !row_ptr) { set_error("bad %s arguments (C >= 1; cell_ptr and row_ptr given)", who); return EGNN_EINVAL; }
  const int N = cell_ptr[C];
  if (cut == 0.0) { set_error("%s: cut must be positive and finite", who); return EGNN_EINVAL; }
  if (int rc = cell_soap_batch_check(who, C, N, cell_ptr, lattice, cut)) return rc;
  if (int rc = cell_soap_inputs_check(who, N, frac, M, centre_atom)) return rc;
  Scratch<double> w(3 * (size_t)N);
  if (int rc = cell_wrap_batch(who, N, frac, w)) return rc;
  const double cut2 = cut * cut;
  const bool lists = site_atom && site_shift;
  row_ptr[0] = 0;
  for (int pass = 0; pass < 2; ++pass) {
    int64_t total = 0;
    for (int m = 0; m < M; ++m) {
      const int i = centre_atom[m], c = cell_of_atom_host(cell_ptr, C, i), lo = cell_ptr[c], n = cell_ptr[c + 1] - lo;
      const double* L = lattice + 9 * (size_t)c;
      int b[3];
      double width[3];
      cell_soap_box(L, cut, b, width);
      const int nbox = cell_soap_box_count(b);
      for (int j = 0; j < n; ++j)
        for (int t = 0; t < nbox; ++t) {
          int s[3];
          double r[3];
          cell_soap_box_shift(t, b, s);
          if (lo + j == i && s[0] == 0 && s[1] == 0 && s[2] == 0) continue;
          if (!cell_soap_site(&w[3 * (size_t)(lo + j)], &w[3 * (size_t)i], s, L, cut2, r)) continue;
          if (pass == 1) {
            site_atom[(size_t)total] = lo + j;
            site_shift[(size_t)total] = cell_shift_code(s[0], s[1], s[2]);
          }
          ++total;
        }
      if (total > 2147483647LL) { set_error("%s: more than 2^31 - 1 sites", who); return EGNN_EINVAL; }
      row_ptr[m + 1] = (int32_t)total;
    }
    if (!lists || site_cap < total) break;   // sizes only
  }
  return EGNN_OK;
}

int egnn_cell_soap_host(int C, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type, int n_max,
                        int l_max, double cut, const double* tables, int M, const int32_t* centre_atom, double* desc, double* coeff) {
  const char* who = "egnn_cell_soap_host";
  if (C < 1 || !cell_ptr || (M > 0 && !desc)) { set_error("bad %s arguments (C >= 1; cell_ptr and desc given)", who); return EGNN_EINVAL; }
  const int N = cell_ptr[C];
  if (int rc = cell_soap_basis_check(who, A, n_max, l_max, tables)) return rc;
  if (cut == 0.0) { set_error("%s: cut must be positive and finite", who); return EGNN_EINVAL; }
  if (int rc = cell_soap_batch_check(who, C, N, cell_ptr, lattice, cut)) return rc;
  if (int rc = cell_soap_inputs_check(who, N, frac, M, centre_atom)) return rc;
  if (N > 0 && !type) { set_error("bad %s arguments (type given)", who); return EGNN_EINVAL; }
  if (int rc = type_range_check(who, type, 0, N, A)) return rc;
  const int L1 = l_max + 1, LM = soap_lm_count(l_max), nF = soap_feature_count(A, n_max, l_max);
  const size_t nC = (size_t)A * n_max * LM;
  Scratch<double> w(3 * (size_t)N), prim(nC), c(nC), solid((size_t)LM), radial((size_t)n_max * L1);
  if (int rc = cell_wrap_batch(who, N, frac, w)) return rc;
  if (!prim.p || !c.p || !solid.p || !radial.p) { set_error("%s: out of memory", who); return EGNN_ENOMEM; }
  const double cut2 = cut * cut;
  const double* norm = tables + soap_table_norm(n_max, l_max);
  const double* beta = tables + soap_table_beta(n_max, l_max);
  for (int m = 0; m < M; ++m) {
    const int i = centre_atom[m], cell = cell_of_atom_host(cell_ptr, C, i), lo = cell_ptr[cell], n = cell_ptr[cell + 1] - lo;
    const double* L = lattice + 9 * (size_t)cell;
    int b[3];
    double width[3];
    cell_soap_box(L, cut, b, width);
    const int nbox = cell_soap_box_count(b);
    for (size_t o = 0; o < nC; ++o) prim[o] = 0.0;
    for (int q = -1; q < n * nbox; ++q) {   // -1: the centre itself, first
      int s[3] = {0, 0, 0};
      double r[3] = {0.0, 0.0, 0.0};
      int j = i;
      if (q >= 0) {
        j = lo + q / nbox;
        cell_soap_box_shift(q % nbox, b, s);
        if (j == i && s[0] == 0 && s[1] == 0 && s[2] == 0) continue;
        if (!cell_soap_site(&w[3 * (size_t)j], &w[3 * (size_t)i], s, L, cut2, r)) continue;
      }
      const double d2 = cell_norm2(r);
      for (int mm = 0; mm <= l_max; ++mm) soap_solid_column(r[0], r[1], r[2], d2, mm, l_max, norm, solid.p);
      for (int k = 0; k < n_max * L1; ++k) radial[k] = soap_radial(tables, n_max, l_max, k, d2);
      double* pz = prim.p + (size_t)type[j] * n_max * LM;
      for (int nn = 0; nn < n_max; ++nn)
        for (int lm = 0; lm < LM; ++lm) pz[nn * LM + lm] += radial[nn * L1 + soap_l_of(lm)] * solid[lm];
    }
    for (int z = 0; z < A; ++z)
      for (int lm = 0; lm < LM; ++lm) {
        const double* bl = beta + (size_t)soap_l_of(lm) * n_max * n_max;
        for (int nn = 0; nn < n_max; ++nn) {
          double sum = 0.0;
          for (int np = 0; np < n_max; ++np) sum += bl[nn * n_max + np] * prim[((size_t)z * n_max + np) * LM + lm];
          c[((size_t)z * n_max + nn) * LM + lm] = sum;
        }
      }
    if (coeff) memcpy(coeff + (size_t)m * nC, c.p, sizeof(double) * nC);
    for (int f = 0; f < nF; ++f) desc[(size_t)m * nF + f] = soap_power_entry(c.p, tables, f, A, n_max, l_max);
  }
  return EGNN_OK;
}

int egnn_cell_soap_mean_host(int C, int F, const int32_t* cell_rows, const double* desc, const int64_t* count, int first, int final,
                             double* sum) {
  const char* who = "egnn_cell_soap_mean_host";
  if (C < 1 || F < 1 || !cell_rows || !sum || (final && !count)) {
    set_error("bad %s arguments (C, F >= 1; cell_rows and sum given; count given with final)", who);
    return EGNN_EINVAL;
  }
  if (cell_rows[0] != 0) { set_error("%s: cell_rows must start at 0", who); return EGNN_EINVAL; }
  for (int c = 0; c < C; ++c)
    if (cell_rows[c + 1] < cell_rows[c]) { set_error("%s: cell_rows decreases at cell %d", who, c); return EGNN_EINVAL; }
  if (cell_rows[C] > 0 && !desc) { set_error("bad %s arguments (desc given)", who); return EGNN_EINVAL; }
  for (int c = 0; c < C; ++c)
    for (int f = 0; f < F; ++f) {
      double acc = first ? 0.0 : sum[(size_t)c * F + f];
      for (int m = cell_rows[c]; m < cell_rows[c + 1]; ++m) acc += desc[(size_t)m * F + f];
      if (final) acc = count[c] > 0 ? acc / (double)count[c] : 0.0;
      sum[(size_t)c * F + f] = acc;
    }
  return EGNN_OK;
}

}  // extern "C"

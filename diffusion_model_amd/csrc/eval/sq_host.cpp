// Host side of the reciprocal-space statistics: the argument checks of the device entries (sq.hip), the index plan of a batch of
// cells (egnn_sq_cell_plan) and the host statement egnn_sq_host -- Debye sums, per-vector rho and shell averages computed on the
// CPU through sq_math.h, the text the kernels compile, in a summation order of its own (pairs i < j ascending; atoms ascending;
// vectors ascending).  No HIP call, no device code: checked (and run under the sanitizers, make asan) on a machine without a GPU.
#include <math.h>
#include <string.h>

#include "sq_host.h"
#include "sq_math.h"

namespace egnn {

int sq_debye_args_check(const char* who, int B, int A, const void* pos, const void* type, const void* graph_ptr, int max_atoms, int Q,
                        const double* q, double r_max, int window, const void* out) {
  if (B < 1 || !pos || !type || !graph_ptr || !out) { set_error("bad %s arguments (B >= 1; pos, type, graph_ptr and the output given)", who); return EGNN_EINVAL; }
  if (int rc = atom_types_check(who, A, kSqMaxTypes)) return rc;
  if (max_atoms < 0 || max_atoms > kSqMaxAtoms) { set_error("%s: a graph of %d atoms (at most %d)", who, max_atoms, kSqMaxAtoms); return EGNN_EINVAL; }
  if (Q < 1 || Q > kSqMaxQ || !q) { set_error("%s: %d q values (1 <= Q <= %d, the host copy of q given)", who, Q, kSqMaxQ); return EGNN_EINVAL; }
  for (int k = 0; k < Q; ++k)
    if (!(q[k] >= 0.0) || !(q[k] < INFINITY)) { set_error("%s: q[%d] = %g (every q must be finite and not negative)", who, k, q[k]); return EGNN_EINVAL; }
  if (!(r_max > 0.0)) { set_error("%s: r_max must be positive (+inf: no cut)", who); return EGNN_EINVAL; }
  if (window != kSqWindowNone && window != kSqWindowLorch) { set_error("%s: window %d (0: none, 1: Lorch)", who, window); return EGNN_EINVAL; }
  if (window == kSqWindowLorch && !(r_max < INFINITY)) { set_error("%s: the Lorch window needs a finite r_max", who); return EGNN_EINVAL; }
  return EGNN_OK;
}

int sq_tiles_args_check(const char* who, const void* tiles, int n_tiles, const void* tile_ptr, const void* partial) {
  if (n_tiles < 0 || !tile_ptr || (n_tiles > 0 && (!tiles || !partial))) {
    set_error("bad %s arguments (n_tiles >= 0 tiles, tile_ptr and the partial sums given)", who);
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

int sq_cells_check(const char* who, int C, int A, const int32_t* cell_ptr, const double* lattice, double q_max, int32_t* hkl_box) {
  if (C < 1 || C > 65535 || !lattice) { set_error("bad %s arguments (1 <= C <= 65535, the host copy of the lattices given)", who); return EGNN_EINVAL; }
  if (int rc = atom_types_check(who, A, kSqMaxTypes)) return rc;
  if (!(q_max > 0.0) || !(q_max < 1e30)) { set_error("%s: q_max must be positive and finite", who); return EGNN_EINVAL; }
  for (int c = 0; c < C; ++c) {
    if (cell_ptr)
      if (int rc = ptr_step_check(who, "cell_ptr", "cell", cell_ptr, c, kCellMaxAtoms)) return rc;
    double Bm[9];
    int need[3];
    if (!sq_reciprocal(lattice + 9 * (size_t)c, Bm)) { set_error("%s: cell %d has a singular lattice", who, c); return EGNN_EINVAL; }
    if (!sq_index_need(lattice + 9 * (size_t)c, q_max, need)) {
      set_error("%s: cell %d needs a Miller index above %d at q_max = %g (lower q_max)", who, c, kSqMaxIndex, q_max);
      return EGNN_EINVAL;
    }
    if (hkl_box)
      for (int i = 0; i < 3; ++i) hkl_box[3 * c + i] = sq_index_box(need[i]);
  }
  return EGNN_OK;
}

int sq_bins_check(const char* who, double q_max, double dq, int nbins) {
  if (!(dq > 0.0) || !(dq < 1e30)) { set_error("%s: dq must be positive and finite", who); return EGNN_EINVAL; }
  const int want = sq_nbins(q_max, dq);
  if (want < 1 || want > kSqMaxBins) { set_error("%s: ceil(q_max / dq) = %d shell bins (1 <= nbins <= %d)", who, want, kSqMaxBins); return EGNN_EINVAL; }
  if (nbins != want) { set_error("%s: nbins %d, but ceil(q_max / dq) = %d", who, nbins, want); return EGNN_EINVAL; }
  return EGNN_OK;
}

int sq_plan_check(const char* who, int C, const double* lattice, double q_max, const int32_t* plan, int n_rows, int* max_rows) {
  if (!plan || n_rows < 0) { set_error("bad %s arguments (the host copy of the plan given, n_rows >= 0)", who); return EGNN_EINVAL; }
  long long rows = 0;
  *max_rows = 0;
  for (int c = 0; c < C; ++c) {
    int need[3];
    if (!sq_index_need(lattice + 9 * (size_t)c, q_max, need)) { set_error("%s: cell %d needs a Miller index above %d", who, c, kSqMaxIndex); return EGNN_EINVAL; }
    const int32_t* p = plan + 4 * (size_t)c;
    if (p[0] != sq_index_box(need[0]) || p[1] != sq_index_box(need[1]) || p[2] != sq_index_box(need[2]) || p[3] != rows) {
      set_error("%s: the plan of cell %d is not egnn_sq_cell_plan's for these lattices and this q_max", who, c);
      return EGNN_EINVAL;
    }
    const int r = sq_box_rows(p[0], p[1]);
    rows += r;
    if (r > *max_rows) *max_rows = r;
  }
  if (rows != n_rows) { set_error("%s: n_rows %d, the plan has %lld", who, n_rows, rows); return EGNN_EINVAL; }
  return EGNN_OK;
}

int sq_vec_ptr_check(const char* who, int C, const int32_t* vec_ptr, int K) {
  if (!vec_ptr || K < 0 || vec_ptr[0] != 0 || vec_ptr[C] != K) { set_error("%s: the host copy of vec_ptr must run from 0 to K = %d", who, K); return EGNN_EINVAL; }
  for (int c = 0; c < C; ++c) {
    const long long n = (long long)vec_ptr[c + 1] - vec_ptr[c];
    if (n < 0) { set_error("%s: vec_ptr decreases at cell %d", who, c); return EGNN_EINVAL; }
    if (n > kSqMaxVectors) { set_error("%s: cell %d has %lld vectors below q_max (at most %d; lower q_max)", who, c, n, kSqMaxVectors); return EGNN_EINVAL; }
  }
  return EGNN_OK;
}

namespace {

int debye_host(const char* who, int B, int N, int A, const float* pos, const int32_t* type, const int32_t* graph_ptr, int Q, const double* q,
               double r_max, int window, double* out) {
  if (int rc = sq_debye_args_check(who, B, A, pos, type, graph_ptr, 0, Q, q, r_max, window, out)) return rc;
  if (graph_ptr[0] != 0 || graph_ptr[B] != N) { set_error("%s: graph_ptr must run from 0 to N = %d", who, N); return EGNN_EINVAL; }
  for (int g = 0; g < B; ++g)
    if (int rc = ptr_step_check(who, "graph_ptr", "graph", graph_ptr, g, kSqMaxAtoms)) return rc;
  if (int rc = type_range_check(who, type, 0, N, A)) return rc;
  const int P = type_pairs(A);
  Scratch<double> sum((size_t)P * Q);
  if (!sum.p) { set_error("%s: out of memory", who); return EGNN_EINVAL; }
  for (int g = 0; g < B; ++g) {
    const int lo = graph_ptr[g], hi = graph_ptr[g + 1];
    memset(sum.p, 0, sizeof(double) * (size_t)P * Q);
    for (int i = lo; i < hi; ++i)
      for (int j = i + 1; j < hi; ++j) {
        const float* a = pos + 3 * (size_t)i;
        const float* b = pos + 3 * (size_t)j;
        const double r = distance64(a[0], a[1], a[2], b[0], b[1], b[2]);
        if (!(r < r_max)) continue;
        const double w = sq_window(r, r_max, window);
        double* row = sum.p + (size_t)type_pair_index(type[i], type[j], A) * Q;
        for (int k = 0; k < Q; ++k) row[k] += w * sq_sinc(q[k] * r);
      }
    for (int a = 0; a < A; ++a)
      for (int b = 0; b < A; ++b) {
        const double* row = sum.p + (size_t)type_pair_index(a, b, A) * Q;
        double* o = out + (((size_t)g * A + a) * A + b) * Q;
        for (int k = 0; k < Q; ++k) o[k] = a == b ? 2.0 * row[k] : row[k];
      }
  }
  return EGNN_OK;
}

int cells_host(const char* who, int C, int N, int A, const int32_t* cell_ptr, const double* lattice, const double* frac, const int32_t* type,
               double q_max, double dq, int nbins, int64_t vec_cap, int64_t* vec_ptr, int32_t* hkl, double* kabs, int32_t* bin, double* rho,
               int64_t* count, double* mean_k, double* s) {
  if (!cell_ptr || !frac || !type || !vec_ptr || vec_cap < 0) { set_error("bad %s arguments (cell_ptr, frac, type and vec_ptr given)", who); return EGNN_EINVAL; }
  if (C < 1 || C > 65535 || cell_ptr[0] != 0 || cell_ptr[C] != N) { set_error("%s: 1 <= C <= 65535 and cell_ptr must run from 0 to N = %d", who, N); return EGNN_EINVAL; }
  Scratch<int32_t> box(3 * (size_t)(C > 0 ? C : 1));
  if (int rc = sq_cells_check(who, C, A, cell_ptr, lattice, q_max, box.p)) return rc;
  if (int rc = sq_bins_check(who, q_max, dq, nbins)) return rc;
  for (int i = 0; i < cell_ptr[C]; ++i) {
    if (type[i] < 0 || type[i] >= A) { set_error("%s: atom %d has type %d outside [0, %d)", who, i, type[i], A); return EGNN_EINVAL; }
    for (int x = 0; x < 3; ++x)
      if (!(fabs(frac[3 * (size_t)i + x]) < 1e15)) { set_error("%s: atom %d has a coordinate that is not finite", who, i); return EGNN_EINVAL; }
  }
  const bool shells = count && mean_k && s;
  if (shells) {
    for (size_t t = 0; t < (size_t)C * nbins; ++t) { count[t] = 0; mean_k[t] = 0.0; }
    for (size_t t = 0; t < (size_t)C * A * A * nbins; ++t) s[t] = 0.0;
  }
  int64_t K = 0;
  vec_ptr[0] = 0;
  Scratch<double> half((size_t)(shells ? nbins : 1));   // half-space vectors of each bin
  for (int c = 0; c < C; ++c) {
    const int lo = cell_ptr[c], n = cell_ptr[c + 1] - lo;
    double Bm[9];
    sq_reciprocal(lattice + 9 * (size_t)c, Bm);
    Scratch<double> w(3 * (size_t)n);
    if (!w.p) { set_error("%s: out of memory", who); return EGNN_EINVAL; }
    for (int t = 0; t < 3 * n; ++t) w[t] = cell_wrap(frac[3 * (size_t)lo + t]);
    if (shells) memset(half.p, 0, sizeof(double) * nbins);
    int64_t n_vec = 0;
    const int H = box[3 * c], Kb = box[3 * c + 1], Lb = box[3 * c + 2];
    for (int h = 0; h <= H; ++h)
      for (int k = -Kb; k <= Kb; ++k)
        sq_row_vectors(h, k, Lb, Bm, q_max, [&](int, int l, double k2) {
          const double ka = sqrt(k2);
          const int bn = sq_bin(ka, dq, nbins);
          double re[kSqMaxTypes] = {0.0, 0.0, 0.0, 0.0}, im[kSqMaxTypes] = {0.0, 0.0, 0.0, 0.0};
          for (int j = 0; j < n; ++j) {
            double sn, cs;
            sq_phase_sincos(sq_phase(h, k, l, w.p + 3 * (size_t)j), &sn, &cs);
            re[type[lo + j]] += cs;
            im[type[lo + j]] -= sn;
          }
          const int64_t v = K + n_vec;
          if (v < vec_cap) {
            if (hkl) { hkl[3 * v] = h; hkl[3 * v + 1] = k; hkl[3 * v + 2] = l; }
            if (kabs) kabs[v] = ka;
            if (bin) bin[v] = bn;
            if (rho)
              for (int a = 0; a < A; ++a) { rho[(v * A + a) * 2] = re[a]; rho[(v * A + a) * 2 + 1] = im[a]; }
          }
          if (shells) {
            half[bn] += 1.0;
            mean_k[(size_t)c * nbins + bn] += ka;
            for (int a = 0; a < A; ++a)
              for (int b = 0; b < A; ++b) s[(((size_t)c * A + a) * A + b) * nbins + bn] += re[a] * re[b] + im[a] * im[b];
          }
          ++n_vec;
        });
    if (n_vec > kSqMaxVectors) { set_error("%s: cell %d has %lld vectors below q_max (at most %d; lower q_max)", who, c, (long long)n_vec, kSqMaxVectors); return EGNN_EINVAL; }
    K += n_vec;
    vec_ptr[c + 1] = K;
    if (shells)
      for (int bn = 0; bn < nbins; ++bn) {
        const double m = half[bn];
        count[(size_t)c * nbins + bn] = 2 * (int64_t)m;
        mean_k[(size_t)c * nbins + bn] = m > 0.0 ? mean_k[(size_t)c * nbins + bn] / m : NAN;
        for (int ab = 0; ab < A * A; ++ab) {
          double* v = &s[((size_t)c * A * A + ab) * nbins + bn];
          *v = m > 0.0 ? *v / m : NAN;
        }
      }
  }
  return EGNN_OK;
}

}  // namespace

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_sq_cell_plan(int C, const double* lattice, double q_max, int32_t* plan, int32_t* n_rows) {
  const char* who = "egnn_sq_cell_plan";
  if (!plan || !n_rows) { set_error("bad %s arguments (plan and n_rows given)", who); return EGNN_EINVAL; }
  if (int rc = sq_cells_check(who, C, 1, nullptr, lattice, q_max, nullptr)) return rc;
  long long rows = 0;
  for (int c = 0; c < C; ++c) {
    int need[3];
    sq_index_need(lattice + 9 * (size_t)c, q_max, need);
    int32_t* p = plan + 4 * (size_t)c;
    for (int i = 0; i < 3; ++i) p[i] = sq_index_box(need[i]);
    p[3] = (int32_t)rows;
    rows += sq_box_rows(p[0], p[1]);
    if (rows > 2147483647LL) { set_error("%s: more than 2^31 - 1 (h, k) rows in the batch (fewer cells per call)", who); return EGNN_EINVAL; }
  }
  *n_rows = (int32_t)rows;
  return EGNN_OK;
}

int egnn_sq_host(int B, int N, int A, const float* pos, const int32_t* type, const int32_t* graph_ptr, int Q, const double* q, double r_max,
                 int window, double* debye, int C, int cell_N, int cell_A, const int32_t* cell_ptr, const double* lattice, const double* frac,
                 const int32_t* cell_type, double q_max, double dq, int nbins, int64_t vec_cap, int64_t* vec_ptr, int32_t* hkl, double* kabs,
                 int32_t* bin, double* rho, int64_t* count, double* mean_k, double* s) {
  const char* who = "egnn_sq_host";
  if (B < 0 || C < 0 || (B == 0 && C == 0)) { set_error("bad %s arguments (graphs, B > 0, or cells, C > 0)", who); return EGNN_EINVAL; }
  if (B > 0)
    if (int rc = debye_host(who, B, N, A, pos, type, graph_ptr, Q, q, r_max, window, debye)) return rc;
  if (C > 0)
    if (int rc = cells_host(who, C, cell_N, cell_A, cell_ptr, lattice, frac, cell_type, q_max, dq, nbins, vec_cap, vec_ptr, hkl, kabs, bin, rho, count,
                            mean_k, s))
      return rc;
  return EGNN_OK;
}

}  // extern "C"

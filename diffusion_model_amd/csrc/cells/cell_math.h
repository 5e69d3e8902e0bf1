// Definitions of the local environments of periodic cells (cell_env.hip, cell_host.cpp): the periodic bond list of a batch of
// cells and the shell cluster about a centre.  Plain C++ behind a host/device macro (the pattern of eval/structure_math.h), so that
// the kernels and the host statement read the same text.  They restate make_dataset.py:79-142 (3x3x3 supercell,
// return_index_within_2ang, nested loops to 2NN / 3NN / 4NN, positions relative to the centre) on the INFINITE lattice.
//
//  * cell: lattice double [9], rows are the lattice vectors a, b, c; fractional coordinates are wrapped to [0, 1) first,
//    w = f - floor(f) in fp64 (a result that rounds to 1.0, f = -1e-18, is 0.0), and every shift refers to the wrapped atoms.
//  * site (j, s), s in Z^3: the image of atom j displaced by s lattice vectors.  Its vector from the wrapped centre i:
//    d_k = (w_j[k] - w_i[k]) + (double)s_k, r_x = (d_0 L[0][x] + d_1 L[1][x]) + d_2 L[2][x], in exactly this order (the library is
//    built with -ffp-contract=off); the position of a site is (float)r_x, rounded once, computed from the site and not along a path.
//  * bond: site (j, s), s in {-1, 0, 1}^3, (j, s) != (i, 0), is bonded to atom i iff (r_x r_x + r_y r_y) + r_z r_z < cutoff * cutoff
//    in fp64.  With every perpendicular width of the cell >= cutoff these 27 images are complete: |d_k| w_k <= |r| < cutoff <= w_k.
//  * shift code: ((s_x + 4) 9 + (s_y + 4)) 9 + (s_z + 4) in [0, 729): |s_k| <= 4 covers four bonds of |s_k| <= 1 each; ascending
//    codes are ascending (s_x, s_y, s_z).  A site key is atom * 729 + code, atom counted inside its cell.
//  * environment of centre i to depth `shells`: the sites reachable from (i, 0) in at most `shells` bonds, the centre first, the
//    others by ascending key.
#pragma once
#include "../eval/eval_math.h"

namespace egnn {

constexpr int kCellMaxTypes = 4;            // A
constexpr int kCellMaxShells = 4;           // hops
constexpr int kCellShiftSpan = 9;           // shift values per axis, -4 .. 4
constexpr int kCellShiftCodes = 729;        // 9^3
constexpr int kCellCentreCode = 364;        // the code of shift (0, 0, 0)
constexpr int kCellMaxEnvAtoms = 1024;      // max_atoms: sites of one environment
constexpr int kCellMaxAtoms = 1 << 20;      // atoms of one cell: atom * 729 + code stays inside int32
constexpr int kCellCentreBlock = 64;        // bond tile: centres (16 per wavefront)
constexpr int kCellChunk = 1024;            // bond tile: neighbour atoms staged in LDS
constexpr int kCellEnvWaves = 4;            // environment tile: centres, one wavefront each
constexpr int kCellEnvSlack = 64;           // sites one breadth-first step of a wavefront can append beyond max_atoms

EGNN_HD double cell_wrap(double f) {
  const double w = f - floor(f);
  return w < 1.0 ? w : 0.0;
}

EGNN_HD int cell_shift_code(int sx, int sy, int sz) { return ((sx + 4) * kCellShiftSpan + (sy + 4)) * kCellShiftSpan + (sz + 4); }
EGNN_HD void cell_shift_decode(int code, int* s) {
  s[0] = code / (kCellShiftSpan * kCellShiftSpan) - 4;
  s[1] = code / kCellShiftSpan % kCellShiftSpan - 4;
  s[2] = code % kCellShiftSpan - 4;
}
// the code of the sum of two shifts, -1 where a component leaves [-4, 4]
EGNN_HD int cell_shift_add(int code_a, int code_b) {
  int a[3], b[3];
  cell_shift_decode(code_a, a);
  cell_shift_decode(code_b, b);
  for (int k = 0; k < 3; ++k) {
    a[k] += b[k];
    if (a[k] < -4 || a[k] > 4) return -1;
  }
  return cell_shift_code(a[0], a[1], a[2]);
}

EGNN_HD double cell_delta(double wj, double wi, int s) { return (wj - wi) + (double)s; }
EGNN_HD void cell_cartesian(double d0, double d1, double d2, const double* L, double* r) {
  for (int x = 0; x < 3; ++x) r[x] = (d0 * L[x] + d1 * L[3 + x]) + d2 * L[6 + x];
}
EGNN_HD double cell_norm2(const double* r) { return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]; }

// vector from the wrapped centre (fractional wi) to site (wj, s)
EGNN_HD void cell_site_vector(const double* wj, const double* wi, const int* s, const double* L, double* r) {
  cell_cartesian(cell_delta(wj[0], wi[0], s[0]), cell_delta(wj[1], wi[1], s[1]), cell_delta(wj[2], wi[2], s[2]), L, r);
}

// the wrapped fractional coordinates of batch atom i
EGNN_HD void cell_wrapped_read(const double* frac, int i, double* w) {
  for (int k = 0; k < 3; ++k) w[k] = cell_wrap(frac[3 * (size_t)i + k]);
}

// whether entry (atom j, shift code) of a bond or site list names a site of the cell [lo, hi)
EGNN_HD bool cell_site_listed(int lo, int hi, int j, int code) { return j >= lo && j < hi && code >= 0 && code < kCellShiftCodes; }

// vector from the centre at wrapped wi to the site (j, code) of an entry that cell_site_listed has passed.  frac may be wrapped
// already: cell_wrap of a value in [0, 1) is that value.
EGNN_HD void cell_listed_vector(const double* frac, const double* L, const double* wi, int j, int code, double* r) {
  double wj[3];
  int s[3];
  cell_wrapped_read(frac, j, wj);
  cell_shift_decode(code, s);
  cell_site_vector(wj, wi, s, L, r);
}

// the test and the vector of a list entry in one: false, r untouched, where (j, code) names no site of the cell [lo, hi)
EGNN_HD bool cell_listed_site_vector(const double* frac, const double* L, int lo, int hi, const double* wi, int j, int code, double* r) {
  if (!cell_site_listed(lo, hi, j, code)) return false;
  cell_listed_vector(frac, L, wi, j, code, r);
  return true;
}

// perpendicular widths w_k =|det L| / |a_{k+1} x a_{k+2}|; false for a lattice that is singular (|det| <= 1e-9 |a||b||c|) or not
// finite
EGNN_HD bool cell_widths(const double* L, double* w) {
  const double* a = L;
  const double* b = L + 3;
  const double* c = L + 6;
  const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
  const double ca[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
  const double ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double det = fabs((a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2]);
  const double scale = sqrt(cell_norm2(a)) * sqrt(cell_norm2(b)) * sqrt(cell_norm2(c));
  if (!(scale < 1e300) || !(det > 1e-9 * scale)) return false;
  w[0] = det / sqrt(cell_norm2(bc));
  w[1] = det / sqrt(cell_norm2(ca));
  w[2] = det / sqrt(cell_norm2(ab));
  return true;
}

}  // namespace egnn

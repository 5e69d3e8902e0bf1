// Stand-alone run of egnn_cell_sites_host, egnn_cell_soap_host and egnn_cell_soap_mean_host (csrc/cells/cell_soap_host.cpp), built with
// -fsanitize=address,undefined by tests/test_cell_soap_host.py.  Every array has EXACTLY the size the contract states, so that ASan
// sees a write past a site row, a descriptor row, a coefficient block or a mean.  The tables are float64 stand-ins (beta = identity):
// the program checks memory and argument handling, the accuracy is test_cell_soap_host.py's business.
// Cases: the thin triclinic cell (image boxes 4 / 1 / 2 at cut 4.37) and a batch of it with a one-atom cell, every atom and a
// scrambled centre list with a repeat; the mean in one call and continued over two; every bad-argument case.
#include <math.h>
#include "../../diffusion_model_amd/csrc/cells/cell_soap_math.h"
#include "../../include/egnn_amd.h"
#include "cell_fixtures.h"

using namespace egnn;
using namespace cell_fixtures;

namespace {

std::vector<double> stand_in_tables(double r_cut, int n_max, int l_max, double sigma) {
  const int L1 = l_max + 1;
  const double a = 1.0 / (2.0 * sigma * sigma), pi = 3.14159265358979323846;
  std::vector<double> t((size_t)soap_table_count(n_max, l_max), 0.0);
  for (int n = 0; n < n_max; ++n)
    for (int l = 0; l < L1; ++l) {
      const double r = n_max > 1 ? 1.0 + (r_cut - 1.0) * n / (n_max - 1) : 1.0;
      const double alpha = -log(1e-3 / pow(r, l)) / (r * r), p = alpha + a;
      t[n * L1 + l] = pow(pi, 1.5) * pow(p, -1.5) * pow(a / p, l);
      t[soap_table_gamma(n_max, l_max) + n * L1 + l] = a * alpha / p;
    }
  for (int l = 0; l < L1; ++l)
    for (int n = 0; n < n_max; ++n) t[soap_table_beta(n_max, l_max) + (l * n_max + n) * n_max + n] = 1.0;
  for (int l = 0; l < L1; ++l) {
    for (int m = -l; m <= l; ++m) {
      const int am = m < 0 ? -m : m;
      t[soap_table_norm(n_max, l_max) + l * l + l + m] = sqrt((2 * l + 1) / (4 * pi) * factorial(l - am) / factorial(l + am)) * (m ? sqrt(2.0) : 1.0);
    }
    t[soap_table_weight(n_max, l_max) + l] = pi * sqrt(8.0 / (2 * l + 1));
  }
  return t;
}

// the two-call protocol: sizes, then lists of exactly the size learnt
void sites(const Cells& b, const std::vector<int32_t>& centres, std::vector<int32_t>& row_ptr, std::vector<int32_t>& atom,
           std::vector<int32_t>& code) {
  row_ptr.assign(centres.size() + 1, -7);
  int rc = egnn_cell_sites_host(b.C(), b.cell_ptr.data(), b.lattice.data(), b.frac.data(), kCut, (int)centres.size(), centres.data(),
                                row_ptr.data(), 0, nullptr, nullptr);
  CHECK(rc == 0, "rc %d: %s", rc, egnn_last_error());
  const int T = row_ptr.back();
  atom.assign((size_t)T, -7);
  code.assign((size_t)T, -7);
  rc = egnn_cell_sites_host(b.C(), b.cell_ptr.data(), b.lattice.data(), b.frac.data(), kCut, (int)centres.size(), centres.data(), row_ptr.data(),
                            T, T ? atom.data() : nullptr, T ? code.data() : nullptr);
  CHECK(rc == 0 && row_ptr.back() == T, "rc %d: %s", rc, egnn_last_error());
  for (size_t m = 0; m < centres.size(); ++m)
    for (int e = row_ptr[m]; e < row_ptr[m + 1]; ++e) {
      CHECK(atom[e] >= 0 && atom[e] < b.N() && code[e] >= 0 && code[e] < kCellShiftCodes, "row %zu entry %d: atom %d code %d", m, e, atom[e], code[e]);
      CHECK(!(atom[e] == centres[m] && code[e] == kCellCentreCode), "row %zu lists its centre", m);
      if (e > row_ptr[m])
        CHECK(atom[e] > atom[e - 1] || (atom[e] == atom[e - 1] && code[e] > code[e - 1]), "row %zu is not ascending at %d", m, e);
    }
}

std::vector<double> soap(const Cells& b, int A, const std::vector<double>& tables, const std::vector<int32_t>& centres, bool with_coeff) {
  const int F = soap_feature_count(A, 3, 2);
  std::vector<double> desc(centres.size() * (size_t)F, -7.0), coeff(with_coeff ? centres.size() * (size_t)A * 3 * 9 : 0, -7.0);
  const int rc = egnn_cell_soap_host(b.C(), A, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), 3, 2, kCut, tables.data(),
                                     (int)centres.size(), centres.data(), desc.data(), with_coeff ? coeff.data() : nullptr);
  CHECK(rc == 0, "rc %d: %s", rc, egnn_last_error());
  for (double v : desc) CHECK(isfinite(v) && v != -7.0, "a descriptor entry was not written");
  for (double v : coeff) CHECK(isfinite(v) && v != -7.0, "a coefficient was not written");
  return desc;
}

}  // namespace

int main() {
  seed(97531);
  const std::vector<double> tables = stand_in_tables(4.0, 3, 2, 0.1);
  Cells thin, mixed;
  add_cell(thin, kThin, 12, 3);
  add_cell(mixed, kCube, 1, 3);
  add_cell(mixed, kThin, 12, 3);
  add_cell(mixed, kCube, 1, 3);
  {   // the image box of the thin cell
    int b[3];
    double w[3];
    CHECK(cell_soap_box(kThin, kCut, b, w) && b[0] == 4 && b[1] == 1 && b[2] == 2, "box %d %d %d", b[0], b[1], b[2]);
    CHECK(cell_soap_box_count(b) == 9 * 3 * 5, "box count");
    int s[3];
    cell_soap_box_shift(0, b, s);
    CHECK(s[0] == -4 && s[1] == -1 && s[2] == -2, "first shift");
    cell_soap_box_shift(9 * 3 * 5 - 1, b, s);
    CHECK(s[0] == 4 && s[1] == 1 && s[2] == 2, "last shift");
  }
  std::vector<int32_t> row_ptr, atom, code, all(12), scrambled = {7, 0, 11, 3, 7};
  for (int i = 0; i < 12; ++i) all[i] = i;
  sites(thin, all, row_ptr, atom, code);
  CHECK(row_ptr.back() > 12 * 100, "the thin cell: %d sites", row_ptr.back());
  const std::vector<int32_t> rows_all = row_ptr, atom_all = atom, code_all = code;
  sites(thin, scrambled, row_ptr, atom, code);
  for (size_t m = 0; m < scrambled.size(); ++m) {
    const int i = scrambled[m], len = rows_all[i + 1] - rows_all[i];
    CHECK(row_ptr[m + 1] - row_ptr[m] == len, "listed centre %zu: row length", m);
    for (int e = 0; e < len; ++e)
      CHECK(atom[row_ptr[m] + e] == atom_all[rows_all[i] + e] && code[row_ptr[m] + e] == code_all[rows_all[i] + e], "listed centre %zu entry %d", m, e);
  }
  {   // the one-atom cells of the mixed batch: no site at this cut (5 A > 4.37 A); the thin cell in the middle keeps its rows
    std::vector<int32_t> every(14);
    for (int i = 0; i < 14; ++i) every[i] = i;
    sites(mixed, every, row_ptr, atom, code);
    CHECK(row_ptr[1] == 0 && row_ptr[14] == row_ptr[13], "one-atom cells: %d and %d sites", row_ptr[1], row_ptr[14] - row_ptr[13]);
    for (int e = row_ptr[1]; e < row_ptr[13]; ++e) CHECK(atom[e] >= 1 && atom[e] < 13, "a site outside its cell: %d", atom[e]);
    // with a cut above 5 A the atom sees its own images only
    row_ptr.assign(2, -7);
    const int32_t lone = 0, ptr1[2] = {0, 1};
    int rc = egnn_cell_sites_host(1, ptr1, kCube, mixed.frac.data(), 8.37, 1, &lone, row_ptr.data(), 0, nullptr, nullptr);
    CHECK(rc == 0 && row_ptr[1] == 18, "one atom at 8.37 A: %d sites (6 + 12)", row_ptr[1]);
  }
  const int F = soap_feature_count(3, 3, 2);
  const std::vector<double> d_all = soap(thin, 3, tables, all, true);
  const std::vector<double> d_some = soap(thin, 3, tables, scrambled, false);
  for (size_t m = 0; m < scrambled.size(); ++m)
    for (int f = 0; f < F; ++f) CHECK(d_some[m * F + f] == d_all[(size_t)scrambled[m] * F + f], "centre %zu feature %d", m, f);
  {   // a cell gives the same bits in any batch
    std::vector<int32_t> middle(12);
    for (int i = 0; i < 12; ++i) middle[i] = 1 + i;
    Cells again;   // the same thin cell as `mixed` holds: the generator state differs from `thin`, so build it alone too
    again.cell_ptr = {0, 12};
    again.lattice.assign(mixed.lattice.begin() + 9, mixed.lattice.begin() + 18);
    again.frac.assign(mixed.frac.begin() + 3, mixed.frac.begin() + 39);
    again.type.assign(mixed.type.begin() + 1, mixed.type.begin() + 13);
    const std::vector<double> in_batch = soap(mixed, 3, tables, middle, false), alone = soap(again, 3, tables, all, false);
    for (size_t o = 0; o < alone.size(); ++o) CHECK(in_batch[o] == alone[o], "entry %zu differs in the batch", o);
    const std::vector<int32_t> lone = {0, 13};
    const std::vector<double> d = soap(mixed, 3, tables, lone, true);
    int nonzero = 0;
    for (int f = 0; f < F; ++f) nonzero += d[f] != 0.0;
    CHECK(nonzero == 6, "an atom without a site: %d non-zero entries", nonzero);   // n <= n' of 3, l = 0, one species block
  }
  {   // the mean: one call, and the same continued over two
    const int32_t rows[2] = {0, 12}, first_half[2] = {0, 5}, second_half[2] = {0, 7};
    const int64_t count[1] = {12};
    std::vector<double> once((size_t)F, -7.0), twice((size_t)F, -7.0);
    CHECK(egnn_cell_soap_mean_host(1, F, rows, d_all.data(), count, 1, 1, once.data()) == 0, "%s", egnn_last_error());
    CHECK(egnn_cell_soap_mean_host(1, F, first_half, d_all.data(), nullptr, 1, 0, twice.data()) == 0, "%s", egnn_last_error());
    CHECK(egnn_cell_soap_mean_host(1, F, second_half, d_all.data() + (size_t)5 * F, count, 0, 1, twice.data()) == 0, "%s", egnn_last_error());
    for (int f = 0; f < F; ++f) {
      double acc = 0.0;
      for (int m = 0; m < 12; ++m) acc += d_all[(size_t)m * F + f];
      CHECK(once[f] == acc / 12.0 && twice[f] == once[f], "mean of feature %d", f);
    }
    const int32_t two[3] = {0, 0, 12};   // a cell without a centre: zeros
    const int64_t counts[2] = {0, 12};
    std::vector<double> both((size_t)2 * F, -7.0);
    CHECK(egnn_cell_soap_mean_host(2, F, two, d_all.data(), counts, 1, 1, both.data()) == 0, "%s", egnn_last_error());
    for (int f = 0; f < F; ++f) CHECK(both[f] == 0.0 && both[(size_t)F + f] == once[f], "two cells, feature %d", f);
  }
  {   // bad arguments
    std::vector<int32_t> c = {0}, rp(2, -7);
    std::vector<double> desc((size_t)F, 0.0);
    auto run = [&](const Cells& b, int A, int n_max, int l_max, double cut, const double* t, double* out) {
      return egnn_cell_soap_host(b.C(), A, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), n_max, l_max, cut, t, 1, c.data(),
                                 out, nullptr);
    };
    CHECK(run(thin, 3, 3, 2, kCut, tables.data(), desc.data()) == 0, "the good call");
    CHECK(run(thin, 5, 3, 2, kCut, tables.data(), desc.data()) == EGNN_EINVAL, "A = 5");
    CHECK(run(thin, 3, 17, 2, kCut, tables.data(), desc.data()) == EGNN_EINVAL, "n_max = 17");
    CHECK(run(thin, 3, 3, 11, kCut, tables.data(), desc.data()) == EGNN_EINVAL, "l_max = 11");
    CHECK(run(thin, 3, 3, 2, 0.0, tables.data(), desc.data()) == EGNN_EINVAL, "cut = 0");
    CHECK(run(thin, 3, 3, 2, NAN, tables.data(), desc.data()) == EGNN_EINVAL, "cut = NaN");
    CHECK(run(thin, 3, 3, 2, INFINITY, tables.data(), desc.data()) == EGNN_EINVAL, "cut = inf");
    CHECK(run(thin, 3, 3, 2, 5.3, tables.data(), desc.data()) == EGNN_EINVAL, "a width below cut / 4");
    CHECK(run(thin, 3, 3, 2, kCut, nullptr, desc.data()) == EGNN_EINVAL, "no tables");
    CHECK(run(thin, 3, 3, 2, kCut, tables.data(), nullptr) == EGNN_EINVAL, "no desc");
    CHECK(run(thin, 2, 3, 2, kCut, tables.data(), desc.data()) == EGNN_EINVAL, "a type outside [0, A)");
    c[0] = 12;
    CHECK(run(thin, 3, 3, 2, kCut, tables.data(), desc.data()) == EGNN_EINVAL, "centre N");
    c[0] = -1;
    CHECK(run(thin, 3, 3, 2, kCut, tables.data(), desc.data()) == EGNN_EINVAL, "centre -1");
    c[0] = 0;
    Cells flat = thin;
    for (int k = 0; k < 3; ++k) flat.lattice[6 + k] = 2.0 * flat.lattice[k];   // c = 2 a: singular
    CHECK(run(flat, 3, 3, 2, kCut, tables.data(), desc.data()) == EGNN_EINVAL, "a singular lattice");
    CHECK(egnn_cell_sites_host(1, flat.cell_ptr.data(), flat.lattice.data(), flat.frac.data(), kCut, 1, c.data(), rp.data(), 0, nullptr, nullptr) ==
              EGNN_EINVAL, "a singular lattice, sites");
    CHECK(egnn_cell_sites_host(1, thin.cell_ptr.data(), thin.lattice.data(), thin.frac.data(), 5.3, 1, c.data(), rp.data(), 0, nullptr, nullptr) ==
              EGNN_EINVAL, "a width below cut / 4, sites");
    Cells bad = thin;
    bad.frac[4] = NAN;
    CHECK(run(bad, 3, 3, 2, kCut, tables.data(), desc.data()) == EGNN_EINVAL, "a coordinate that is not finite");
    const int32_t down[3] = {0, 5, 3};
    const int64_t counts[2] = {5, 0};
    CHECK(egnn_cell_soap_mean_host(2, F, down, d_all.data(), counts, 1, 1, desc.data()) == EGNN_EINVAL, "cell_rows decreases");
  }
  printf("CELL-SOAP-OK\n");
  return 0;
}

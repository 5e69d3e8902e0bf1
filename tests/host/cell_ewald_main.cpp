// Stand-alone run of egnn_cell_ewald_host (csrc/cells/cell_ewald_host.cpp), built with -fsanitize=address,undefined by
// tests/test_cell_ewald_host.py.  Every array has EXACTLY the size the contract states, so that ASan sees a write past a row of
// components, a force or a count.  The program checks memory and argument handling; the accuracy is test_cell_ewald_host.py's
// business.  Cases: the thin triclinic cell (image boxes 4 / 1 / 2 at 4.37 A) alone and in a batch with one-atom cells, with and
// without forces, the optional outputs, the pair tables and the charges; a cell with coincident atoms; every bad-argument case.
#include <math.h>
#include "../../include/egnn_amd.h"
#include "cell_fixtures.h"

using namespace cell_fixtures;

namespace {

struct Model {
  std::vector<double> charges, pot;
  int n = 12, shift = 1;
  double kappa = 14.3996454784, alpha = 0.85, r_cut = kCut, short_cut = 3.0, k_max = 6.3;
};

Model model(int A, bool with_pot) {
  Model m;
  for (int a = 0; a < A; ++a) m.charges.push_back(a == 2 ? 0.0 : (a ? 2.3 : -1.1));
  if (with_pot) {
    m.pot.assign(4 * A * A, 0.0);
    for (int t = 0; t < 4; ++t)
      for (int a = 0; a < A; ++a)
        for (int b = 0; b < A; ++b) m.pot[(t * A + a) * A + b] = (t == 0 ? 400.0 : t == 1 ? 2.5 : t == 2 ? 10.0 : 0.1) * (1.0 + 0.1 * (a + b));
  }
  return m;
}

struct Result {
  std::vector<double> energy, components, e_atom, comp_atom, force;
  std::vector<int32_t> n_sites, coincident;
  std::vector<int64_t> n_vectors;
};

int call(const Cells& b, int A, const Model& m, bool forces, bool optional, Result* r) {
  const size_t C = b.C(), N = b.N();
  r->energy.assign(C, -7.0);
  r->components.assign(5 * C, -7.0);
  r->e_atom.assign(N, -7.0);
  r->comp_atom.assign(optional ? 5 * N : 0, -7.0);
  r->force.assign(forces ? 3 * N : 0, -7.0);
  r->n_sites.assign(optional ? N : 0, -7);
  r->coincident.assign(C, -7);
  r->n_vectors.assign(C, -7);
  return egnn_cell_ewald_host(b.C(), A, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), m.charges.data(),
                              m.pot.empty() ? nullptr : m.pot.data(), m.n, m.shift, m.kappa, m.alpha, m.r_cut, m.short_cut, m.k_max, forces,
                              r->energy.data(), r->components.data(), r->e_atom.data(), optional ? r->comp_atom.data() : nullptr,
                              forces ? r->force.data() : nullptr, optional ? r->n_sites.data() : nullptr, r->n_vectors.data(),
                              r->coincident.data());
}

Result run(const Cells& b, int A, const Model& m, bool forces, bool optional) {
  Result r;
  const int rc = call(b, A, m, forces, optional, &r);
  CHECK(rc == 0, "rc %d: %s", rc, egnn_last_error());
  for (const std::vector<double>* v : {&r.energy, &r.components, &r.e_atom, &r.comp_atom, &r.force})
    for (double x : *v) CHECK(isfinite(x) && x != -7.0, "an output was not written");
  for (int32_t x : r.n_sites) CHECK(x >= 0, "a site count was not written");
  for (size_t c = 0; c < r.coincident.size(); ++c) CHECK(r.n_vectors[c] >= 0 && (r.coincident[c] == 0 || r.coincident[c] == 1), "cell %zu", c);
  return r;
}

}  // namespace

int main() {
  seed(13579);
  Cells thin, mixed;
  add_cell(thin, kThin, 12, 3);
  add_cell(mixed, kCube, 1, 3);
  add_cell(mixed, kThin, 12, 3);
  add_cell(mixed, kCube, 1, 3);
  for (bool with_pot : {true, false}) {
    const Model m = model(3, with_pot);
    const Result full = run(thin, 3, m, true, true), bare = run(thin, 3, m, false, false);
    CHECK(full.n_vectors[0] > 20 && full.coincident[0] == 0, "the thin cell: %lld vectors", (long long)full.n_vectors[0]);
    for (int i = 0; i < 12; ++i) CHECK(full.n_sites[i] > 200, "the thin cell: atom %d has %d sites", i, full.n_sites[i]);
    for (int i = 0; i < 12; ++i) CHECK(bare.e_atom[i] == full.e_atom[i], "forces change the energy of atom %d", i);
    CHECK((full.components[4] != 0.0) == with_pot, "the short component");
    Cells again;   // a cell gives the same bits in any batch
    again.cell_ptr = {0, 12};
    again.lattice.assign(mixed.lattice.begin() + 9, mixed.lattice.begin() + 18);
    again.frac.assign(mixed.frac.begin() + 3, mixed.frac.begin() + 39);
    again.type.assign(mixed.type.begin() + 1, mixed.type.begin() + 13);
    const Result in_batch = run(mixed, 3, m, true, true), alone = run(again, 3, m, true, true);
    for (size_t k = 0; k < alone.force.size(); ++k) CHECK(in_batch.force[3 + k] == alone.force[k], "force entry %zu differs in the batch", k);
    for (int k = 0; k < 5; ++k) CHECK(in_batch.components[5 + k] == alone.components[k], "component %d differs in the batch", k);
    CHECK(in_batch.energy[1] == alone.energy[0] && in_batch.n_sites[0] == 0 && in_batch.n_sites[13] == 0, "the batch");
  }
  {   // no charge: no reciprocal part
    Model m = model(3, true);
    m.charges.assign(3, 0.0);
    const Result r = run(thin, 3, m, true, true);
    CHECK(r.n_vectors[0] == 0 && r.components[0] == 0.0 && r.components[1] == 0.0 && r.components[4] != 0.0, "zero charges");
  }
  {   // coincident atoms are flagged, the cell beside them is not
    Cells b;
    b.add(5.0, {0.25, 0.5, 0.75, 0.6, 0.1, 0.7}, {0, 1});
    b.add(5.0, {0.25, 0.5, 0.75, 0.6, 0.1, 0.7, 1.25, 0.5, 0.75}, {0, 1, 0});
    Model m = model(2, true);
    m.r_cut = 6.0;
    const Result r = run(b, 2, m, true, true);
    CHECK(r.coincident[0] == 0 && r.coincident[1] == 1, "flags %d %d", r.coincident[0], r.coincident[1]);
  }
  {   // bad arguments
    Result r;
    const Model good = model(3, true);
    CHECK(call(thin, 3, good, true, true, &r) == 0, "the good call: %s", egnn_last_error());
    auto bad = [&](const char* what, void (*change)(Model&)) {
      Model m = good;
      change(m);
      CHECK(call(thin, 3, m, true, true, &r) == EGNN_EINVAL, "%s", what);
    };
    bad("short_cut above r_cut", [](Model& m) { m.short_cut = 4.38; });
    bad("short_cut = 0", [](Model& m) { m.short_cut = 0.0; });
    bad("alpha = NaN", [](Model& m) { m.alpha = NAN; });
    bad("k_max = inf", [](Model& m) { m.k_max = INFINITY; });
    bad("kappa = -1", [](Model& m) { m.kappa = -1.0; });
    bad("n = 0", [](Model& m) { m.n = 0; });
    bad("n = 65", [](Model& m) { m.n = 65; });
    bad("a width below r_cut / 4", [](Model& m) { m.r_cut = 5.3; });
    bad("an index need above the limit", [](Model& m) { m.k_max = 6000.0; });
    bad("a charge that is not finite", [](Model& m) { m.charges[1] = INFINITY; });
    bad("a table that is not finite", [](Model& m) { m.pot[1] = m.pot[3] = NAN; });
    bad("a table that is not symmetric", [](Model& m) { m.pot[1] += 1.0; });
    CHECK(call(thin, 5, good, true, true, &r) == EGNN_EINVAL, "A = 5");
    CHECK(call(thin, 2, model(2, true), true, true, &r) == EGNN_EINVAL, "a type outside [0, A)");
    Cells flat = thin;
    for (int k = 0; k < 3; ++k) flat.lattice[6 + k] = 2.0 * flat.lattice[k];   // c = 2 a: singular
    CHECK(call(flat, 3, good, true, true, &r) == EGNN_EINVAL, "a singular lattice");
    Cells nan = thin;
    nan.frac[4] = NAN;
    CHECK(call(nan, 3, good, true, true, &r) == EGNN_EINVAL, "a coordinate that is not finite");
  }
  printf("CELL-EWALD-OK\n");
  return 0;
}

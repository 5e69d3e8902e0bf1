// Stand-alone run of egnn_cell_ewald_virial_host (csrc/cells/cell_stress_host.cpp), built with -fsanitize=address,undefined by
// tests/test_cell_stress_host.py.  Every array has EXACTLY the size the contract states, so that ASan sees a write past a row of
// six, a block of components or a count.  The program checks memory and argument handling; the accuracy is
// test_cell_stress_host.py's business.  Cases: the thin triclinic cell (image boxes 4 / 1 / 2 at 4.37 A) alone and in a batch with
// one-atom cells, with and without the optional output, the pair tables and the charges; a cell with coincident atoms; every
// bad-argument case.
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
  std::vector<double> strain, components, per_atom, comp_atom, stress, pressure;
  std::vector<int32_t> coincident;
  std::vector<int64_t> n_vectors;
};

int call(const Cells& b, int A, const Model& m, bool optional, Result* r) {
  const size_t C = b.C(), N = b.N();
  r->strain.assign(6 * C, -7.0);
  r->components.assign(30 * C, -7.0);
  r->per_atom.assign(6 * N, -7.0);
  r->comp_atom.assign(optional ? 30 * N : 0, -7.0);
  r->stress.assign(6 * C, -7.0);
  r->pressure.assign(C, -7.0);
  r->coincident.assign(C, -7);
  r->n_vectors.assign(C, -7);
  return egnn_cell_ewald_virial_host(b.C(), A, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), m.charges.data(),
                                     m.pot.empty() ? nullptr : m.pot.data(), m.n, m.shift, m.kappa, m.alpha, m.r_cut, m.short_cut, m.k_max,
                                     r->strain.data(), r->components.data(), r->per_atom.data(), optional ? r->comp_atom.data() : nullptr,
                                     r->stress.data(), r->pressure.data(), r->n_vectors.data(), r->coincident.data());
}

Result run(const Cells& b, int A, const Model& m, bool optional) {
  Result r;
  const int rc = call(b, A, m, optional, &r);
  CHECK(rc == 0, "rc %d: %s", rc, egnn_last_error());
  for (const std::vector<double>* v : {&r.strain, &r.components, &r.per_atom, &r.comp_atom, &r.stress, &r.pressure})
    for (double x : *v) CHECK(isfinite(x) && x != -7.0, "an output was not written");
  for (size_t c = 0; c < r.coincident.size(); ++c) CHECK(r.n_vectors[c] >= 0 && (r.coincident[c] == 0 || r.coincident[c] == 1), "cell %zu", c);
  return r;
}

}  // namespace

int main() {
  seed(24680);
  Cells thin, mixed;
  add_cell(thin, kThin, 12, 3);
  seed(24680);
  add_cell(mixed, kCube, 1, 3);
  seed(24680);
  add_cell(mixed, kThin, 12, 3);   // the atoms of `thin` again
  add_cell(mixed, kCube, 1, 3);
  for (bool with_pot : {true, false}) {
    const Model m = model(3, with_pot);
    const Result full = run(thin, 3, m, true), bare = run(thin, 3, m, false);
    CHECK(full.n_vectors[0] > 20 && full.coincident[0] == 0, "the thin cell: %lld vectors", (long long)full.n_vectors[0]);
    for (size_t k = 0; k < full.per_atom.size(); ++k) CHECK(bare.per_atom[k] == full.per_atom[k], "the optional output changes entry %zu", k);
    for (int v = 0; v < 6; ++v) {
      CHECK((full.components[24 + v] != 0.0) == with_pot, "the short component %d", v);
      CHECK(full.components[12 + v] == 0.0, "the self component %d", v);
      CHECK(full.stress[v] != 0.0, "stress %d", v);
    }
    CHECK(full.pressure[0] == -(((full.stress[0] + full.stress[1]) + full.stress[2]) / 3.0), "the pressure");
    const Result in_batch = run(mixed, 3, m, true);   // a cell gives the same bits in any batch
    for (size_t k = 0; k < full.per_atom.size(); ++k) CHECK(in_batch.per_atom[6 + k] == full.per_atom[k], "entry %zu differs in the batch", k);
    for (int k = 0; k < 30; ++k) CHECK(in_batch.components[30 + k] == full.components[k], "component %d differs in the batch", k);
    for (int v = 0; v < 6; ++v) CHECK(in_batch.strain[6 + v] == full.strain[v] && in_batch.stress[6 + v] == full.stress[v], "the batch, %d", v);
    CHECK(in_batch.pressure[1] == full.pressure[0], "the pressure in the batch");
  }
  {   // no charge: no reciprocal part
    Model m = model(3, true);
    m.charges.assign(3, 0.0);
    const Result r = run(thin, 3, m, true);
    CHECK(r.n_vectors[0] == 0 && r.components[0] == 0.0 && r.components[6] == 0.0 && r.components[24] != 0.0, "zero charges");
  }
  {   // coincident atoms are flagged, the cell beside them is not
    Cells b;
    b.add(5.0, {0.25, 0.5, 0.75, 0.6, 0.1, 0.7}, {0, 1});
    b.add(5.0, {0.25, 0.5, 0.75, 0.6, 0.1, 0.7, 1.25, 0.5, 0.75}, {0, 1, 0});
    Model m = model(2, true);
    m.r_cut = 6.0;
    const Result r = run(b, 2, m, true);
    CHECK(r.coincident[0] == 0 && r.coincident[1] == 1, "flags %d %d", r.coincident[0], r.coincident[1]);
  }
  {   // bad arguments
    Result r;
    const Model good = model(3, true);
    CHECK(call(thin, 3, good, true, &r) == 0, "the good call: %s", egnn_last_error());
    auto bad = [&](const char* what, void (*change)(Model&)) {
      Model m = good;
      change(m);
      CHECK(call(thin, 3, m, true, &r) == EGNN_EINVAL, "%s", what);
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
    CHECK(call(thin, 5, good, true, &r) == EGNN_EINVAL, "A = 5");
    CHECK(call(thin, 2, model(2, true), true, &r) == EGNN_EINVAL, "a type outside [0, A)");
    CHECK(egnn_cell_ewald_virial_host(1, 3, thin.cell_ptr.data(), thin.lattice.data(), thin.frac.data(), thin.type.data(), good.charges.data(),
                                      good.pot.data(), good.n, good.shift, good.kappa, good.alpha, good.r_cut, good.short_cut, good.k_max,
                                      r.strain.data(), r.components.data(), r.per_atom.data(), nullptr, nullptr, r.pressure.data(),
                                      r.n_vectors.data(), r.coincident.data()) == EGNN_EINVAL, "stress = NULL");
    Cells flat = thin;
    for (int k = 0; k < 3; ++k) flat.lattice[6 + k] = 2.0 * flat.lattice[k];   // c = 2 a: singular
    CHECK(call(flat, 3, good, true, &r) == EGNN_EINVAL, "a singular lattice");
    Cells nan = thin;
    nan.frac[4] = NAN;
    CHECK(call(nan, 3, good, true, &r) == EGNN_EINVAL, "a coordinate that is not finite");
  }
  printf("CELL-STRESS-OK\n");
  return 0;
}

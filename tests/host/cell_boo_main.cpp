// Stand-alone run of egnn_cell_boo_host (csrc/cells/cell_boo_host.cpp), built with -fsanitize=address,undefined by
// tests/test_cell_boo_host.py.  Every array has EXACTLY the size the contract states, so that ASan sees a write past a row of
// invariants, a count or a q_lm row.  The tables are float64 stand-ins (N_lm from libm, G^l a few entries at the ends of the index
// range): the program checks memory and argument handling, the accuracy is test_cell_boo_host.py's business.
// Cases: the thin triclinic cell (image boxes 4 / 1 / 2 at 4.37 A) alone and in a batch with one-atom cells, every atom and a
// scrambled centre list with a repeat, with and without the averages and q_lm, l_max = 0, 4 and 10; every bad-argument case.
#include <math.h>
#include "../../diffusion_model_amd/csrc/cells/cell_boo_math.h"
#include "../../include/egnn_amd.h"
#include "cell_fixtures.h"

using namespace egnn;
using namespace cell_fixtures;

namespace {

struct Tables {
  std::vector<double> norm, val;
  std::vector<int32_t> off, idx;
  int E() const { return (int)val.size(); }
};

Tables stand_in_tables(int l_max) {
  const double pi = 3.14159265358979323846;
  Tables t;
  for (int l = 0; l <= l_max; ++l)
    for (int m = -l; m <= l; ++m) {
      const int am = m < 0 ? -m : m;
      t.norm.push_back(sqrt((2 * l + 1) / (4 * pi) * factorial(l - am) / factorial(l + am)) * (m ? sqrt(2.0) : 1.0));
    }
  t.off.push_back(0);
  for (int l = 0; l <= l_max; ++l) {
    if (l % 2 == 0) {
      const int32_t rows[3][3] = {{0, 0, 0}, {0, l, 2 * l}, {2 * l, 2 * l, 2 * l}};
      for (const auto& r : rows) {
        for (int k = 0; k < 3; ++k) t.idx.push_back(r[k]);
        t.val.push_back(0.25 + 0.125 * l);
      }
    }
    t.off.push_back(t.E());
  }
  return t;
}

struct Result {
  std::vector<double> out, qlm;
  std::vector<int32_t> n, n_solid;
};

Result boo(const Cells& b, int A, unsigned select, int l_max, const Tables& t, double cut, const std::vector<int32_t>& centres, bool averaged,
           bool with_qlm) {
  const size_t M = centres.size(), L1 = l_max + 1;
  Result r;
  r.out.assign(M * (averaged ? 6 : 3) * L1, -7.0);
  r.qlm.assign(with_qlm ? M * L1 * L1 : 0, -7.0);
  r.n.assign(M, -7);
  r.n_solid.assign(M, -7);
  const int rc = egnn_cell_boo_host(b.C(), A, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), cut, select, l_max, t.norm.data(),
                                    t.E(), t.off.data(), t.idx.data(), t.val.data(), l_max < 4 ? l_max : 4, 0.5, averaged, (int)M, centres.data(),
                                    r.out.data(), r.n.data(), r.n_solid.data(), with_qlm ? r.qlm.data() : nullptr);
  CHECK(rc == 0, "rc %d: %s", rc, egnn_last_error());
  for (double v : r.out) CHECK(isfinite(v) && v != -7.0, "an invariant was not written");
  for (double v : r.qlm) CHECK(isfinite(v) && v != -7.0, "a q_lm was not written");
  for (size_t m = 0; m < M; ++m) CHECK(r.n[m] >= 0 && r.n_solid[m] >= 0 && r.n_solid[m] <= r.n[m], "row %zu: n %d, n_solid %d", m, r.n[m], r.n_solid[m]);
  return r;
}

}  // namespace

int main() {
  seed(24680);
  Cells thin, mixed;
  add_cell(thin, kThin, 12, 3);
  add_cell(mixed, kCube, 1, 3);
  add_cell(mixed, kThin, 12, 3);
  add_cell(mixed, kCube, 1, 3);
  std::vector<int32_t> all(12), scrambled = {7, 0, 11, 3, 7};
  for (int i = 0; i < 12; ++i) all[i] = i;
  const unsigned every = 0x1ff, some = 0x1a5;   // 3 x 3 type pairs: all, and a mask with holes
  for (int l_max : {0, 4, 10}) {
    const Tables t = stand_in_tables(l_max);
    const size_t L1 = l_max + 1, LM = L1 * L1;
    const Result full = boo(thin, 3, every, l_max, t, kCut, all, true, true);
    for (int i = 0; i < 12; ++i) CHECK(full.n[i] > 40, "the thin cell: atom %d has %d sites", i, full.n[i]);
    for (int i = 0; i < 12; ++i) CHECK(fabs(full.out[(size_t)i * 6 * L1] - 1.0) < 1e-12, "q_0 of atom %d is %.17g", i, full.out[(size_t)i * 6 * L1]);
    const Result part = boo(thin, 3, some, l_max, t, kCut, all, true, false);
    for (int i = 0; i < 12; ++i) CHECK(part.n[i] <= full.n[i], "select keeps more than all");
    const Result plain = boo(thin, 3, every, l_max, t, kCut, all, false, false);
    for (int i = 0; i < 12; ++i)
      for (size_t k = 0; k < 3 * L1; ++k) CHECK(plain.out[i * 3 * L1 + k] == full.out[i * 6 * L1 + k], "averaged changes the own invariants");
    const Result listed = boo(thin, 3, every, l_max, t, kCut, scrambled, true, true);
    for (size_t m = 0; m < scrambled.size(); ++m) {
      const size_t i = scrambled[m];
      CHECK(listed.n[m] == full.n[i] && listed.n_solid[m] == full.n_solid[i], "listed centre %zu: counts", m);
      for (size_t k = 0; k < 6 * L1; ++k) CHECK(listed.out[m * 6 * L1 + k] == full.out[i * 6 * L1 + k], "listed centre %zu entry %zu", m, k);
      for (size_t k = 0; k < LM; ++k) CHECK(listed.qlm[m * LM + k] == full.qlm[i * LM + k], "listed centre %zu q_lm %zu", m, k);
    }
    {   // a cell gives the same bits in any batch; the one-atom cells have no site at this cutoff
      std::vector<int32_t> everyone(14);
      for (int i = 0; i < 14; ++i) everyone[i] = i;
      Cells again;
      again.cell_ptr = {0, 12};
      again.lattice.assign(mixed.lattice.begin() + 9, mixed.lattice.begin() + 18);
      again.frac.assign(mixed.frac.begin() + 3, mixed.frac.begin() + 39);
      again.type.assign(mixed.type.begin() + 1, mixed.type.begin() + 13);
      const Result in_batch = boo(mixed, 3, every, l_max, t, kCut, everyone, true, true), alone = boo(again, 3, every, l_max, t, kCut, all, true, true);
      for (size_t o = 0; o < alone.out.size(); ++o) CHECK(in_batch.out[6 * L1 + o] == alone.out[o], "entry %zu differs in the batch", o);
      CHECK(in_batch.n[0] == 0 && in_batch.n[13] == 0, "one-atom cells: %d and %d sites", in_batch.n[0], in_batch.n[13]);
      for (size_t k = 0; k < 6 * L1; ++k) CHECK(in_batch.out[k] == 0.0, "an atom without a site: entry %zu", k);
      const std::vector<int32_t> lone = {0};
      Cells cube;
      add_cell(cube, kCube, 1, 3);
      const Result images = boo(cube, 3, every, l_max, t, 5.5, lone, true, false);   // its own six images
      CHECK(images.n[0] == 6, "one atom at 5.5 A: %d sites", images.n[0]);
    }
    boo(thin, 3, every, l_max, t, kCut, {}, true, false);   // no centre: nothing is written
  }
  {   // bad arguments
    const Tables t = stand_in_tables(4);
    std::vector<int32_t> c = {0}, n(1), ns(1);
    std::vector<double> out(6 * 5, 0.0);
    auto run = [&](const Cells& b, int A, unsigned select, int l_max, int l_solid, double cut, const Tables& tab) {
      return egnn_cell_boo_host(b.C(), A, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), cut, select, l_max, tab.norm.data(),
                                tab.E(), tab.off.data(), tab.idx.data(), tab.val.data(), l_solid, 0.7, 1, 1, c.data(), out.data(), n.data(), ns.data(),
                                nullptr);
    };
    CHECK(run(thin, 3, 0x1ff, 4, 4, kCut, t) == 0, "the good call: %s", egnn_last_error());
    CHECK(run(thin, 5, 0x1ff, 4, 4, kCut, t) == EGNN_EINVAL, "A = 5");
    CHECK(run(thin, 3, 0x3ff, 4, 4, kCut, t) == EGNN_EINVAL, "a select bit beyond A x A");
    CHECK(run(thin, 3, 0x1ff, 11, 4, kCut, t) == EGNN_EINVAL, "l_max = 11");
    CHECK(run(thin, 3, 0x1ff, -1, 0, kCut, t) == EGNN_EINVAL, "l_max = -1");
    CHECK(run(thin, 3, 0x1ff, 4, 5, kCut, t) == EGNN_EINVAL, "l_solid above l_max");
    CHECK(run(thin, 3, 0x1ff, 4, -1, kCut, t) == EGNN_EINVAL, "l_solid = -1");
    CHECK(run(thin, 3, 0x1ff, 4, 4, 0.0, t) == EGNN_EINVAL, "cutoff = 0");
    CHECK(run(thin, 3, 0x1ff, 4, 4, NAN, t) == EGNN_EINVAL, "cutoff = NaN");
    CHECK(run(thin, 3, 0x1ff, 4, 4, INFINITY, t) == EGNN_EINVAL, "cutoff = inf");
    CHECK(run(thin, 3, 0x1ff, 4, 4, 5.3, t) == EGNN_EINVAL, "a width below cutoff / 4");
    CHECK(run(thin, 2, 0xf, 4, 4, kCut, t) == EGNN_EINVAL, "a type outside [0, A)");
    Tables broken = t;
    broken.off[2] = broken.off[3] + 1;
    CHECK(run(thin, 3, 0x1ff, 4, 4, kCut, broken) == EGNN_EINVAL, "g_off decreases");
    c[0] = 12;
    CHECK(run(thin, 3, 0x1ff, 4, 4, kCut, t) == EGNN_EINVAL, "centre N");
    c[0] = -1;
    CHECK(run(thin, 3, 0x1ff, 4, 4, kCut, t) == EGNN_EINVAL, "centre -1");
    c[0] = 0;
    Cells flat = thin;
    for (int k = 0; k < 3; ++k) flat.lattice[6 + k] = 2.0 * flat.lattice[k];   // c = 2 a: singular
    CHECK(run(flat, 3, 0x1ff, 4, 4, kCut, t) == EGNN_EINVAL, "a singular lattice");
    Cells bad = thin;
    bad.frac[4] = NAN;
    CHECK(run(bad, 3, 0x1ff, 4, 4, kCut, t) == EGNN_EINVAL, "a coordinate that is not finite");
  }
  printf("CELL-BOO-OK\n");
  return 0;
}

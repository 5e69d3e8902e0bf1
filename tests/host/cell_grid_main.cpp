// Stand-alone run of egnn_cell_grid_dims and egnn_cell_grid_host (csrc/cells/cell_grid_host.cpp), built with
// -fsanitize=address,undefined by tests/test_cell_grid_host.py.  Every output array is allocated at EXACTLY its documented size, so
// that ASan sees a write past a bin table or a bond row: ideal beta-cristobalite (nb = 3, every neighbour bin wraps; 64 bonds; the
// pair totals of [0, 2.3) through the walk), a one-atom 7 A cell (no bond; 13 bins per axis at reach 3 and nothing within 1.5 A), an
// empty cell alone and beside cristobalite, and refused arguments, which leave the lists alone.
#include <math.h>
#include "../../diffusion_model_amd/csrc/cells/cell_grid_math.h"
#include "../../include/egnn_amd.h"
#include "cell_fixtures.h"

using namespace egnn;
using namespace cell_fixtures;

namespace {

struct Result {
  std::vector<int32_t> nb, atom_bin, bin_start, sorted_atom, bond_ptr, bond_atom, bond_shift;
  std::vector<double> sorted_frac;
  std::vector<int64_t> counts;
  int64_t n_bins = -7;
};

Result run(const Batch& b, int A, double radius, int reach, bool bonds, double dR, int nbins) {
  const int C = (int)b.cell_ptr.size() - 1, N = b.cell_ptr.back();
  Result r;
  r.nb.assign(3 * (size_t)C, -7);
  CHECK(egnn_cell_grid_dims(C, b.lattice.data(), radius, reach, 0.0, r.nb.data()) == EGNN_OK, "%s", egnn_last_error());
  int64_t B = 0;
  for (int c = 0; c < C; ++c) B += (int64_t)r.nb[3 * c] * r.nb[3 * c + 1] * r.nb[3 * c + 2];
  r.atom_bin.assign(N, -7);
  r.sorted_atom.assign(N, -7);
  r.sorted_frac.assign(3 * (size_t)N, -7.0);
  r.bin_start.assign((size_t)B + 1, -7);
  if (bonds) r.bond_ptr.assign((size_t)N + 1, -7);
  if (nbins) r.counts.assign((size_t)C * A * A * nbins, -7);
  for (int pass = 0; pass < 2; ++pass) {
    CHECK(egnn_cell_grid_host(C, A, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), radius, reach, 0.0, r.nb.data(), &r.n_bins,
                              r.atom_bin.data(), B + 1, r.bin_start.data(), r.sorted_atom.data(), r.sorted_frac.data(),
                              bonds ? r.bond_ptr.data() : nullptr, (int64_t)r.bond_atom.size(), r.bond_atom.data(), r.bond_shift.data(), dR, nbins,
                              nbins ? r.counts.data() : nullptr) == EGNN_OK, "%s", egnn_last_error());
    if (!bonds || pass == 1) break;
    r.bond_atom.assign((size_t)r.bond_ptr[N], -7);
    r.bond_shift.assign((size_t)r.bond_ptr[N], -7);
  }
  CHECK(r.n_bins == B, "n_bins %lld, not %lld", (long long)r.n_bins, (long long)B);
  for (int32_t v : r.bin_start) CHECK(v >= 0 && v <= N, "a bin start was not written");
  for (int32_t v : r.sorted_atom) CHECK(v >= 0 && v < N, "a sorted atom was not written");
  for (double v : r.sorted_frac) CHECK(v >= 0.0 && v < 1.0, "a sorted coordinate was not written");
  for (int32_t v : r.bond_atom) CHECK(v >= 0 && v < N, "a bond was not written");
  for (int32_t v : r.bond_shift) CHECK(v >= 0 && v < kCellShiftCodes, "a shift was not written");
  for (int64_t v : r.counts) CHECK(v >= 0, "a count was not written");
  return r;
}

}  // namespace

int main() {
  {   // beta-cristobalite: 3 x 3 x 3 bins, every neighbour bin of every centre wraps
    Batch b;
    add_cristobalite(b, -2.0);
    Result r = run(b, 2, 2.0, 1, true, 0.0, 0);
    CHECK(r.nb[0] == 3 && r.nb[1] == 3 && r.nb[2] == 3, "nb %d %d %d", r.nb[0], r.nb[1], r.nb[2]);
    CHECK(r.bond_ptr[24] == 64, "%d bonds", r.bond_ptr[24]);
    for (int i = 0; i < 24; ++i) {
      CHECK(r.bond_ptr[i + 1] - r.bond_ptr[i] == (b.type[i] == 1 ? 4 : 2), "atom %d has %d bonds", i, r.bond_ptr[i + 1] - r.bond_ptr[i]);
      for (int e = r.bond_ptr[i] + 1; e < r.bond_ptr[i + 1]; ++e)
        CHECK(r.bond_atom[e - 1] * kCellShiftCodes + r.bond_shift[e - 1] < r.bond_atom[e] * kCellShiftCodes + r.bond_shift[e], "row %d is not ascending", i);
      if (i > 0) CHECK(r.atom_bin[r.sorted_atom[i - 1]] <= r.atom_bin[r.sorted_atom[i]], "the sorted order is not ascending by bin");
    }
    Result p = run(b, 2, 23 * 0.1, 1, false, 0.1, 23);   // [0, 2.3): the 64 Si-O bonds at 1.55 A and nothing else
    int64_t total[4] = {0, 0, 0, 0};
    for (int ab = 0; ab < 4; ++ab)
      for (int k = 0; k < 23; ++k) total[ab] += p.counts[(size_t)ab * 23 + k];
    CHECK(total[0] == 0 && total[1] == 32 && total[2] == 32 && total[3] == 0, "pairs %lld %lld %lld %lld", (long long)total[0], (long long)total[1],
          (long long)total[2], (long long)total[3]);
    CHECK(p.counts[(size_t)1 * 23 + 15] == 32, "the Si-O distance is 1.55 A");
  }
  {   // one atom in a 7 A cell: no bond; at reach 3 and radius 1.5 A, 13 bins per axis and no pair
    Batch b;
    b.add(7.0, {0.3, -0.6, 0.9}, {0});
    Result r = run(b, 1, 2.0, 1, true, 0.0, 0);
    CHECK(r.nb[0] == 3 && r.bond_ptr[1] == 0 && r.sorted_atom[0] == 0, "one atom: %d bonds", r.bond_ptr[1]);
    Result p = run(b, 1, 3 * 0.5, 3, false, 0.5, 3);
    CHECK(p.nb[0] == 13, "one atom, reach 3: nb %d", p.nb[0]);
    for (int64_t v : p.counts) CHECK(v == 0, "nothing within 1.5 A");
    int nb[3];
    const double L[9] = {7, 0, 0, 0, 7, 0, 0, 0, 7};
    CHECK(cell_grid_dims(L, 2.34, 1, 0.0, nb) && nb[0] == 0, "7 / 2.34 = 2.99: not griddable");
  }
  {   // an empty cell, alone and beside cristobalite
    Batch b;
    b.add(7.0, {}, {});
    Result r = run(b, 1, 2.0, 1, true, 0.1, 20);
    CHECK(r.n_bins == 27 && r.bond_ptr[0] == 0 && r.bin_start[27] == 0, "empty cell");
    add_cristobalite(b, -2.0);
    Result q = run(b, 2, 2.0, 1, true, 0.0, 0);
    CHECK(q.n_bins == 54 && q.bond_ptr[24] == 64 && q.bin_start[27] == 0 && q.bin_start[54] == 24, "empty cell beside cristobalite");
  }
  {   // refused arguments leave the lists alone
    Batch b;
    add_cristobalite(b, -2.0);
    int32_t nb[3] = {-7, -7, -7}, bond_ptr[25];
    int64_t n_bins = -7, counts[4 * 30];
    for (int64_t& v : counts) v = -7;
    for (int32_t& v : bond_ptr) v = -7;
    CHECK(egnn_cell_grid_host(1, 2, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), 30 * 0.1, 2, 0.0, nb, &n_bins, nullptr, 0,
                              nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0.1, 30, counts) == EGNN_EINVAL, "(3.0, 2) is not griddable");
    CHECK(egnn_cell_grid_host(1, 2, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), 2.39, 1, 0.0, nb, &n_bins, nullptr, 0,
                              nullptr, nullptr, nullptr, bond_ptr, 0, nullptr, nullptr, 0.0, 0, nullptr) == EGNN_EINVAL, "2.39 is not griddable");
    CHECK(egnn_cell_grid_host(0, 2, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), 2.0, 1, 0.0, nb, &n_bins, nullptr, 0,
                              nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0.0, 0, nullptr) == EGNN_EINVAL, "C = 0");
    CHECK(counts[0] == -7 && counts[119] == -7 && bond_ptr[0] == -7 && bond_ptr[24] == -7, "nothing written");
  }
  printf("CELL-GRID-OK\n");
  return 0;
}

// Stand-alone run of egnn_cell_env_host (csrc/cells/cell_host.cpp), built with -fsanitize=address,undefined by
// tests/test_cells_host.py.  Every output array is allocated at EXACTLY the size the first call reports, so that ASan sees a write
// past the bond list or past an environment: the two-atom chain cell (3 / 5 / 7 / 9 sites for 1-4 shells, shifts up to 2),
// ideal beta-cristobalite (24 atoms, 4 bonds per Si and 2 per O, 9 sites at 2 shells, 33 at 4), both in one batch, and the overflow
// case (max_atoms = 8 where every environment holds 9: sentinel sizes, no row written).  The dense regime: the exact 2 x 2 x 2
// simple-cubic cell of spacing 1.1 A (26 bonds per atom, 27 / 125 / 343 / 729 sites for 1-4 shells) at max_atoms = 729, which fits,
// and 728, where the two scratch lists of max_atoms + 2 keys are at their fullest before the sentinel; and the ladder (five atoms
// 0.41 A apart in a 2.05 A cell: 33 sites at 4 shells, shifts up to +-4, the ends of the code range).
#include "../../diffusion_model_amd/csrc/cells/cell_math.h"
#include "../../include/egnn_amd.h"
#include "cell_fixtures.h"

using namespace egnn;
using namespace cell_fixtures;

namespace {

void add_cubic_block(Batch& b) {   // 2 x 2 x 2 atoms, 1.1 A apart: neighbours at 1.1, 1.556 and 1.905 A, the next at 2.2 A
  std::vector<double> f;
  std::vector<int32_t> t;
  for (int x = 0; x < 2; ++x)
    for (int y = 0; y < 2; ++y)
      for (int z = 0; z < 2; ++z) {
        f.push_back(0.5 * x); f.push_back(0.5 * y); f.push_back(0.5 * z);
        t.push_back((x + y + z) & 1);
      }
  b.add(2.2, f, t);
}

void add_ladder(Batch& b) { b.add(2.05, {0.0, 0.3, 0.3, 0.2, 0.3, 0.3, 0.4, 0.3, 0.3, 0.6, 0.3, 0.3, 0.8, 0.3, 0.3}, {0, 1, 0, 1, 0}); }

struct Result {
  std::vector<int32_t> bond_ptr, bond_atom, bond_shift, size, atom, shift, type;
  std::vector<float> pos;
};

Result run(const Batch& b, const std::vector<int32_t>& centre_cell, const std::vector<int32_t>& centre, int shells, int max_atoms) {
  const int C = (int)b.cell_ptr.size() - 1, N = b.cell_ptr.back(), M = (int)centre.size();
  Result r;
  r.bond_ptr.resize(N + 1);
  r.size.resize(M);
  auto call = [&](int64_t bc, int64_t ec) {
    return egnn_cell_env_host(C, 2, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), 2.0, M, centre_cell.data(),
                              centre.data(), shells, max_atoms, r.bond_ptr.data(), bc, bc ? r.bond_atom.data() : nullptr,
                              bc ? r.bond_shift.data() : nullptr, r.size.data(), ec, ec ? r.atom.data() : nullptr,
                              ec ? r.shift.data() : nullptr, ec ? r.type.data() : nullptr, ec ? r.pos.data() : nullptr);
  };
  CHECK(call(0, 0) == EGNN_OK, "%s", egnn_last_error());
  const int64_t E = r.bond_ptr[N];
  int64_t T = 0;
  for (int m = 0; m < M; ++m) T += r.size[m] <= max_atoms ? r.size[m] : 0;
  r.bond_atom.assign(E, -7); r.bond_shift.assign(E, -7);
  r.atom.assign(T, -7); r.shift.assign(T, -7); r.type.assign(T, -7);
  r.pos.assign(3 * T, -7.f);
  CHECK(call(E, T) == EGNN_OK, "%s", egnn_last_error());
  for (int64_t e = 0; e < E; ++e) CHECK(r.bond_atom[e] >= 0 && r.bond_atom[e] < N && r.bond_shift[e] >= 0 && r.bond_shift[e] < 729, "bond %lld", (long long)e);
  for (int64_t t = 0; t < T; ++t) CHECK(r.atom[t] >= 0 && r.atom[t] < N && r.shift[t] >= 0 && r.shift[t] < 729 && r.type[t] >= 0, "row %lld", (long long)t);
  return r;
}

}  // namespace

int main() {
  Batch b;
  add_chain(b);
  add_cristobalite(b);
  std::vector<int32_t> centre_cell, centre;
  for (int c = 0; c < 2; ++c)
    for (int i = b.cell_ptr[c]; i < b.cell_ptr[c + 1]; ++i) { centre_cell.push_back(c); centre.push_back(i); }
  const int chain_sites[5] = {0, 3, 5, 7, 9};
  for (int shells = 1; shells <= 4; ++shells) {
    Result r = run(b, centre_cell, centre, shells, 256);
    CHECK(r.size[0] == chain_sites[shells] && r.size[1] == chain_sites[shells], "chain: %d sites at %d shells", r.size[1], shells);
    int at = r.size[0], widest = 0;
    for (int k = 0; k < r.size[1]; ++k) {
      int s[3];
      cell_shift_decode(r.shift[at + k], s);
      CHECK(s[1] == 0 && s[2] == 0, "the chain runs along x");
      widest = abs(s[0]) > widest ? abs(s[0]) : widest;
    }
    CHECK(widest == (shells + 1) / 2, "chain: shifts up to %d at %d shells", widest, shells);
    CHECK(r.atom[at] == 1 && r.shift[at] == kCellCentreCode && r.pos[3 * at] == 0.f, "the centre comes first, at the origin");
    for (int i = 2; i < 26; ++i) {
      CHECK(r.bond_ptr[i + 1] - r.bond_ptr[i] == (b.type[i] == 1 ? 4 : 2), "cristobalite: %d bonds at atom %d", r.bond_ptr[i + 1] - r.bond_ptr[i], i);
      if (shells == 2) CHECK(r.size[i] == 9, "cristobalite: %d sites at 2 shells", r.size[i]);
      if (shells == 4) CHECK(r.size[i] == 33, "cristobalite: %d sites at 4 shells", r.size[i]);
    }
  }
  {   // overflow: every environment of cristobalite holds 9 sites at 2 shells
    Result r = run(b, centre_cell, centre, 2, 8);
    for (int i = 2; i < 26; ++i) CHECK(r.size[i] == 9, "sentinel %d", r.size[i]);
    CHECK(r.size[0] == 5 && r.atom.size() == 10u, "the chain's two environments are the only rows (%zu)", r.atom.size());
    Result ok = run(b, centre_cell, centre, 2, 9);
    CHECK(ok.atom.size() == 10u + 24u * 9u, "max_atoms = 9 holds them (%zu)", ok.atom.size());
  }
  {   // the dense regime: 729 sites per centre, and the ladder's shifts of +-4
    Batch d;
    add_cubic_block(d);
    add_ladder(d);
    std::vector<int32_t> cc, ct;
    for (int c = 0; c < 2; ++c)
      for (int i = d.cell_ptr[c]; i < d.cell_ptr[c + 1]; ++i) { cc.push_back(c); ct.push_back(i); }
    const int block_sites[5] = {0, 27, 125, 343, 729};
    for (int shells = 1; shells <= 4; ++shells) {
      Result r = run(d, cc, ct, shells, 729);
      for (int i = 0; i < 8; ++i) {
        CHECK(r.bond_ptr[i + 1] - r.bond_ptr[i] == 26, "cubic block: %d bonds at atom %d", r.bond_ptr[i + 1] - r.bond_ptr[i], i);
        CHECK(r.size[i] == block_sites[shells], "cubic block: %d sites at %d shells", r.size[i], shells);
      }
      for (int i = 8; i < 13; ++i) {
        CHECK(r.bond_ptr[i + 1] - r.bond_ptr[i] == 8, "ladder: %d bonds at atom %d", r.bond_ptr[i + 1] - r.bond_ptr[i], i);
        CHECK(r.size[i] == 1 + 8 * shells, "ladder: %d sites at %d shells", r.size[i], shells);
      }
      if (shells < 4) continue;
      CHECK(r.atom.size() == 8u * 729u + 5u * 33u, "%zu rows", r.atom.size());
      int at = 8 * 729, low = 0, high = 0;
      for (int i = 8; i < 13; ++i)
        for (int k = 0; k < 33; ++k, ++at) {
          int s[3];
          cell_shift_decode(r.shift[at], s);
          CHECK(s[1] == 0 && s[2] == 0, "the ladder runs along x");
          if (i == 8 || i == 12) { low = s[0] < low ? s[0] : low; high = s[0] > high ? s[0] : high; }
        }
      CHECK(low == -4 && high == 4, "ladder: shifts from %d to %d", low, high);
    }
    Result full = run(d, cc, ct, 4, 728);   // one below: keys and seen hold max_atoms + 1 entries when the search stops
    for (int i = 0; i < 8; ++i) CHECK(full.size[i] == 729, "sentinel %d", full.size[i]);
    CHECK(full.size[8] == 33 && full.atom.size() == 5u * 33u, "the ladder's environments are the only rows (%zu)", full.atom.size());
  }
  {   // refused arguments leave every output alone
    Batch bad;
    bad.add(1.9, {0, 0, 0}, {0});
    int32_t bp[2] = {-7, -7};
    CHECK(egnn_cell_env_host(1, 2, bad.cell_ptr.data(), bad.lattice.data(), bad.frac.data(), bad.type.data(), 2.0, 0, nullptr, nullptr,
                             2, 256, bp, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == EGNN_EINVAL, "a narrow cell");
    CHECK(bp[0] == -7 && bp[1] == -7, "nothing written");
  }
  printf("CELL-ENV-OK\n");
  return 0;
}

// What the stand-alone programs of the periodic-cell host statements (cell_*_main.cpp) share: the CHECK macro, a batch of cells and
// its builders (cubic cells from listed atoms, the chain, ideal beta-cristobalite; seeded random atoms in any lattice), and the small
// generator behind the random ones.  Header only; every program keeps its own cases, result arrays and checks.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                              \
      fprintf(stderr, "\n");                                     \
      exit(1);                                                   \
    }                                                            \
  } while (0)

namespace cell_fixtures {

// a small LCG: the programs need no library for their numbers.  A program seeds it first (seed), so its numbers are its own.
inline uint64_t& lcg_state() {
  static uint64_t state = 0;
  return state;
}
inline void seed(uint64_t s) { lcg_state() = s; }
inline double uniform() {
  uint64_t& s = lcg_state();
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(s >> 11) / 9007199254740992.0;
}

inline double factorial(int n) { return n <= 1 ? 1.0 : n * factorial(n - 1); }

struct Cells {
  std::vector<int32_t> cell_ptr{0};
  std::vector<double> lattice, frac;
  std::vector<int32_t> type;
  int C() const { return (int)cell_ptr.size() - 1; }
  int N() const { return (int)type.size(); }
  // a cubic cell of edge a with the atoms listed
  void add(double a, const std::vector<double>& f, const std::vector<int32_t>& t) {
    const double L[9] = {a, 0, 0, 0, a, 0, 0, 0, a};
    lattice.insert(lattice.end(), L, L + 9);
    frac.insert(frac.end(), f.begin(), f.end());
    type.insert(type.end(), t.begin(), t.end());
    cell_ptr.push_back(N());
  }
};
typedef Cells Batch;

// n atoms of A types drawn from the generator in the lattice L; some coordinates fall outside [0, 1)
inline void add_cell(Cells& b, const double* L, int n, int A) {
  for (int k = 0; k < 9; ++k) b.lattice.push_back(L[k]);
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) b.frac.push_back(2.0 * uniform() - 0.5);
    b.type.push_back((int32_t)(uniform() * A) % A);
  }
  b.cell_ptr.push_back(b.N());
}

inline void add_chain(Cells& b) { b.add(3.2, {0, 0, 0, 0.5, 0, 0}, {1, 0}); }

// ideal beta-cristobalite, 8 Si (type 1) then 16 O (type 0); the O are displaced by `outside` whole cells: wrapped by the statement
inline void add_cristobalite(Cells& b, double outside = 2.0) {
  const double fcc[4][3] = {{0, 0, 0}, {0, .5, .5}, {.5, 0, .5}, {.5, .5, 0}};
  const double arm[4][3] = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
  std::vector<double> f;
  std::vector<int32_t> t;
  for (int o = 0; o < 2; ++o)
    for (int k = 0; k < 4; ++k) {
      for (int x = 0; x < 3; ++x) f.push_back(fcc[k][x] + 0.25 * o);
      t.push_back(1);
    }
  for (int k = 0; k < 4; ++k)
    for (int m = 0; m < 4; ++m) {
      for (int x = 0; x < 3; ++x) f.push_back(fcc[k][x] + arm[m][x] / 8.0 + outside);
      t.push_back(0);
    }
  b.add(7.16, f, t);
}

// the thin triclinic cell of the site tests (image boxes 4 / 1 / 2 at kCut) and a plain cube
const double kThin[9] = {1.15, 0.0, 0.0, 0.4, 4.8, 0.0, 0.3, -0.5, 3.1};
const double kCube[9] = {5.0, 0.0, 0.0, 0.0, 5.0, 0.0, 0.0, 0.0, 5.0};
const double kCut = 4.37;

}  // namespace cell_fixtures

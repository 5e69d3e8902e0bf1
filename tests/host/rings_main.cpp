// Stand-alone run of egnn_rings_host (csrc/eval/rings_host.cpp), built with -fsanitize=address,undefined by
// tests/test_rings_host.py.  Every array is allocated at EXACTLY its size, so that ASan sees a read past a list or a write past an
// output: ideal beta-cristobalite with its periodic bond list built here (size 12 through every angle: 2 paths at a Si, 6 at an
// O), the same at a site limit that every search exceeds, the two-atom chain cell (no ring), and a random symmetric cluster graph
// at several max_size, where only the bounds are checked.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../diffusion_model_amd/csrc/eval/rings_math.h"
#include "../../include/egnn_amd.h"

using namespace egnn;

namespace {

#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                              \
      fprintf(stderr, "\n");                                     \
      exit(1);                                                   \
    }                                                            \
  } while (0)

struct Graph {
  int N = 0;
  bool periodic = false;
  std::vector<int32_t> row_ptr{0}, atom, shift, type;
};

// a cubic cell of edge a: image (j, s), s in {-1,0,1}^3, is bonded to i iff closer than cutoff (and not i itself)
Graph cubic(double a, const std::vector<double>& frac, const std::vector<int32_t>& type, double cutoff) {
  Graph g;
  g.N = (int)type.size();
  g.periodic = true;
  g.type = type;
  for (int i = 0; i < g.N; ++i) {
    for (int j = 0; j < g.N; ++j)
      for (int sx = -1; sx <= 1; ++sx)
        for (int sy = -1; sy <= 1; ++sy)
          for (int sz = -1; sz <= 1; ++sz) {
            if (j == i && !sx && !sy && !sz) continue;
            const int s[3] = {sx, sy, sz};
            double r2 = 0;
            for (int x = 0; x < 3; ++x) {
              const double d = (frac[3 * j + x] - frac[3 * i + x] + s[x]) * a;
              r2 += d * d;
            }
            if (r2 >= cutoff * cutoff) continue;
            g.atom.push_back(j);
            g.shift.insert(g.shift.end(), s, s + 3);
          }
    g.row_ptr.push_back((int32_t)g.atom.size());
  }
  return g;
}

Graph cristobalite() {
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
      for (int x = 0; x < 3; ++x) {
        const double v = fcc[k][x] + arm[m][x] / 8.0;
        f.push_back(v - floor(v));
      }
      t.push_back(0);
    }
  return cubic(7.16, f, t, 2.0);
}

struct Result {
  std::vector<int32_t> angle_ptr, size, count, overflow, hist;
};

Result run(const Graph& g, const std::vector<int32_t>& centre, int max_size, int max_sites, bool with_hist = true) {
  Result r;
  r.angle_ptr.push_back(0);
  for (int32_t c : centre) {
    const int d = g.row_ptr[c + 1] - g.row_ptr[c];
    r.angle_ptr.push_back(r.angle_ptr.back() + ring_angles(d));
  }
  const int n = r.angle_ptr.back(), M = (int)centre.size();
  r.size.assign(n, -7);
  r.count.assign(n, -7);
  r.overflow.assign(M, -7);
  if (with_hist) r.hist.assign(2 * (size_t)(max_size + 1), -7);
  int32_t dummy = 0;   // a non-null pointer for an empty array
  const int rc = egnn_rings_host(g.N, g.row_ptr.data(), (int)g.atom.size(), g.atom.data(), g.periodic ? g.shift.data() : nullptr,
                                 g.type.data(), 2, M, centre.data(), r.angle_ptr.data(), n, max_size, max_sites, n ? r.size.data() : &dummy,
                                 n ? r.count.data() : &dummy, r.overflow.data(), with_hist ? r.hist.data() : nullptr);
  CHECK(rc == EGNN_OK, "%s", egnn_last_error());
  for (int a = 0; a < n; ++a)
    CHECK((r.size[a] == -1 || r.size[a] == 0 || (r.size[a] >= 2 && r.size[a] <= max_size)) && r.count[a] >= 0 && (r.count[a] > 0) == (r.size[a] > 0),
          "angle %d: size %d, count %d", a, r.size[a], r.count[a]);
  return r;
}

std::vector<int32_t> everybody(const Graph& g) {
  std::vector<int32_t> c(g.N);
  for (int i = 0; i < g.N; ++i) c[i] = i;
  return c;
}

}  // namespace

int main() {
  {
    const Graph g = cristobalite();
    const Result r = run(g, everybody(g), 16, 4096);
    for (int i = 0; i < 24; ++i) {
      const int d = g.row_ptr[i + 1] - g.row_ptr[i];
      CHECK(d == (g.type[i] == 1 ? 4 : 2), "cristobalite: %d bonds at atom %d", d, i);
      for (int a = r.angle_ptr[i]; a < r.angle_ptr[i + 1]; ++a)
        CHECK(r.size[a] == 12 && r.count[a] == (g.type[i] == 1 ? 2 : 6), "atom %d: size %d, count %d", i, r.size[a], r.count[a]);
      CHECK(r.overflow[i] == 0, "no overflow");
    }
    CHECK(r.hist[12] == 16 && r.hist[17 + 12] == 48, "histogram %d %d", r.hist[12], r.hist[17 + 12]);
    const Result s = run(g, everybody(g), 16, 64);          // every search needs more than 64 sites
    for (int i = 0; i < 24; ++i) {
      CHECK(s.overflow[i] == 1, "overflow at atom %d", i);
      for (int a = s.angle_ptr[i]; a < s.angle_ptr[i + 1]; ++a) CHECK(s.size[a] == -1 && s.count[a] == 0, "sentinel");
    }
    for (int32_t v : s.hist) CHECK(v == 0, "overflowed angles are not counted");
    const Result t = run(g, {23, 0, 23}, 10, 1, false);     // max_sites 1: the source alone; rings of 12 lie above max_size anyway
    CHECK(t.size.size() == 8u, "1 + 6 + 1 angles");
  }
  {
    const Graph g = cubic(3.2, {0, 0, 0, 0.5, 0, 0}, {1, 0}, 2.0);
    const Result r = run(g, everybody(g), 32, 4096);
    CHECK(r.size.size() == 2u && r.size[0] == 0 && r.size[1] == 0 && r.count[0] == 0, "the chain has no ring");
    CHECK(r.hist[0] == 1 && r.hist[33] == 1, "two angles without a ring");
  }
  {   // a random symmetric cluster graph: 300 atoms, about 4 bonds each
    Graph g;
    g.N = 300;
    std::vector<std::vector<int32_t>> nb(g.N);
    uint64_t x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int e = 0; e < 600; ++e) {
      const int i = (int)(next() % g.N), j = (int)(next() % g.N);
      if (i == j) continue;
      bool dup = false;
      for (int32_t v : nb[i]) dup |= v == j;
      if (dup || nb[i].size() >= 12 || nb[j].size() >= 12) continue;
      nb[i].push_back(j);
      nb[j].push_back(i);
    }
    for (int i = 0; i < g.N; ++i) {
      g.atom.insert(g.atom.end(), nb[i].begin(), nb[i].end());
      g.row_ptr.push_back((int32_t)g.atom.size());
      g.type.push_back(i % 2);
    }
    int rings = 0;
    for (int max_size : {3, 4, 12, 32}) {
      const Result r = run(g, everybody(g), max_size, 4096);
      for (int32_t v : r.size) rings += v > 0;
      const Result s = run(g, everybody(g), max_size, 7);
      for (size_t m = 0; m < s.overflow.size(); ++m) CHECK(s.overflow[m] == 0 || s.overflow[m] == 1, "flag");
    }
    CHECK(rings > 0, "a random graph of mean degree 4 has rings");
  }
  {   // refused arguments leave every output alone
    const Graph g = cubic(3.2, {0, 0, 0, 0.5, 0, 0}, {1, 0}, 2.0);
    const int32_t centre[1] = {0}, ap[2] = {0, 1};
    int32_t size[1] = {-7}, count[1] = {-7}, over[1] = {-7};
    CHECK(egnn_rings_host(2, g.row_ptr.data(), (int)g.atom.size(), g.atom.data(), g.shift.data(), g.type.data(), 2, 1, centre, ap, 1, 2,
                          4096, size, count, over, nullptr) == EGNN_EINVAL, "max_size 2");
    CHECK(size[0] == -7 && count[0] == -7 && over[0] == -7, "nothing written");
  }
  printf("RINGS-OK\n");
  return 0;
}

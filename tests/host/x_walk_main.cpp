// x_walk (csrc/x_walk.h), the walk of the persistent coordinate kernel over its (tile, column share) units, enumerated on the
// host for every workgroup: who runs what, in which order, on which XCD, and how many units.  Stand-alone (own main), built with
// AddressSanitizer + UBSan by tests/test_x_walk_host.py.
//
// Checks, for T in {1, 2, 255, 256, 257, 511, 512, 513, 8064, 8065} tiles x G in {1, 8, 104, 255, 256, 304} workgroups x 2 shares
// (and 1 share: checks 1 and 3 only):
//   1. every (tile, share) is visited exactly once, and a workgroup's valid steps are a prefix of its steps;
//   2. a kept share 1 directly follows the kept share 0 of the same tile on the same workgroup, and a kept share 0 is directly
//      followed by its share 1;
//   3. a tile's units run on a workgroup with the XCD index (blockIdx & 7) that xcd_tile assigns.  xcd_tile(b, n) places n workgroups
//      on n consecutive positions, and the XCD it assigns to position xcd_tile(b, n) is b & 7.  The positions are worked out here
//      without the walk: the tiles of a full sweep (G at a time) are the positions of xcd_tile(., G); the units of the remainder of
//      T % G tiles, in (tile, share) order and again G at a time, are the positions of xcd_tile(., n) for the n <= G units of their
//      window.  Both units of a tile of a full sweep therefore have one XCD;
//   4. no workgroup runs more than ceil(2 T / G) units.  That is the bound for EVERY G, not only where 8 divides G: every window
//      of the walk gives a workgroup at most one step, the full sweeps take 2 (T / G) steps and the remainder's 2 (T % G) units
//      ceil(2 (T % G) / G) windows.  No workgroup runs fewer than floor(2 T / G) units either;
//   5. T = 8,064, G = 256 (the benchmark's shape): every workgroup runs 63 units.
#include <cstdio>
#include <vector>

#include "../../diffusion_model_amd/csrc/x_walk.h"

using egnn::x_walk;
using egnn::xcd_tile;
using egnn::XUnit;

static int g_fail = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      if (++g_fail < 40) { std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); } \
    }                                                        \
  } while (0)

static int ceil_div(int a, int b) { return (a + b - 1) / b; }

// XCD index that xcd_tile assigns to each of n consecutive positions (and: xcd_tile(., n) is a bijection of 0 .. n - 1)
static std::vector<int> xcd_of_positions(int n) {
  std::vector<int> x((size_t)n, -1);
  for (int b = 0; b < n; ++b) {
    const int p = xcd_tile(b, n);
    CHECK(p >= 0 && p < n && x[p] < 0, "xcd_tile(%d, %d) = %d: out of range or taken", b, n, p);
    if (p >= 0 && p < n) x[p] = b & 7;
  }
  return x;
}

int main() {
  const int Ts[] = {1, 2, 255, 256, 257, 511, 512, 513, 8064, 8065};
  const int Gs[] = {1, 8, 104, 255, 256, 304};
  for (const int T : Ts) {
    for (const int G : Gs) {
      for (int nshare = 1; nshare <= 2; ++nshare) {
        // the XCD of every unit, from xcd_tile alone
        const int S = T / G, R = T % G;
        std::vector<int> xcd_unit((size_t)T * nshare, -1);
        {
          const std::vector<int> xs = xcd_of_positions(G);
          for (int t = 0; t < S * G; ++t)
            for (int h = 0; h < nshare; ++h) xcd_unit[(size_t)t * nshare + h] = xs[t % G];
          for (int v0 = 0; v0 < nshare * R; v0 += G) {
            const int n = nshare * R - v0 < G ? nshare * R - v0 : G;
            const std::vector<int> xr = xcd_of_positions(n);
            for (int p = 0; p < n; ++p) xcd_unit[(size_t)S * G * nshare + v0 + p] = xr[p];
          }
        }
        std::vector<int> seen((size_t)T * nshare, 0);
        int max_units = 0, min_units = 1 << 30;
        for (int b = 0; b < G; ++b) {
          int k = 0;
          XUnit prev{-1, -1, false, false};
          for (;; ++k) {
            const XUnit u = x_walk(b, G, T, nshare, k);
            if (!u.valid) break;
            CHECK(u.tile >= 0 && u.tile < T && u.share >= 0 && u.share < nshare, "T %d G %d b %d k %d: unit (%d, %d) out of range", T, G, b,
                  k, u.tile, u.share);
            if (u.tile < 0 || u.tile >= T || u.share < 0 || u.share >= nshare) break;
            const size_t id = (size_t)u.tile * nshare + u.share;
            ++seen[id];
            CHECK(!u.kept || nshare == 2, "T %d G %d: kept chunks with one share", T, G);
            if (u.kept && u.share == 1)
              CHECK(prev.valid && prev.kept && prev.share == 0 && prev.tile == u.tile, "T %d G %d b %d k %d: kept share 1 of tile %d does not follow its share 0",
                    T, G, b, k, u.tile);
            if (prev.valid && prev.kept && prev.share == 0)
              CHECK(u.kept && u.share == 1 && u.tile == prev.tile, "T %d G %d b %d k %d: kept share 0 of tile %d is not followed by its share 1", T, G, b, k,
                    prev.tile);
            CHECK(xcd_unit[id] == (b & 7), "T %d G %d b %d: unit (%d, %d) belongs to XCD %d", T, G, b, u.tile, u.share, xcd_unit[id]);
            if (u.kept) CHECK(xcd_unit[(size_t)u.tile * nshare] == xcd_unit[(size_t)u.tile * nshare + 1], "T %d G %d: kept tile %d on two XCDs", T, G, u.tile);
            prev = u;
          }
          CHECK(!(prev.valid && prev.kept && prev.share == 0), "T %d G %d b %d: the walk ends between the shares of tile %d", T, G, b, prev.tile);
          for (int m = 1; m <= 3; ++m) CHECK(!x_walk(b, G, T, nshare, k + m).valid, "T %d G %d b %d: step %d valid after an invalid one", T, G, b, k + m);
          if (k > max_units) max_units = k;
          if (k < min_units) min_units = k;
        }
        for (size_t i = 0; i < seen.size(); ++i)
          CHECK(seen[i] == 1, "T %d G %d shares %d: unit (%d, %d) visited %d times", T, G, nshare, (int)(i / nshare), (int)(i % nshare), seen[i]);
        if (nshare != 2) continue;
        const int even = ceil_div(2 * T, G);
        CHECK(max_units <= even, "T %d G %d: max units %d above ceil(2T/G) = %d", T, G, max_units, even);
        CHECK(min_units >= 2 * T / G, "T %d G %d: min units %d below floor(2T/G) = %d", T, G, min_units, 2 * T / G);
        if (T == 8064 && G == 256) CHECK(max_units == 63 && min_units == 63, "T 8064 G 256: units per workgroup %d .. %d, expected 63", min_units, max_units);
        std::printf("T %5d G %3d: units per workgroup %d .. %d (ceil(2T/G) = %d)\n", T, G, min_units, max_units, even);
      }
    }
  }
  if (g_fail) { std::printf("X-WALK-FAILED %d\n", g_fail); return 1; }
  std::printf("X-WALK-OK\n");
  return 0;
}

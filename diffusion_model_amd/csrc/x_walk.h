// The XCD-aware workgroup -> tile map of the tiled kernels and the walk of the persistent coordinate kernel
// (edge_x_m16.hip) over its (tile, column share) units.  Plain integer arithmetic for host and device: no HIP calls, so that
// tests/host/x_walk_main.cpp can enumerate it.
#pragma once

#if defined(__HIPCC__)
#define EGNN_XWALK_HD __host__ __device__ __forceinline__
#else
#define EGNN_XWALK_HD inline
#endif

namespace egnn {

// XCD-aware workgroup -> tile map: workgroups b and b+8 share an XCD (round-robin dispatch), so give
// each XCD a contiguous range of tiles; tiles of one graph then share an L2 (table rows are re-read
// by every tile of the graph).  Bijective for any grid size; affects speed only.
EGNN_XWALK_HD int xcd_tile(int b, int nwg) {
  const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// Step k of persistent workgroup b of G over T tiles of nshare column shares each.  The tiles are taken G at a time, and within such a
// sweep xcd_tile(b, G) places the workgroups exactly as it places those of a one-tile-per-workgroup launch: the workgroups of an XCD
// (b % 8) run a contiguous window of the sweep's tiles together, so one to two graphs' table rows are hot in the XCD's L2 at any moment.
//   * Full sweeps (S = T / G of them) are whole tiles: the workgroup runs share 0 and then share 1 of ITS tile, sweep * G +
//     xcd_tile(b, G), in consecutive steps, and the activation chunks share 0 left in LDS are there for share 1 (kept).
//   * The remainder of R = T % G < G tiles is handed out as single units, each building everything (kept = false): its nshare R
//     units, in (tile, share) order, are taken G at a time like the tiles before them, the last window being the n < G units that are
//     left, placed by xcd_tile(b, n) for b < n.  (Whole tiles there would leave half of the workgroups a unit short at 31.5 tiles
//     per workgroup, the benchmark's shape.)
// A workgroup runs nshare S units and one more for every remainder window that reaches it: ceil(nshare T / G) at most, for every G,
// and no workgroup more than one unit above another.
// valid = false: the workgroup has no step k (and none after it).
struct XUnit {
  int tile, share;
  bool kept, valid;
};

EGNN_XWALK_HD XUnit x_walk(int b, int G, int T, int nshare, int k) {
  const int S = T / G, R = T - S * G;
  XUnit u;
  if (k < nshare * S) {
    const int sweep = k / nshare;
    u.tile = sweep * G + xcd_tile(b, G);
    u.share = k - sweep * nshare;
    u.kept = nshare == 2;
    u.valid = true;
  } else {
    const int v0 = (k - nshare * S) * G;     // first unit of this window of the remainder
    const int left = nshare * R - v0;        // (R < G: at most nshare windows, so v0 stays small)
    const int n = left < G ? left : G;
    u.valid = b < n;                         // (n <= 0 behind the last window)
    const int v = u.valid ? v0 + xcd_tile(b, n) : 0;
    u.tile = S * G + v / nshare;
    u.share = v % nshare;
    u.kept = false;
  }
  return u;
}

}  // namespace egnn

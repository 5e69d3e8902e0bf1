// Definitions of the shortest-path ring statistics (rings.hip, rings_host.cpp): King's shortest-path criterion as Rino et al. apply
// it per O-Si-O / Si-O-Si angle.  Plain C++ behind a host/device macro (the pattern of topo_math.h), so that the kernel and the host
// statement read the same text.  No reference file computes rings: this is an extension beyond the reference.
//
//  * sites and bonds: the input is a bond list in CSR form, row a = the bonds of atom a.  For clusters a site is an atom (every
//    shift is 0); for periodic cells a site is (atom, integer lattice shift) of the INFINITE lattice: following bond e of atom a from
//    site (a, s) leads to (atom[e], s + shift[e]).  There is no minimum-image folding and no aliasing of images.  A bond whose
//    neighbour lies outside [0, N) or whose shift has a component outside {-1, 0, 1} is refused by the host statement and ignored by
//    the kernel.
//  * angles: an angle of a centre c (site (c, 0)) is a pair (p, q), p < q, of positions in c's row; a centre of degree d has
//    d (d - 1) / 2 of them, in lexicographic order of (p, q).  Two images of one atom in a row are two neighbours.
//  * per angle, with j = row[p], k = row[q] as sites: size = 2 + the number of bonds on a shortest path from j to k in the graph
//    with the site (c, 0) removed (images (c, s != 0) stay), 0 if no such path has size <= max_size; count = the number of
//    distinct shortest such paths, saturating at 2^31 - 1, 0 where size is 0.  size counts ATOMS on the ring: a "6-membered"
//    silica ring has size 12.
//  * search: one per (centre, p), level by level from j (level 0, count 1), targets row[q] for q > p.  It stops after the first
//    level at which every target is labelled, at level max_size - 2, or when the frontier is empty; a level is always completed.
//    The count of a site that joins level l is the saturating sum, over the bonds of ITS OWN row, of the counts of the neighbour
//    sites labelled at level l - 1 (a pull after the level's discovery: no atomic, and min(total, 2^31 - 1) does not depend on the
//    order of the terms).
//  * overflow: a search that labels more than max_sites sites (the source included; the removed centre is never labelled) is
//    overflowed: its angles get size -1, count 0 and overflow[m] = 1.  A centre with more than kRingMaxDegree bonds is reported
//    the same way: all its angles get size -1, count 0 and nothing is searched.
//  * histogram [A][max_size + 1]: angles by centre type and size, bin 0 = no ring; overflowed angles are not counted.
//
// A site key holds the atom in 32 bits and every shift component in 6 bits (-32 .. 31): from a neighbour of the centre (|s| <= 1)
// max_size - 2 <= 30 bonds of |shift| <= 1 reach |s| <= 31.  The level of a labelled site rides in the top byte of its table
// entry, so that one 64-bit compare-and-swap labels a site; kRingEmpty (all ones) is no entry.
#pragma once
#include "eval_math.h"

#define RING_MAX_SITES 4096

namespace egnn {

constexpr int kRingMaxDegree = 32;           // bonds of a centre (and of every atom a search passes)
constexpr int kRingMinSize = 3;              // max_size
constexpr int kRingMaxSize = 32;
constexpr int kRingMaxSites = RING_MAX_SITES;
constexpr int kRingCountMax = 2147483647;    // count saturates here
constexpr int kRingMinSlots = 512;           // table slots: a power of two >= 2 max_sites and >= this
constexpr uint64_t kRingEmpty = ~0ull;
constexpr uint64_t kRingKeyMask = (1ull << 50) - 1ull;
constexpr int kRingLevelShift = 56;

EGNN_HD bool ring_shift_ok(int s) { return s >= -1 && s <= 1; }

EGNN_HD uint64_t ring_key(int atom, int sx, int sy, int sz) {
  return ((uint64_t)(uint32_t)atom << 18) | ((uint64_t)(uint32_t)(sx + 32) << 12) | ((uint64_t)(uint32_t)(sy + 32) << 6) |
         (uint64_t)(uint32_t)(sz + 32);
}
EGNN_HD int ring_key_atom(uint64_t key) { return (int)(uint32_t)((key & kRingKeyMask) >> 18); }
EGNN_HD int ring_key_sx(uint64_t key) { return (int)((key >> 12) & 63) - 32; }
EGNN_HD int ring_key_sy(uint64_t key) { return (int)((key >> 6) & 63) - 32; }
EGNN_HD int ring_key_sz(uint64_t key) { return (int)(key & 63) - 32; }

// the site bond (atom, shift) leads to from the site `key`; shift = NULL for clusters
EGNN_HD uint64_t ring_step(uint64_t key, int atom, const int32_t* shift) {
  if (!shift) return ring_key(atom, ring_key_sx(key), ring_key_sy(key), ring_key_sz(key));
  return ring_key(atom, ring_key_sx(key) + shift[0], ring_key_sy(key) + shift[1], ring_key_sz(key) + shift[2]);
}

EGNN_HD uint64_t ring_entry(uint64_t key, int level) { return key | ((uint64_t)level << kRingLevelShift); }
EGNN_HD int ring_entry_level(uint64_t entry) { return (int)(entry >> kRingLevelShift); }

EGNN_HD int ring_sat_add(int a, int b) {   // a, b >= 0
  const int64_t s = (int64_t)a + (int64_t)b;
  return s > kRingCountMax ? kRingCountMax : (int)s;
}

EGNN_HD int ring_angles(int degree) { return degree * (degree - 1) / 2; }
// the first angle of row position p in a centre of degree d (angles in lexicographic order of (p, q))
EGNN_HD int ring_angle_first(int p, int d) { return p * d - p * (p + 1) / 2; }

EGNN_HD int ring_slots(int max_sites) {
  int s = kRingMinSlots;
  while (s < 2 * max_sites) s <<= 1;
  return s;
}

EGNN_HD uint32_t ring_hash(uint64_t key) {   // the finaliser of splitmix64
  key ^= key >> 30; key *= 0xbf58476d1ce4e5b9ull;
  key ^= key >> 27; key *= 0x94d049bb133111ebull;
  key ^= key >> 31;
  return (uint32_t)key;
}

}  // namespace egnn

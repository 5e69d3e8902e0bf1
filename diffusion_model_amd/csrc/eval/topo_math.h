// Definitions of the topological (bond-graph) fingerprint (topo.hip, topo_host.cpp): bonds guessed from distances, hop distances
// on the bond graph, connected fragments, the atom-pair count vector and its Tanimoto similarity.  Plain C++ behind a host/device
// macro (the pattern of structure_math.h), so that the kernels and the host statement read the same text.  They restate
// evaluate_fingerprint.py:49-114 (guess_bonds, GetAtomPairFingerprint, TanimotoSimilarity) without ASE or RDKit.
//
//  * bond: atoms i != j of one graph are bonded iff d < thr[type i][type j], d in fp64 from the float32 positions (distance64 of
//    eval_math.h: d(i, j) == d(j, i) bitwise, so the bond graph is symmetric).  thr = scale * (radius_a + radius_b) is computed
//    once per type pair in fp64 by the caller.
//  * degree: the number of bonds of an atom.  The lists hold kTopoMaxDegree neighbours; a graph with an atom above that is
//    reported in overflow[g] and has no distances, components or fingerprint.
//  * hop distance: bonds on a shortest path, uint16, kTopoUnreachable where there is none; never capped (a chain of 1024 atoms
//    has 1023).
//  * component[i]: the lowest atom index reachable from i (i itself included); fragments = atoms with component[i] == i.
//  * atom class: type * kTopoBranchModulus + degree % kTopoBranchModulus (RDKit's atom-pair code takes numBranches % 7; its
//    pi-electron field is 0 on a graph of single bonds).
//  * fingerprint: for unordered pairs i < j with 1 <= d <= L, ++fp[topo_pair_index(class i, class j) * L + (d - 1)].
//  * Tanimoto of rows a, b: and = sum min(a, b), sa = sum a, sb = sum b in int64; and / (sa + sb - and) as ONE fp64 division,
//    0.0 where the denominator is 0.
#pragma once
#include "eval_math.h"

namespace egnn {

constexpr int kTopoMaxTypes = 4;            // A
constexpr int kTopoMaxAtoms = 1024;         // atoms of one graph, as egnn_assign
constexpr int kTopoMaxDegree = 32;          // neighbours kept per atom
constexpr int kTopoBranchModulus = 7;       // degree field of the atom class
constexpr int kTopoMaxLength = 64;          // L
constexpr uint16_t kTopoUnreachable = 0xFFFF;

// thr is the table [A][A]; a type outside [0, A) bonds to nothing
EGNN_HD bool topo_bonded(const float* p, int tp, const float* q, int tq, const double* thr, int A) {
  if (tp < 0 || tp >= A || tq < 0 || tq >= A) return false;
  return distance64(p[0], p[1], p[2], q[0], q[1], q[2]) < thr[tp * A + tq];
}

EGNN_HD bool topo_threshold_ok(double t) { return t > 0.0 && t < 1e300; }   // positive, finite, not NaN

EGNN_HD int topo_classes(int A) { return kTopoBranchModulus * A; }
EGNN_HD int topo_class(int type, int degree) { return type * kTopoBranchModulus + degree % kTopoBranchModulus; }
EGNN_HD int topo_pair_index(int c1, int c2, int C) { return type_pair_index(c1, c2, C); }
EGNN_HD int topo_keys(int A, int L) { return topo_classes(A) * (topo_classes(A) + 1) / 2 * L; }
EGNN_HD int topo_key(int c1, int c2, int d, int C, int L) { return topo_pair_index(c1, c2, C) * L + (d - 1); }

EGNN_HD double topo_tanimoto(int64_t both, int64_t sa, int64_t sb) {
  const int64_t den = sa + sb - both;
  return den != 0 ? (double)both / (double)den : 0.0;
}

}  // namespace egnn

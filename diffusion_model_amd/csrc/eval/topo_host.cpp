// Host side of the topological fingerprint: the argument checks of the device entries (topo.hip) and the host statement
// egnn_topo_host -- bond lists, hop distances, components, atom-pair counts and Tanimoto similarities computed on the CPU through
// topo_math.h, the text the kernels compile.  No HIP call, no device code: checked (and run under the sanitizers) on a machine
// without a GPU.
#include <string.h>

#include <vector>

#include "topo_host.h"
#include "topo_math.h"

namespace egnn {

int topo_common_check(const char* who, int B, int A, const void* type, const void* graph_ptr, int max_atoms) {
  if (B < 1 || !type || !graph_ptr) { set_error("bad %s arguments (B >= 1; type and graph_ptr given)", who); return EGNN_EINVAL; }
  if (int rc = atom_types_check(who, A, kTopoMaxTypes)) return rc;
  if (max_atoms < 0 || max_atoms > kTopoMaxAtoms) {
    set_error("%s: a graph of %d atoms (at most %d: one workgroup holds a graph's bond lists)", who, max_atoms, kTopoMaxAtoms);
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

int topo_threshold_check(const char* who, int A, const double* thr) {
  if (!thr) { set_error("bad %s arguments (thr given)", who); return EGNN_EINVAL; }
  for (int k = 0; k < A * A; ++k)
    if (!topo_threshold_ok(thr[k])) {
      set_error("%s: threshold [%d][%d] must be positive and finite", who, k / A, k % A);
      return EGNN_EINVAL;
    }
  return EGNN_OK;
}

int topo_length_check(const char* who, int L) {
  if (L < 1 || L > kTopoMaxLength) { set_error("%s: max_length %d (1 <= L <= %d)", who, L, kTopoMaxLength); return EGNN_EINVAL; }
  return EGNN_OK;
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_topo_host(int B, int A, const float* pos, const int32_t* type, const int32_t* graph_ptr, const double* thr, int L,
                   int32_t* row_ptr, int32_t* neighbours, int32_t* degree, int32_t* overflow, uint16_t* dist, int32_t* component,
                   int32_t* fragments, int32_t* fp, int n_pairs, const int32_t* pairs, double* sim, int64_t* sa, int64_t* sb) {
  const char* who = "egnn_topo_host";
  if (int rc = topo_common_check(who, B, A, type, graph_ptr, 0)) return rc;
  if (!pos || !row_ptr || !neighbours || !degree || !overflow) {
    set_error("bad %s arguments (pos, row_ptr, neighbours, degree and overflow given)", who);
    return EGNN_EINVAL;
  }
  if (int rc = topo_threshold_check(who, A, thr)) return rc;
  if (int rc = topo_length_check(who, L)) return rc;
  if (n_pairs < 0 || (n_pairs > 0 && (!pairs || !sim || !sa || !sb || !fp))) {
    set_error("bad %s arguments (n_pairs >= 0; pairs, sim, sa, sb and fp given)", who);
    return EGNN_EINVAL;
  }
  for (int g = 0; g < B; ++g) {
    const int lo = graph_ptr[g], hi = graph_ptr[g + 1];
    if (lo < 0 || hi < lo || (g == 0 && lo != 0)) { set_error("%s: graph_ptr must start at 0 and not decrease", who); return EGNN_EINVAL; }
    if (int rc = topo_common_check(who, B, A, type, graph_ptr, hi - lo)) return rc;
    if (int rc = type_range_check(who, type, lo, hi, A)) return rc;
  }
  for (int p = 0; p < 2 * n_pairs; ++p)
    if (pairs[p] < 0 || pairs[p] >= B) { set_error("%s: pair %d names row %d outside [0, %d)", who, p / 2, pairs[p], B); return EGNN_EINVAL; }

  const int C = topo_classes(A), K = topo_keys(A, L);
  if (fp) memset(fp, 0, sizeof(int32_t) * (size_t)B * K);
  row_ptr[0] = 0;
  std::vector<int> queue(kTopoMaxAtoms), cls(kTopoMaxAtoms);
  std::vector<uint16_t> row(kTopoMaxAtoms);
  size_t dist_at = 0;
  for (int g = 0; g < B; ++g) {
    const int lo = graph_ptr[g], hi = graph_ptr[g + 1], n = hi - lo;
    overflow[g] = 0;
    for (int i = lo; i < hi; ++i) {
      int count = 0;
      for (int j = lo; j < hi; ++j) {
        if (j == i || !topo_bonded(pos + 3 * (size_t)i, type[i], pos + 3 * (size_t)j, type[j], thr, A)) continue;
        if (count < kTopoMaxDegree) neighbours[row_ptr[i] + count] = j;
        ++count;
      }
      degree[i] = count;
      row_ptr[i + 1] = row_ptr[i] + (count < kTopoMaxDegree ? count : kTopoMaxDegree);
      if (count > kTopoMaxDegree) ++overflow[g];
    }
    uint16_t* dist_g = dist ? dist + dist_at : nullptr;
    dist_at += (size_t)n * n;
    if (overflow[g]) {   // a bond list is cut short: no distances, no components, no fingerprint
      if (dist_g) for (size_t k = 0; k < (size_t)n * n; ++k) dist_g[k] = kTopoUnreachable;
      if (component) for (int i = lo; i < hi; ++i) component[i] = -1;
      if (fragments) fragments[g] = -1;
      continue;
    }
    for (int i = 0; i < n; ++i) cls[i] = topo_class(type[lo + i], degree[lo + i]);
    int roots = 0;
    for (int s = 0; s < n; ++s) {   // breadth first from s
      for (int j = 0; j < n; ++j) row[j] = kTopoUnreachable;
      int head = 0, tail = 0, lowest = s;
      row[s] = 0;
      queue[tail++] = s;
      while (head < tail) {
        const int u = queue[head++];
        for (int k = row_ptr[lo + u]; k < row_ptr[lo + u + 1]; ++k) {
          const int v = neighbours[k] - lo;
          if (row[v] != kTopoUnreachable) continue;
          row[v] = (uint16_t)(row[u] + 1);
          queue[tail++] = v;
          if (v < lowest) lowest = v;
        }
      }
      if (dist_g) memcpy(dist_g + (size_t)s * n, row.data(), sizeof(uint16_t) * (size_t)n);
      if (component) component[lo + s] = lo + lowest;
      roots += lowest == s;
      if (fp)
        for (int j = s + 1; j < n; ++j)
          if (row[j] >= 1 && row[j] <= L) ++fp[(size_t)g * K + topo_key(cls[s], cls[j], row[j], C, L)];
    }
    if (fragments) fragments[g] = roots;
  }
  for (int p = 0; p < n_pairs; ++p) {
    const int32_t* a = fp + (size_t)pairs[2 * p] * K;
    const int32_t* b = fp + (size_t)pairs[2 * p + 1] * K;
    int64_t both = 0, ta = 0, tb = 0;
    for (int k = 0; k < K; ++k) {
      both += a[k] < b[k] ? a[k] : b[k];
      ta += a[k];
      tb += b[k];
    }
    sim[p] = topo_tanimoto(both, ta, tb);
    sa[p] = ta;
    sb[p] = tb;
  }
  return EGNN_OK;
}

}  // extern "C"

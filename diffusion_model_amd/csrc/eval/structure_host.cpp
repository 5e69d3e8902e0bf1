// Host side of the whole-structure statistics: the argument checks of the device entries (structure.hip) and the host statement
// egnn_struct_counts_host -- the same three integer outputs computed on the CPU through structure_math.h, the text the kernels
// compile.  No HIP call, no device code: checked (and run under the sanitizers, make asan) on a machine without a GPU.
#include <string.h>

#include <vector>

#include "structure_host.h"
#include "structure_math.h"

namespace egnn {

static int struct_common_check(const char* who, int B, int A, const void* pos, const void* type, const void* graph_ptr, int max_atoms) {
  if (B < 1 || !pos || !type || !graph_ptr) { set_error("bad %s arguments (B >= 1; pos, type and graph_ptr given)", who); return EGNN_EINVAL; }
  if (int rc = atom_types_check(who, A, kStructMaxTypes)) return rc;
  if (max_atoms < 0 || max_atoms > kStructMaxAtoms) {
    set_error("%s: a graph of %d atoms (at most %d: the ordered pairs of one graph are counted in int32)", who, max_atoms, kStructMaxAtoms);
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

int struct_pair_args_check(const char* who, int B, int A, const void* pos, const void* type, const void* graph_ptr, int max_atoms,
                           double dR, int nbins, const void* counts) {
  if (int rc = struct_common_check(who, B, A, pos, type, graph_ptr, max_atoms)) return rc;
  if (!counts) { set_error("bad %s arguments (counts given)", who); return EGNN_EINVAL; }
  if (nbins < 1 || nbins > kStructMaxBins) { set_error("%s: %d radial bins (1 <= nbins <= %d)", who, nbins, kStructMaxBins); return EGNN_EINVAL; }
  if (!(dR > 0.0) || !(dR < 1e30)) { set_error("%s: dR must be positive and finite", who); return EGNN_EINVAL; }
  return EGNN_OK;
}

int struct_bond_args_check(const char* who, int B, int A, const void* pos, const void* type, const void* graph_ptr, int max_atoms,
                           float cutoff, double dtheta, int max_cn, const void* cn, const void* angles) {
  if (int rc = struct_common_check(who, B, A, pos, type, graph_ptr, max_atoms)) return rc;
  if (!cn || !angles) { set_error("bad %s arguments (cn and angles given)", who); return EGNN_EINVAL; }
  if (!(cutoff > 0.f)) { set_error("%s: cutoff must be positive", who); return EGNN_EINVAL; }
  if (!(dtheta > 0.0) || !(dtheta <= 180.0) || struct_angle_bins(dtheta) > kStructMaxAngleBins) {
    set_error("%s: dtheta must lie in [0.5, 180] degrees (at most %d angle bins)", who, kStructMaxAngleBins);
    return EGNN_EINVAL;
  }
  if (max_cn < 1 || max_cn > kStructMaxCn) { set_error("%s: max_cn %d (1 <= max_cn <= %d)", who, max_cn, kStructMaxCn); return EGNN_EINVAL; }
  return EGNN_OK;
}

int struct_finish_args_check(int B, int A, const void* counts, const void* type, const void* graph_ptr, double R, double dR,
                             double sigma, int nbins, const void* out) {
  if (B < 1 || !counts || !type || !graph_ptr || !out) { set_error("bad egnn_struct_rdf_finish arguments"); return EGNN_EINVAL; }
  if (int rc = atom_types_check("egnn_struct_rdf_finish", A, kStructMaxTypes)) return rc;
  if (nbins < 1 || nbins > kStructMaxBins) { set_error("egnn_struct_rdf_finish: %d radial bins (1 <= nbins <= %d)", nbins, kStructMaxBins); return EGNN_EINVAL; }
  if (!(dR > 0.0) || !(R > 0.0) || !(sigma > 0.0)) { set_error("egnn_struct_rdf_finish: R, dR and sigma must be positive"); return EGNN_EINVAL; }
  if ((long long)B * A * A > 2147483647LL) { set_error("egnn_struct_rdf_finish: B * A * A exceeds the grid"); return EGNN_EINVAL; }
  return EGNN_OK;
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_struct_counts_host(int B, int A, const float* pos, const int32_t* type, const int32_t* graph_ptr, double dR, int nbins,
                            float cutoff, double dtheta, int max_cn, int32_t* counts, int32_t* cn, int32_t* angles, int32_t* overflow) {
  const char* who = "egnn_struct_counts_host";
  if (int rc = struct_pair_args_check(who, B, A, pos, type, graph_ptr, 0, dR, nbins, counts)) return rc;
  if (int rc = struct_bond_args_check(who, B, A, pos, type, graph_ptr, 0, cutoff, dtheta, max_cn, cn, angles)) return rc;
  for (int g = 0; g < B; ++g) {
    const int lo = graph_ptr[g], hi = graph_ptr[g + 1];
    if (lo < 0 || hi < lo) { set_error("%s: graph_ptr must start at 0 or above and not decrease", who); return EGNN_EINVAL; }
    if (int rc = struct_common_check(who, B, A, pos, type, graph_ptr, hi - lo)) return rc;
    if (int rc = type_range_check(who, type, lo, hi, A)) return rc;
  }
  const int nth = struct_angle_bins(dtheta), P = type_pairs(A), ncn = max_cn + 1;
  memset(counts, 0, sizeof(int32_t) * (size_t)B * A * A * nbins);
  memset(cn, 0, sizeof(int32_t) * (size_t)B * A * A * ncn);
  memset(angles, 0, sizeof(int32_t) * (size_t)B * A * P * nth);
  if (overflow) memset(overflow, 0, sizeof(int32_t) * (size_t)B);
  const float inv_dR = (float)(1.0 / dR);
  std::vector<double> bond(3 * (size_t)kMaxNeighbours);
  std::vector<int> bond_type(kMaxNeighbours);
  for (int g = 0; g < B; ++g) {
    const int lo = graph_ptr[g], hi = graph_ptr[g + 1];
    int32_t* c_g = counts + (size_t)g * A * A * nbins;
    int32_t* cn_g = cn + (size_t)g * A * A * ncn;
    int32_t* ang_g = angles + (size_t)g * A * P * nth;
    for (int i = lo; i < hi; ++i) {
      const float* p = pos + 3 * (size_t)i;
      const int ti = type[i];
      int nb[kStructMaxTypes] = {0, 0, 0, 0}, nlist = 0;
      for (int j = lo; j < hi; ++j) {
        if (j == i) continue;
        const float* q = pos + 3 * (size_t)j;
        const int tj = type[j];
        const float d = struct_distance(p[0], p[1], p[2], q[0], q[1], q[2]);
        const int k0 = struct_bin_guess(d, inv_dR, nbins);
        for (int k = k0 - 1; k <= k0 + 1; ++k)
          if (k >= 0 && k < nbins && struct_in_bin(d, k, dR)) ++c_g[((size_t)ti * A + tj) * nbins + k];
        if (d < cutoff) {
          ++nb[tj];
          if (nlist < kMaxNeighbours) {
            for (int x = 0; x < 3; ++x) bond[3 * (size_t)nlist + x] = (double)q[x] - (double)p[x];
            bond_type[nlist] = tj;
          }
          ++nlist;
        }
      }
      for (int b = 0; b < A; ++b) ++cn_g[((size_t)ti * A + b) * ncn + (nb[b] < max_cn ? nb[b] : max_cn)];
      if (nlist > kMaxNeighbours) {   // the device list is full: counted, its angles are not taken
        if (overflow) ++overflow[g];
        continue;
      }
      for (int a = 0; a < nlist; ++a)
        for (int b = a + 1; b < nlist; ++b) {
          const int k = struct_angle_bin(&bond[3 * (size_t)a], &bond[3 * (size_t)b], dtheta, nth);
          if (k >= 0) ++ang_g[((size_t)ti * P + type_pair_index(bond_type[a], bond_type[b], A)) * nth + k];
        }
    }
  }
  return EGNN_OK;
}

}  // extern "C"

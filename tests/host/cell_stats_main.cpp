// Stand-alone run of egnn_cell_stats_host (csrc/cells/cell_stats_host.cpp), built with -fsanitize=address,undefined by
// tests/test_cell_stats_host.py.  Every output array is allocated at EXACTLY its documented size, so that ASan sees a write past a
// histogram: the one-atom cubic cell (the theta series of the simple cubic lattice, an image box of 5 per axis, 1,331 images),
// the two-atom chain and ideal beta-cristobalite in one batch at R = 10 (image boxes 4 and 2; totals 2976 / 1376 / 688, CN 2 and 4,
// 48 tetrahedral and 16 straight angles, eight Q^4), nbins = 1, the exact 3 x 3 x 3 grid of spacing 0.7 A (92 bonds per atom: the
// overflow beyond 64, CN still exact, max_cn = 64 at its largest) and refused arguments, which leave every output alone.
#include <math.h>
#include "../../diffusion_model_amd/csrc/cells/cell_stats_math.h"
#include "../../include/egnn_amd.h"
#include "cell_fixtures.h"

using namespace egnn;
using namespace cell_fixtures;

namespace {

void add_grid(Batch& b) {   // 3 x 3 x 3 atoms, 0.7 A apart: 92 neighbours within 2.0 A (i^2 + j^2 + k^2 <= 8)
  std::vector<double> f;
  std::vector<int32_t> t;
  for (int x = 0; x < 3; ++x)
    for (int y = 0; y < 3; ++y)
      for (int z = 0; z < 3; ++z) {
        f.push_back(x / 3.0); f.push_back(y / 3.0); f.push_back(z / 3.0);
        t.push_back((x + y + z) & 1);
      }
  b.add(2.1, f, t);
}

struct Result {
  std::vector<int64_t> counts, cn, angles, qn_hist;
  std::vector<int32_t> coordination, qn, overflow;
};

Result run(const Batch& b, int A, double dR, int nbins, double dtheta, int max_cn, int former, int bridge) {
  const int C = (int)b.cell_ptr.size() - 1, N = b.cell_ptr.back();
  const int nth = struct_angle_bins(dtheta), P = type_pairs(A);
  Result r;
  r.counts.assign((size_t)C * A * A * nbins, -7);
  r.cn.assign((size_t)C * A * A * (max_cn + 1), -7);
  r.angles.assign((size_t)C * A * P * nth, -7);
  r.qn_hist.assign((size_t)C * (max_cn + 1), -7);
  r.coordination.assign((size_t)N * A, -7);
  r.qn.assign(N, -7);
  r.overflow.assign(C, -7);
  CHECK(egnn_cell_stats_host(C, A, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), dR, nbins, r.counts.data(), 2.0, dtheta,
                             max_cn, former, bridge, r.coordination.data(), r.cn.data(), r.angles.data(), r.qn.data(), r.qn_hist.data(),
                             r.overflow.data()) == EGNN_OK, "%s", egnn_last_error());
  for (int64_t v : r.counts) CHECK(v >= 0, "a count was not written");
  for (int64_t v : r.cn) CHECK(v >= 0, "a CN bin was not written");
  for (int64_t v : r.angles) CHECK(v >= 0, "an angle bin was not written");
  for (int64_t v : r.qn_hist) CHECK(v >= 0, "a Q^n bin was not written");
  for (int32_t v : r.coordination) CHECK(v >= 0, "a coordination was not written");
  for (int32_t v : r.qn) CHECK(v >= -1, "a Q^n was not written");
  for (int32_t v : r.overflow) CHECK(v >= 0, "an overflow count was not written");
  return r;
}

}  // namespace

int main() {
  {   // theta series: one atom, L = 2, bins of 1/16: distances 2 sqrt(n)
    Batch b;
    b.add(2.0, {0.25, 0.5, 0.75}, {0});
    const int theta[17] = {0, 6, 12, 8, 6, 24, 24, 0, 12, 30, 24, 24, 8, 24, 48, 0, 6};
    const int nbins = 130;
    int S[3];
    CHECK(cell_stat_image_box(b.lattice.data(), 0.0625, nbins, S) && S[0] == 5 && S[1] == 5 && S[2] == 5, "image box %d %d %d", S[0], S[1], S[2]);
    std::vector<int64_t> counts(nbins, -7), want(nbins, 0);
    for (int n = 1; n <= 16; ++n) want[(int)floor(2.0 * sqrt((double)n) / 0.0625)] += theta[n];
    CHECK(egnn_cell_stats_host(1, 1, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), 0.0625, nbins, counts.data(), 2.0, 1.0,
                               16, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == EGNN_OK, "%s", egnn_last_error());
    for (int k = 0; k < nbins; ++k) CHECK(counts[k] == want[k], "theta series: bin %d holds %lld, not %lld", k, (long long)counts[k], (long long)want[k]);
  }
  {   // the chain and cristobalite in one batch
    Batch b;
    add_chain(b);
    add_cristobalite(b);
    const int nbins = 1000, nth = 181, P = 3;
    Result r = run(b, 2, 0.01, nbins, 1.0, 16, 1, 0);
    const int64_t want[4] = {2976, 1376, 1376, 688};
    for (int ab = 0; ab < 4; ++ab) {
      int64_t total = 0;
      for (int k = 0; k < nbins; ++k) {
        total += r.counts[((size_t)4 + ab) * nbins + k];
        CHECK(r.counts[((size_t)4 + ab) * nbins + k] == r.counts[((size_t)4 + (ab % 2) * 2 + ab / 2) * nbins + k], "c[a][b] == c[b][a] at bin %d", k);
      }
      CHECK(total == want[ab], "cristobalite: %lld pairs of types %d, %d", (long long)total, ab / 2, ab % 2);
    }
    for (int i = 2; i < 26; ++i) {
      const bool si = b.type[i] == 1;
      CHECK(r.coordination[2 * i] == (si ? 4 : 0) && r.coordination[2 * i + 1] == (si ? 0 : 2), "cristobalite: atom %d", i);
      CHECK(r.qn[i] == (si ? 4 : -1), "cristobalite: Q^n %d at atom %d", r.qn[i], i);
    }
    const int64_t* ang = r.angles.data() + (size_t)2 * P * nth;
    CHECK(ang[((size_t)1 * P + 0) * nth + 109] == 48 && ang[((size_t)0 * P + 2) * nth + 180] == 16, "cristobalite: angles");
    CHECK(r.qn_hist[17 + 4] == 8 && r.overflow[0] == 0 && r.overflow[1] == 0, "cristobalite: Q^4 %lld", (long long)r.qn_hist[17 + 4]);
    CHECK(r.coordination[0] == 2 && r.coordination[3] == 2 && r.qn[0] == 2 && r.qn[1] == -1, "chain: two bonds each, every O bridging");
    Result one = run(b, 2, 10.0, 1, 180.0, 1, 0, 1);   // one radial bin, two angle bins, two CN bins, the roles swapped
    CHECK(one.counts[4] == 2976 && one.counts[7] == 688, "one bin: %lld", (long long)one.counts[4]);
    CHECK(one.qn_hist[2 + 1] == 16 && one.qn[2] == -1, "swapped roles: every O has two bridging Si, the bin saturates at max_cn = 1");
  }
  {   // beyond 64 bonds
    Batch b;
    add_grid(b);
    Result r = run(b, 2, 0.05, 50, 0.5, 64, 1, 0);
    CHECK(r.overflow[0] == 27, "overflow %d", r.overflow[0]);
    for (int i = 0; i < 27; ++i) CHECK(r.coordination[2 * i] + r.coordination[2 * i + 1] == 92, "grid: %d bonds", r.coordination[2 * i] + r.coordination[2 * i + 1]);
    for (int64_t v : r.angles) CHECK(v == 0, "no angle is taken beyond 64 bonds");
    int64_t cn = 0;
    for (int64_t v : r.cn) cn += v;
    CHECK(cn == 54, "every atom counts twice in the CN histogram (%lld)", (long long)cn);
  }
  {   // refused arguments leave every output alone
    Batch b;
    add_chain(b);
    int64_t counts[4] = {-7, -7, -7, -7};
    CHECK(egnn_cell_stats_host(1, 2, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), 0.05, 1100, counts, 2.0, 1.0, 16, 1, 0,
                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == EGNN_EINVAL, "an image box too wide");
    CHECK(egnn_cell_stats_host(1, 2, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), 0.0, 1, counts, 2.0, 1.0, 16, 1, 0,
                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == EGNN_EINVAL, "dR = 0");
    CHECK(counts[0] == -7 && counts[3] == -7, "nothing written");
  }
  printf("CELL-STATS-OK\n");
  return 0;
}

// Stand-alone run of egnn_soap_host (csrc/eval/soap_host.cpp), built with -fsanitize=address,undefined by tests/test_soap_host.py.
// Every array has EXACTLY the size the contract states, so that ASan sees a write past a descriptor row, a coefficient block, a
// cosine matrix or a list of nearest spectra.  The tables here are float64 stand-ins (K, gamma, the norms and the weights from their
// formulas, beta = identity): the program checks memory and argument handling, the accuracy is test_soap_host.py's business.
// Cases: a seeded batch of clouds (1, 2, 5, 65 and 130 atoms, three types) at the small configuration, the same at the limits
// (A = 4, n_max = 16, l_max = 10) and at the smallest basis (n_max = 1, l_max = 0), cosines with and without a pair list, the matrix,
// nearest spectra with groups, with k above the candidates and with exactly equal distances, and every bad-argument case.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../diffusion_model_amd/csrc/eval/soap_math.h"
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

uint64_t g_state = 2468;
double uniform() {   // a small LCG: the program needs no library for its numbers
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) / 9007199254740992.0;
}

double factorial(int n) { return n <= 1 ? 1.0 : n * factorial(n - 1); }

std::vector<double> stand_in_tables(double r_cut, int n_max, int l_max, double sigma) {
  const int L1 = l_max + 1;
  const double a = 1.0 / (2.0 * sigma * sigma), pi = 3.14159265358979323846;
  std::vector<double> t((size_t)soap_table_count(n_max, l_max), 0.0);
  for (int n = 0; n < n_max; ++n)
    for (int l = 0; l < L1; ++l) {
      const double r = n_max > 1 ? 1.0 + (r_cut - 1.0) * n / (n_max - 1) : 1.0;
      const double alpha = -log(1e-3 / pow(r, l)) / (r * r), p = alpha + a;
      t[n * L1 + l] = pow(pi, 1.5) * pow(p, -1.5) * pow(a / p, l);
      t[soap_table_gamma(n_max, l_max) + n * L1 + l] = a * alpha / p;
    }
  for (int l = 0; l < L1; ++l)
    for (int n = 0; n < n_max; ++n) t[soap_table_beta(n_max, l_max) + (l * n_max + n) * n_max + n] = 1.0;
  for (int l = 0; l < L1; ++l) {
    for (int m = -l; m <= l; ++m) {
      const int am = m < 0 ? -m : m;
      t[soap_table_norm(n_max, l_max) + l * l + l + m] = sqrt((2 * l + 1) / (4 * pi) * factorial(l - am) / factorial(l + am)) * (m ? sqrt(2.0) : 1.0);
    }
    t[soap_table_weight(n_max, l_max) + l] = pi * sqrt(8.0 / (2 * l + 1));
  }
  return t;
}

struct Batch {
  std::vector<float> pos;
  std::vector<int32_t> type, graph_ptr{0};
};

Batch clouds(int A) {
  Batch b;
  const int sizes[] = {1, 2, 5, 65, 130};
  for (int n : sizes) {
    const double box = 2.2 * cbrt((double)n);
    for (int i = 0; i < n; ++i) {
      for (int k = 0; k < 3; ++k) b.pos.push_back((float)(box * uniform()));
      b.type.push_back((int32_t)(uniform() * A) % A);
    }
    b.graph_ptr.push_back((int32_t)b.type.size());
  }
  return b;
}

int host(const Batch& b, int A, int n_max, int l_max, double cut, const double* tables, const std::vector<int32_t>& centres, double* desc,
         double* coeff) {
  return egnn_soap_host((int)b.graph_ptr.size() - 1, (int)b.type.size(), A, b.pos.data(), b.type.data(), b.graph_ptr.data(), n_max, l_max, cut,
                        tables, (int)centres.size(), centres.data(), desc, coeff, 0, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, 0,
                        0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

std::vector<double> descriptors(const Batch& b, int A, double r_cut, int n_max, int l_max, const std::vector<int32_t>& centres, bool with_coeff) {
  const std::vector<double> tables = stand_in_tables(r_cut, n_max, l_max, 0.1);
  const int F = egnn_soap_features(A, n_max, l_max);
  CHECK(F == soap_feature_count(A, n_max, l_max) && (int)tables.size() == egnn_soap_table_doubles(n_max, l_max), "F %d", F);
  std::vector<double> desc((size_t)centres.size() * F, -7.0), coeff(with_coeff ? (size_t)centres.size() * A * n_max * soap_lm_count(l_max) : 0, -7.0);
  const int rc = host(b, A, n_max, l_max, r_cut + 0.37, tables.data(), centres, desc.data(), with_coeff ? coeff.data() : nullptr);
  CHECK(rc == 0, "rc %d: %s", rc, egnn_last_error());
  for (double v : desc) CHECK(isfinite(v) && v != -7.0, "a descriptor entry was not written");
  for (double v : coeff) CHECK(isfinite(v) && v != -7.0, "a coefficient was not written");
  return desc;
}

}  // namespace

int main() {
  const Batch b = clouds(3);
  const int N = (int)b.type.size();
  std::vector<int32_t> all(N), some = {N - 1, 0, 3, 3, 1, 70};
  for (int i = 0; i < N; ++i) all[i] = i;
  const std::vector<double> small = descriptors(b, 3, 4.0, 3, 2, all, true);
  const int Fs = egnn_soap_features(3, 3, 2);
  {   // a lone atom of type t: only the (t, t) block, l = 0, is non-zero; repeats and order of the centre list
    const std::vector<double> listed = descriptors(b, 3, 4.0, 3, 2, some, false);
    for (size_t c = 0; c < some.size(); ++c)
      for (int f = 0; f < Fs; ++f) CHECK(listed[c * Fs + f] == small[(size_t)some[c] * Fs + f], "centre %zu feature %d", c, f);
    int nonzero = 0;
    for (int f = 0; f < Fs; ++f) nonzero += small[f] != 0.0;
    CHECK(nonzero == 6, "lone atom: %d non-zero entries", nonzero);   // n <= n' of 3, l = 0
  }
  {   // the limits: every LDS-sized array of the kernel has its host twin here
    const Batch b4 = clouds(4);
    const std::vector<int32_t> first = {0, 1, 3, 8, 73};
    const std::vector<double> big = descriptors(b4, 4, 8.0, 16, 10, first, true);
    CHECK((int)(big.size() / first.size()) == 4 * 136 * 11 + 6 * 256 * 11, "F at the limits: %zu", big.size() / first.size());
    // the other end: one radial function, l = 0 only (a 1 x 1 beta, one harmonic, F = 4 + 6)
    const std::vector<double> tiny = descriptors(b4, 4, 4.0, 1, 0, first, true);
    CHECK(tiny.size() == first.size() * 10, "F of the smallest basis: %zu", tiny.size() / first.size());
    int nonzero = 0;
    for (int f = 0; f < 10; ++f) nonzero += tiny[f] != 0.0;
    CHECK(nonzero == 1, "lone atom, smallest basis: %d non-zero entries", nonzero);
  }
  {   // cosines: the diagonal, a pair list, the matrix
    const int n_a = 70, n_b = 33;
    std::vector<int32_t> pairs = {0, 0, 69, 32, 5, 7};
    std::vector<double> cos_diag(n_b, -7.0), cos_pairs(3, -7.0), gram((size_t)n_a * n_b, -7.0);
    int rc = egnn_soap_host(0, 0, 0, nullptr, nullptr, nullptr, 0, 0, 0.0, nullptr, 0, nullptr, nullptr, nullptr, Fs, small.data(), n_a,
                            small.data() + (size_t)100 * Fs, n_b, n_b, nullptr, cos_diag.data(), gram.data(), 0, 0, 0, 0, nullptr, nullptr,
                            nullptr, nullptr, nullptr, nullptr);
    CHECK(rc == 0, "rc %d: %s", rc, egnn_last_error());
    rc = egnn_soap_host(0, 0, 0, nullptr, nullptr, nullptr, 0, 0, 0.0, nullptr, 0, nullptr, nullptr, nullptr, Fs, small.data(), n_a,
                        small.data() + (size_t)100 * Fs, n_b, 3, pairs.data(), cos_pairs.data(), nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr,
                        nullptr, nullptr, nullptr);
    CHECK(rc == 0, "rc %d: %s", rc, egnn_last_error());
    for (int p = 0; p < n_b; ++p) CHECK(cos_diag[p] == gram[(size_t)p * n_b + p], "diagonal %d", p);
    CHECK(cos_pairs[0] == gram[0] && cos_pairs[1] == gram[(size_t)69 * n_b + 32] && cos_pairs[2] == gram[(size_t)5 * n_b + 7], "pairs");
    for (double v : gram) CHECK(v > -1.0000001 && v < 1.0000001, "cosine %g", v);
    rc = egnn_soap_host(0, 0, 0, nullptr, nullptr, nullptr, 0, 0, 0.0, nullptr, 0, nullptr, nullptr, nullptr, Fs, small.data(), 3, small.data(), 3,
                        3, nullptr, cos_pairs.data(), nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    CHECK(rc == 0 && fabs(cos_pairs[1] - 1.0) < 1e-14, "a row with itself: %.17g", cos_pairs[1]);
  }
  {   // nearest spectra: groups, k above the candidates, nothing left
    const int T = 5, R = 70;
    for (int S : {200, 7}) {
      std::vector<float> t((size_t)T * S), r((size_t)R * S);
      for (float& v : t) v = (float)uniform();
      for (float& v : r) v = (float)uniform();
      std::vector<int32_t> tg = {0, 1, -1, 2, 3}, rg(R);
      for (int i = 0; i < R; ++i) rg[i] = i % 3;
      for (int k : {1, 3, 8}) {
        std::vector<int32_t> idx((size_t)T * k, -7);
        std::vector<double> mse((size_t)T * k, -7.0);
        const int rc = egnn_soap_host(0, 0, 0, nullptr, nullptr, nullptr, 0, 0, 0.0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0,
                                      nullptr, 0, 0, nullptr, nullptr, nullptr, T, R, S, k, t.data(), r.data(), tg.data(), rg.data(),
                                      idx.data(), mse.data());
        CHECK(rc == 0, "rc %d: %s", rc, egnn_last_error());
        for (int q = 0; q < T; ++q)
          for (int j = 0; j < k; ++j) {
            const int at = idx[(size_t)q * k + j];
            CHECK(at >= 0 && at < R && !(tg[q] >= 0 && rg[at] == tg[q]), "target %d entry %d names %d", q, j, at);
            CHECK(j == 0 || mse[(size_t)q * k + j] >= mse[(size_t)q * k + j - 1], "not ascending");
          }
      }
      std::vector<int32_t> one(R, 0), idx(8, -7);
      std::vector<double> mse(8, -7.0);
      int rc = egnn_soap_host(0, 0, 0, nullptr, nullptr, nullptr, 0, 0, 0.0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, 0,
                              nullptr, nullptr, nullptr, 1, R, S, 8, t.data(), r.data(), one.data(), one.data(), idx.data(), mse.data());
      CHECK(rc == 0 && idx[0] == -1 && idx[7] == -1 && isinf(mse[0]), "nothing left: %d", idx[0]);
      rc = egnn_soap_host(0, 0, 0, nullptr, nullptr, nullptr, 0, 0, 0.0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, 0,
                          nullptr, nullptr, nullptr, 1, 3, S, 8, t.data(), r.data(), nullptr, nullptr, idx.data(), mse.data());
      CHECK(rc == 0 && idx[2] >= 0 && idx[3] == -1 && isinf(mse[7]), "k above the candidates: %d", idx[3]);
      // exact ties go to the lower index: references 3, 17, 18 and 40 are one row next to target 0, references 5 and 6 one next to
      // target 1
      for (int s = 0; s < S; ++s) {
        for (int q : {3, 17, 18, 40}) r[(size_t)q * S + s] = t[s] + 0.015625f;
        for (int q : {5, 6}) r[(size_t)q * S + s] = t[(size_t)S + s] - 0.03125f;
      }
      std::vector<int32_t> tie_idx((size_t)T * 8, -7);
      std::vector<double> tie_mse((size_t)T * 8, -7.0);
      rc = egnn_soap_host(0, 0, 0, nullptr, nullptr, nullptr, 0, 0, 0.0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, 0,
                          nullptr, nullptr, nullptr, T, R, S, 8, t.data(), r.data(), nullptr, nullptr, tie_idx.data(), tie_mse.data());
      CHECK(rc == 0, "rc %d: %s", rc, egnn_last_error());
      CHECK(tie_idx[0] == 3 && tie_idx[1] == 17 && tie_idx[2] == 18 && tie_idx[3] == 40 && tie_mse[0] == tie_mse[3], "a four-fold tie: %d %d %d %d",
            tie_idx[0], tie_idx[1], tie_idx[2], tie_idx[3]);
      CHECK(tie_idx[8] == 5 && tie_idx[9] == 6 && tie_mse[8] == tie_mse[9], "a tie of two: %d %d", tie_idx[8], tie_idx[9]);
      for (int q = 0; q < T; ++q)
        for (int j = 1; j < 8; ++j)
          CHECK(tie_mse[(size_t)q * 8 + j] > tie_mse[(size_t)q * 8 + j - 1] || tie_idx[(size_t)q * 8 + j] > tie_idx[(size_t)q * 8 + j - 1],
                "target %d: equal distances out of index order at place %d", q, j);
    }
  }
  {   // bad arguments
    const std::vector<double> tables = stand_in_tables(4.0, 3, 2, 0.1);
    std::vector<int32_t> c = {0};
    std::vector<double> desc(4096, 0.0);
    CHECK(host(b, 3, 3, 2, 4.37, tables.data(), c, desc.data(), nullptr) == 0, "the good call");
    CHECK(host(b, 5, 3, 2, 4.37, tables.data(), c, desc.data(), nullptr) == EGNN_EINVAL, "A = 5");
    CHECK(host(b, 3, 0, 2, 4.37, tables.data(), c, desc.data(), nullptr) == EGNN_EINVAL, "n_max = 0");
    CHECK(host(b, 3, 17, 2, 4.37, tables.data(), c, desc.data(), nullptr) == EGNN_EINVAL, "n_max = 17");
    CHECK(host(b, 3, 3, -1, 4.37, tables.data(), c, desc.data(), nullptr) == EGNN_EINVAL, "l_max = -1");
    CHECK(host(b, 3, 3, 11, 4.37, tables.data(), c, desc.data(), nullptr) == EGNN_EINVAL, "l_max = 11");
    CHECK(host(b, 3, 3, 2, 0.0, tables.data(), c, desc.data(), nullptr) == EGNN_EINVAL, "cut = 0");
    CHECK(host(b, 3, 3, 2, NAN, tables.data(), c, desc.data(), nullptr) == EGNN_EINVAL, "cut = NaN");
    CHECK(host(b, 3, 3, 2, INFINITY, tables.data(), c, desc.data(), nullptr) == EGNN_EINVAL, "cut = inf");
    CHECK(host(b, 3, 3, 2, 4.37, nullptr, c, desc.data(), nullptr) == EGNN_EINVAL, "no tables");
    CHECK(host(b, 3, 3, 2, 4.37, tables.data(), c, nullptr, nullptr) == EGNN_EINVAL, "no desc");
    c[0] = N;
    CHECK(host(b, 3, 3, 2, 4.37, tables.data(), c, desc.data(), nullptr) == EGNN_EINVAL, "centre N");
    c[0] = -1;
    CHECK(host(b, 3, 3, 2, 4.37, tables.data(), c, desc.data(), nullptr) == EGNN_EINVAL, "centre -1");
    c[0] = 0;
    CHECK(host(b, 2, 3, 2, 4.37, tables.data(), c, desc.data(), nullptr) == EGNN_EINVAL, "a type outside [0, A)");
    CHECK(egnn_soap_features(5, 3, 2) == EGNN_EINVAL && egnn_soap_features(2, 15, 10) == 5115, "features");
  }
  printf("SOAP-OK\n");
  return 0;
}

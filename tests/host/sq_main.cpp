// Stand-alone run of egnn_sq_host and egnn_sq_cell_plan (csrc/eval/sq_host.cpp), built with -fsanitize=address,undefined by
// tests/test_sq_host.py.  Every array has EXACTLY the size the contract states, so that ASan sees a write past a Debye row, a
// vector list or a shell array.  The program checks memory and argument handling and a few exact values; the accuracy is
// test_sq_host.py's business.  Cases: a seeded ragged batch of clouds (0, 1, 2, 65 and 130 atoms) at A = 1, 3 and 4 with and
// without the cut and the Lorch window, cells (one atom, a triclinic box of 24, a box too small for any vector) with the size
// call followed by the list call, lists that are too short, and every bad-argument case.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../diffusion_model_amd/csrc/eval/sq_math.h"
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

uint64_t g_state = 97531;
double uniform() {   // a small LCG: the program needs no library for its numbers
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) / 9007199254740992.0;
}

struct Batch {
  std::vector<float> pos;
  std::vector<int32_t> type, graph_ptr{0};
};

Batch clouds(int A) {
  Batch b;
  const int sizes[] = {0, 1, 2, 65, 130};
  for (int n : sizes) {
    const double box = cbrt(15.6 * (n ? n : 1));
    for (int i = 0; i < n; ++i) {
      for (int k = 0; k < 3; ++k) b.pos.push_back((float)(box * uniform()));
      b.type.push_back((int32_t)(uniform() * A) % A);
    }
    b.graph_ptr.push_back((int32_t)b.type.size());
  }
  return b;
}

int debye(const Batch& b, int A, const std::vector<double>& q, double r_max, int window, double* out) {
  return egnn_sq_host((int)b.graph_ptr.size() - 1, (int)b.type.size(), A, b.pos.data(), b.type.data(), b.graph_ptr.data(), (int)q.size(),
                      q.data(), r_max, window, out, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0, 0, 0, nullptr, nullptr, nullptr,
                      nullptr, nullptr, nullptr, nullptr, nullptr);
}

struct Cells {
  std::vector<int32_t> cell_ptr{0}, type;
  std::vector<double> lattice, frac;
  void add(const double* L, int n, int A) {
    for (int t = 0; t < 9; ++t) lattice.push_back(L[t]);
    for (int i = 0; i < n; ++i) {
      for (int k = 0; k < 3; ++k) frac.push_back(3.0 * uniform() - 1.0);   // outside [0, 1) too
      type.push_back((int32_t)(uniform() * A) % A);
    }
    cell_ptr.push_back((int32_t)type.size());
  }
};

int cells_call(const Cells& c, int A, double q_max, double dq, int nbins, int64_t cap, int64_t* vec_ptr, int32_t* hkl, double* ka, int32_t* bin,
               double* rho, int64_t* count, double* mean_k, double* s) {
  return egnn_sq_host(0, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, 0.0, 0, nullptr, (int)c.cell_ptr.size() - 1, (int)c.type.size(), A,
                      c.cell_ptr.data(), c.lattice.data(), c.frac.data(), c.type.data(), q_max, dq, nbins, cap, vec_ptr, hkl, ka, bin, rho,
                      count, mean_k, s);
}

}  // namespace

int main() {
  const std::vector<double> q = {0.0, 0.05, 1.5, 7.3, 25.0, 0.0};
  const int Q = (int)q.size();
  for (int A : {1, 3, 4}) {
    const Batch b = clouds(A);
    const int B = (int)b.graph_ptr.size() - 1;
    std::vector<double> D((size_t)B * A * A * Q, -7.0), cut(D.size(), -7.0), lorch(D.size(), -7.0);
    CHECK(debye(b, A, q, INFINITY, 0, D.data()) == 0, "%s", egnn_last_error());
    CHECK(debye(b, A, q, 5.0, 0, cut.data()) == 0, "%s", egnn_last_error());
    CHECK(debye(b, A, q, 5.0, 1, lorch.data()) == 0, "%s", egnn_last_error());
    for (int g = 0; g < B; ++g) {
      int n[kSqMaxTypes] = {0, 0, 0, 0};
      for (int i = b.graph_ptr[g]; i < b.graph_ptr[g + 1]; ++i) ++n[b.type[i]];
      for (int a = 0; a < A; ++a)
        for (int c = 0; c < A; ++c) {
          const double* row = &D[(((size_t)g * A + a) * A + c) * Q];
          CHECK(row[0] == (double)n[a] * n[c] - (a == c ? n[a] : 0) && row[5] == row[0], "D(0) of graph %d (%d, %d): %.17g", g, a, c, row[0]);
          for (int k = 0; k < Q; ++k) {
            CHECK(row[k] == D[(((size_t)g * A + c) * A + a) * Q + k], "symmetry");
            CHECK(isfinite(cut[&row[k] - D.data()]) && isfinite(lorch[&row[k] - D.data()]), "a cut sum was not written");
          }
        }
    }
  }
  {   // cells: sizes first, then the lists at exactly their sizes; lists that are too short are left alone
    const double tri[9] = {7.26, 0.0, -0.89, -0.31, 6.96, 0.73, 0.0, 0.0, 7.5}, one[9] = {5, 0, 0, 0, 5, 0, 0, 0, 5},
                 tiny[9] = {0.9, 0, 0, 0, 0.9, 0, 0, 0, 0.9};
    Cells c;
    c.add(one, 1, 2);
    c.add(tri, 24, 2);
    c.add(tiny, 3, 2);
    c.add(one, 0, 2);
    const int C = 4, A = 2, nbins = 24;
    std::vector<int64_t> vec_ptr(C + 1, -7);
    CHECK(cells_call(c, A, 6.0, 0.25, nbins, 0, vec_ptr.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0, "%s",
          egnn_last_error());
    const int64_t K = vec_ptr[C];
    CHECK(vec_ptr[0] == 0 && vec_ptr[1] > 100 && vec_ptr[2] - vec_ptr[1] > 500 && vec_ptr[3] == vec_ptr[2] && K - vec_ptr[3] == vec_ptr[1],
          "vec_ptr %lld %lld %lld %lld", (long long)vec_ptr[1], (long long)vec_ptr[2], (long long)vec_ptr[3], (long long)K);
    std::vector<int32_t> hkl(3 * (size_t)K, -7), bin((size_t)K, -7);
    std::vector<double> ka((size_t)K, -7.0), rho((size_t)K * A * 2, -7.0), mean_k((size_t)C * nbins, -7.0), s((size_t)C * A * A * nbins, -7.0);
    std::vector<int64_t> count((size_t)C * nbins, -7);
    CHECK(cells_call(c, A, 6.0, 0.25, nbins, K, vec_ptr.data(), hkl.data(), ka.data(), bin.data(), rho.data(), count.data(), mean_k.data(),
                     s.data()) == 0, "%s", egnn_last_error());
    int64_t total = 0;
    for (int64_t v = 0; v < K; ++v) {
      CHECK(sq_half_space(hkl[3 * v], hkl[3 * v + 1], hkl[3 * v + 2]) && ka[v] > 0.0 && ka[v] < 6.0 && bin[v] == (int)floor(ka[v] / 0.25),
            "vector %lld", (long long)v);
      CHECK(v == 0 || v == vec_ptr[1] || v == vec_ptr[3] || hkl[3 * v] > hkl[3 * v - 3] ||
                (hkl[3 * v] == hkl[3 * v - 3] && (hkl[3 * v + 1] > hkl[3 * v - 2] || (hkl[3 * v + 1] == hkl[3 * v - 2] && hkl[3 * v + 2] > hkl[3 * v - 1]))),
            "order at %lld", (long long)v);
      for (int t = 0; t < 2 * A; ++t) CHECK(isfinite(rho[v * 2 * A + t]), "rho was not written");
    }
    for (int64_t v = 0; v < vec_ptr[1]; ++v) {   // one atom: |rho| = 1 for its type, 0 for the other
      const int t = c.type[0];
      CHECK(fabs(hypot(rho[(v * A + t) * 2], rho[(v * A + t) * 2 + 1]) - 1.0) < 1e-14 && rho[(v * A + 1 - t) * 2] == 0.0, "one atom");
    }
    for (size_t t = 0; t < count.size(); ++t) {
      CHECK(count[t] >= 0 && count[t] % 2 == 0 && (count[t] > 0) == isfinite(mean_k[t]), "shell %zu", t);
      total += count[t];
    }
    CHECK(total == 2 * K, "counts %lld", (long long)total);
    for (int n = 0; n < nbins; ++n) CHECK(count[2 * nbins + n] == 0 && isnan(s[(size_t)2 * A * A * nbins + n]), "the empty cells");
    std::vector<int32_t> few(3 * (size_t)(K - 1), -7);
    CHECK(cells_call(c, A, 6.0, 0.25, nbins, K - 1, vec_ptr.data(), few.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0,
          "a short list");
    CHECK(few[0] == hkl[0] && few.back() == hkl[3 * (size_t)(K - 1) - 1], "a short list holds the first K - 1 vectors");
    std::vector<int32_t> plan(4 * C, -7);
    int32_t n_rows = -7;
    CHECK(egnn_sq_cell_plan(C, c.lattice.data(), 6.0, plan.data(), &n_rows) == 0 && plan[0] == 5 && plan[3] == 0 && plan[7] == 6 * 11 &&
              n_rows == plan[4 * (C - 1) + 3] + 6 * 11, "plan: %d rows", n_rows);
    // bad arguments
    CHECK(cells_call(c, 5, 6.0, 0.25, nbins, 0, vec_ptr.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == EGNN_EINVAL, "A = 5");
    CHECK(cells_call(c, 1, 6.0, 0.25, nbins, 0, vec_ptr.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == EGNN_EINVAL, "a type");
    CHECK(cells_call(c, A, 6.0, 0.25, 25, 0, vec_ptr.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == EGNN_EINVAL, "nbins");
    CHECK(cells_call(c, A, 6.0, 0.001, 6000, 0, vec_ptr.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == EGNN_EINVAL, "6000 bins");
    CHECK(cells_call(c, A, 1287.0, 1.0, 1287, 0, vec_ptr.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == EGNN_EINVAL, "|h| > 1023");
    CHECK(cells_call(c, A, NAN, 0.25, nbins, 0, vec_ptr.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == EGNN_EINVAL, "q_max NaN");
    CHECK(cells_call(c, A, 6.0, 0.25, nbins, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == EGNN_EINVAL, "no vec_ptr");
    Cells flat = c;
    flat.lattice[9 + 6] = flat.lattice[9 + 0] + flat.lattice[9 + 3];   // the triclinic cell: c = a + b
    flat.lattice[9 + 7] = flat.lattice[9 + 1] + flat.lattice[9 + 4];
    flat.lattice[9 + 8] = flat.lattice[9 + 2] + flat.lattice[9 + 5];
    CHECK(cells_call(flat, A, 6.0, 0.25, nbins, 0, vec_ptr.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == EGNN_EINVAL, "singular");
    Cells wrong = c;
    wrong.cell_ptr[2] = 0;
    CHECK(cells_call(wrong, A, 6.0, 0.25, nbins, 0, vec_ptr.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == EGNN_EINVAL, "cell_ptr");
    wrong = c;
    wrong.frac[4] = INFINITY;
    CHECK(cells_call(wrong, A, 6.0, 0.25, nbins, 0, vec_ptr.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == EGNN_EINVAL, "frac");
  }
  {   // bad arguments of the Debye part
    const Batch b = clouds(2);
    std::vector<double> out((size_t)5 * 4 * 4 * 4097, 0.0), qq = {0.5, 1.0};
    CHECK(debye(b, 2, qq, INFINITY, 0, out.data()) == 0, "the good call");
    CHECK(debye(b, 5, qq, INFINITY, 0, out.data()) == EGNN_EINVAL, "A = 5");
    CHECK(debye(b, 1, qq, INFINITY, 0, out.data()) == EGNN_EINVAL, "a type outside [0, A)");
    CHECK(debye(b, 2, std::vector<double>(4097, 1.0), INFINITY, 0, out.data()) == EGNN_EINVAL, "Q = 4097");
    CHECK(debye(b, 2, std::vector<double>(4096, 1.0), INFINITY, 0, out.data()) == 0, "Q = 4096");
    CHECK(debye(b, 2, {0.5, -1e-300}, INFINITY, 0, out.data()) == EGNN_EINVAL, "q < 0");
    CHECK(debye(b, 2, {NAN}, INFINITY, 0, out.data()) == EGNN_EINVAL && debye(b, 2, {INFINITY}, INFINITY, 0, out.data()) == EGNN_EINVAL, "q not finite");
    CHECK(debye(b, 2, qq, INFINITY, 1, out.data()) == EGNN_EINVAL, "Lorch without r_max");
    CHECK(debye(b, 2, qq, 0.0, 0, out.data()) == EGNN_EINVAL && debye(b, 2, qq, NAN, 0, out.data()) == EGNN_EINVAL, "r_max");
    CHECK(debye(b, 2, qq, 5.0, 2, out.data()) == EGNN_EINVAL, "window 2");
    CHECK(debye(b, 2, qq, INFINITY, 0, nullptr) == EGNN_EINVAL, "no output");
    Batch w = b;
    w.graph_ptr.back() -= 1;
    CHECK(debye(w, 2, qq, INFINITY, 0, out.data()) == EGNN_EINVAL, "graph_ptr ends below N");
    w = b;
    w.graph_ptr[0] = 1;
    CHECK(debye(w, 2, qq, INFINITY, 0, out.data()) == EGNN_EINVAL, "graph_ptr starts above 0");
    w = b;
    w.graph_ptr[2] = 300;
    CHECK(debye(w, 2, qq, INFINITY, 0, out.data()) == EGNN_EINVAL, "graph_ptr decreases");
  }
  printf("SQ-OK\n");
  return 0;
}

// Stand-alone run of egnn_topo_host (csrc/eval/topo_host.cpp), built with -fsanitize=address,undefined by tests/test_topo_host.py.
// Every case runs twice: first with the 32 N neighbour entries of the contract, then with every array at EXACTLY the size the first
// run used (the bond list cut to row_ptr[N]), so that ASan sees a write past a list, a distance block or a fingerprint row.  Cases:
// the 1024-atom zig-zag chain (distance 1023), a star of degree 8 (the class modulus wraps), 34 atoms inside one threshold (degree
// 33: overflow, no fingerprint), and a seeded batch of clouds with a one-atom graph and an empty graph in it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../diffusion_model_amd/csrc/eval/topo_math.h"
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

struct Batch {
  std::vector<float> pos;
  std::vector<int32_t> type, graph_ptr{0};
  void atom(double x, double y, double z, int t) {
    pos.push_back((float)x); pos.push_back((float)y); pos.push_back((float)z);
    type.push_back(t);
  }
  void close() { graph_ptr.push_back((int32_t)type.size()); }
};

struct Out {
  std::vector<int32_t> row_ptr, neighbours, degree, overflow, component, fragments, fp;
  std::vector<uint16_t> dist;
  std::vector<double> sim;
  std::vector<int64_t> sa, sb;
};

uint64_t g_state = 12345;
double uniform() {   // a small LCG: the program needs no library for its numbers
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) / 9007199254740992.0;
}

const double kRadii[2] = {0.66, 1.11};

Out run(const Batch& b, int L, size_t n_neighbours) {
  const int B = (int)b.graph_ptr.size() - 1, N = (int)b.type.size(), A = 2;
  double thr[4];
  for (int a = 0; a < 2; ++a)
    for (int c = 0; c < 2; ++c) thr[a * 2 + c] = 1.2 * (kRadii[a] + kRadii[c]);
  size_t nd = 0;
  for (int g = 0; g < B; ++g) {
    const size_t n = (size_t)(b.graph_ptr[g + 1] - b.graph_ptr[g]);
    nd += n * n;
  }
  Out o;
  o.row_ptr.assign(N + 1, -7); o.neighbours.assign(n_neighbours, -7); o.degree.assign(N, -7); o.overflow.assign(B, -7);
  o.component.assign(N, -7); o.fragments.assign(B, -7); o.fp.assign((size_t)B * topo_keys(A, L), -7); o.dist.assign(nd, 7);
  std::vector<int32_t> pairs;
  for (int g = 0; g < B; ++g) { pairs.push_back(g); pairs.push_back((g + 1) % B); }
  o.sim.assign(B, -7.0); o.sa.assign(B, -7); o.sb.assign(B, -7);
  const int rc = egnn_topo_host(B, A, b.pos.data(), b.type.data(), b.graph_ptr.data(), thr, L, o.row_ptr.data(), o.neighbours.data(),
                                o.degree.data(), o.overflow.data(), o.dist.data(), o.component.data(), o.fragments.data(), o.fp.data(),
                                B, pairs.data(), o.sim.data(), o.sa.data(), o.sb.data());
  CHECK(rc == 0, "rc %d: %s", rc, egnn_last_error());
  return o;
}

Out run_twice(const Batch& b, int L) {
  const Out first = run(b, L, (size_t)kTopoMaxDegree * b.type.size());
  const Out exact = run(b, L, (size_t)first.row_ptr.back());
  CHECK(first.row_ptr == exact.row_ptr && first.degree == exact.degree && first.fp == exact.fp && first.dist == exact.dist &&
            first.component == exact.component && first.fragments == exact.fragments && first.sim == exact.sim,
        "two runs differ");
  for (size_t k = 0; k < exact.neighbours.size(); ++k) CHECK(exact.neighbours[k] == first.neighbours[k], "neighbour %zu", k);
  return exact;
}

}  // namespace

int main() {
  {   // the chain
    Batch b;
    for (int i = 0; i < 1024; ++i) b.atom(1.4 * i, 0.9 * (i % 2), 0.0, i % 2);
    b.close();
    const Out o = run_twice(b, 64);
    CHECK(o.overflow[0] == 0 && o.fragments[0] == 1 && o.row_ptr[1024] == 2 * 1023, "chain: %d bonds", o.row_ptr[1024]);
    CHECK(o.dist[1023] == 1023 && o.dist[(size_t)1023 * 1024] == 1023 && o.dist[(size_t)5 * 1024 + 5] == 0, "chain: distance %d", o.dist[1023]);
    CHECK(o.component[1023] == 0 && o.sim[0] == 1.0, "chain: component %d", o.component[1023]);
    int64_t total = 0;
    for (int32_t v : o.fp) total += v;
    int64_t want = 0;
    for (int d = 1; d <= 64; ++d) want += 1024 - d;
    CHECK(total == want && o.sa[0] == want, "chain: %lld pairs within 64 bonds", (long long)total);
  }
  {   // the star and the crowd, in one batch with a bondless graph
    Batch b;
    b.atom(0, 0, 0, 1);
    const double e = 1.9 / 1.7320508075688772;
    for (int k = 0; k < 8; ++k) b.atom(k & 4 ? e : -e, k & 2 ? e : -e, k & 1 ? e : -e, 0);
    b.close();
    for (int i = 0; i < 34; ++i) b.atom(1.5 * uniform(), 1.5 * uniform(), 1.5 * uniform(), 1);
    b.close();
    for (int i = 0; i < 5; ++i) b.atom(5.0 * i, 0, 0, i % 2);
    b.close();
    const Out o = run_twice(b, 30);
    CHECK(o.degree[0] == 8 && o.overflow[0] == 0 && o.fragments[0] == 1, "star: degree %d", o.degree[0]);
    CHECK(o.fp[(size_t)topo_key(topo_class(0, 1), topo_class(1, 8), 1, 14, 30)] == 8 && topo_class(1, 8) == topo_class(1, 1), "star: key");
    CHECK(o.overflow[1] == 34 && o.fragments[1] == -1 && o.degree[9] == 33 && o.component[9] == -1, "crowd: overflow %d", o.overflow[1]);
    CHECK(o.row_ptr[9 + 34] - o.row_ptr[9] == 34 * 32 && o.dist[81] == kTopoUnreachable, "crowd: %d list entries", o.row_ptr[43] - o.row_ptr[9]);
    for (int k = 0; k < topo_keys(2, 30); ++k) CHECK(o.fp[(size_t)topo_keys(2, 30) + k] == 0, "crowd: key %d", k);
    CHECK(o.fragments[2] == 5 && o.sim[1] == 0.0 && o.sa[2] == 0, "bondless: %d fragments", o.fragments[2]);
  }
  {   // seeded clouds
    Batch b;
    const int sizes[] = {1, 0, 2, 3, 63, 64, 65, 129};
    for (int n : sizes) {
      const double box = 2.5 * cbrt((double)(n > 0 ? n : 1));
      for (int i = 0; i < n; ++i) b.atom(box * uniform(), box * uniform(), box * uniform(), uniform() < 0.67 ? 0 : 1);
      b.close();
    }
    const Out o = run_twice(b, 30);
    int64_t total = 0;
    for (int32_t v : o.fp) total += v;
    CHECK(total > 500 && o.fragments[0] == 1 && o.fragments[1] == 0, "clouds: %lld pairs", (long long)total);
    for (size_t g = 0; g < 8; ++g) CHECK(o.overflow[g] == 0 && o.sim[g] >= 0.0 && o.sim[g] <= 1.0, "clouds: graph %zu", g);
  }
  printf("TOPO-OK\n");
  return 0;
}

// Stand-alone test of the host side of the training GEMMs (csrc/host_logic.cpp): the split-K plan of egnn_gemm_tn_bf16 and the
// argument checks of both GEMMs, built with -fsanitize=address,undefined by tests/test_gemm_plan_host.py.  No GPU: the checks
// never dereference the operand pointers, so the pointers here are made-up addresses.
//   usage: gemm_plan_main <case file>
// The case file is written by the test from tests/_gemm_cases.py, one case per line:
//   tn   E M N rows cols lda ldb
//   rows E K0 K1 lda0 lda1 ldo out_f32 n_chunks
// For every tn line the program prints "PLAN E M N BN tiles_n S steps_per_slice" (the test compares these with the Python
// restatement), checks that the argument checks accept the case and refuse its bad variants, and remembers (M, N); then it
// sweeps E = 1 .. 40000 over every (M, N) seen and checks the invariants of the plan.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <utility>

#include "../../diffusion_model_amd/csrc/host_logic.h"

using namespace egnn;

namespace {

int g_checks = 0, g_failed = 0;

#define EXPECT(cond, ...)                                  \
  do {                                                     \
    ++g_checks;                                            \
    if (!(cond)) {                                         \
      ++g_failed;                                          \
      printf("FAILED %s:%d %s : ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                 \
      printf("\n");                                        \
    }                                                      \
  } while (0)

const void* at(uintptr_t address) { return reinterpret_cast<const void*>(address); }
constexpr uintptr_t kBase = 1u << 20;   // a 16-byte aligned made-up device address

void tn_case(int E, int M, int N, int rows, int cols, int lda, int ldb) {
  int BN, tiles_n, S, sps;
  plan_gemm_tn(E, M, N, BN, tiles_n, S, sps);
  printf("PLAN %d %d %d %d %d %d %d\n", E, M, N, BN, tiles_n, S, sps);
  const size_t need = egnn_gemm_tn_workspace_bytes(E, M, N);
  EXPECT(need == (size_t)S * M * N * 4, "E=%d M=%d N=%d need=%zu", E, M, N, need);
  const void *A = at(kBase), *B = at(2 * kBase), *C = at(3 * kBase), *W = at(4 * kBase);
  const int ldc = cols + 8;
  EXPECT(gemm_tn_args_check(E, M, N, A, lda, B, ldb, C, ldc, rows, cols, W, need) == EGNN_OK, "E=%d M=%d N=%d: %s", E, M, N, egnn_last_error());
  // bad variants: one byte of workspace short, a stride below the operand width or no multiple of 8, ldc < cols, rows > M
  EXPECT(gemm_tn_args_check(E, M, N, A, lda, B, ldb, C, ldc, rows, cols, W, need - 1) == EGNN_EINVAL, "workspace");
  EXPECT(gemm_tn_args_check(E, M, N, A, M - 8, B, ldb, C, ldc, rows, cols, W, need) == EGNN_EINVAL, "lda < M");
  EXPECT(gemm_tn_args_check(E, M, N, A, lda + 4, B, ldb, C, ldc, rows, cols, W, need) == EGNN_EINVAL, "lda %% 8");
  EXPECT(gemm_tn_args_check(E, M, N, A, lda, B, ldb + 2, C, ldc, rows, cols, W, need) == EGNN_EINVAL, "ldb %% 8");
  EXPECT(gemm_tn_args_check(E, M, N, A, lda, B, ldb, C, cols - 1, rows, cols, W, need) == EGNN_EINVAL, "ldc < cols");
  EXPECT(gemm_tn_args_check(E, M, N, A, lda, B, ldb, C, ldc, M + 1, cols, W, need) == EGNN_EINVAL, "rows > M");
  // a view that starts inside a 16-byte piece (any bf16 column offset that is no multiple of 8)
  for (uintptr_t off = 2; off < 16; off += 2) {
    EXPECT(gemm_tn_args_check(E, M, N, at(kBase + off), lda, B, ldb, C, ldc, rows, cols, W, need) == EGNN_EINVAL, "A + %d", (int)off);
    EXPECT(gemm_tn_args_check(E, M, N, A, lda, at(2 * kBase + off), ldb, C, ldc, rows, cols, W, need) == EGNN_EINVAL, "B + %d", (int)off);
  }
  EXPECT(strstr(egnn_last_error(), "16-byte") != nullptr, "%s", egnn_last_error());
  EXPECT(gemm_tn_args_check(E, M, N, at(kBase + 16), lda, at(2 * kBase + 32), ldb, C, ldc, rows, cols, W, need) == EGNN_OK, "aligned views");
}

void rows_case(int E, int K0, int K1, int lda0, int lda1, int ldo, int f32, int chunks) {
  const void *A0 = at(kBase), *W0 = at(2 * kBase), *O = at(5 * kBase);
  const void *A1 = K1 ? at(3 * kBase) : nullptr, *W1 = K1 ? at(4 * kBase) : nullptr;
  EXPECT(gemm_rows_args_check(E, A0, lda0, K0, W0, A1, lda1, K1, W1, O, ldo) == EGNN_OK, "E=%d K=%d+%d: %s", E, K0, K1, egnn_last_error());
  EXPECT(gemm_rows_out_check(O, ldo, f32, chunks) == EGNN_OK, "E=%d ldo=%d f32=%d chunks=%d: %s", E, ldo, f32, chunks, egnn_last_error());
  // the output side.  bf16 rows are stored in 16-byte pieces: ldo % 8 and an aligned base; fp32 element by element: ldo % 4
  EXPECT(gemm_rows_out_check(O, ldo + 4, 0, chunks) == EGNN_EINVAL, "bf16 ldo %% 8");
  EXPECT(gemm_rows_out_check(O, ldo + 4, 1, chunks) == EGNN_OK, "fp32 ldo %% 4: %s", egnn_last_error());
  EXPECT(gemm_rows_args_check(E, A0, lda0, K0, W0, A1, lda1, K1, W1, O, ldo + 2) == EGNN_EINVAL, "ldo %% 4");
  EXPECT(gemm_rows_out_check(at(5 * kBase + 8), ldo, 0, chunks) == EGNN_EINVAL, "bf16 out + 8 bytes");
  EXPECT(gemm_rows_out_check(at(5 * kBase + 16), ldo, 0, chunks) == EGNN_OK, "bf16 out + 16 bytes");
  EXPECT(gemm_rows_out_check(O, 128 * chunks - 8, f32, chunks) == EGNN_EINVAL, "ldo < 128 chunks");
  EXPECT(gemm_rows_out_check(O, ldo, f32, 0) == EGNN_EINVAL, "no chunk");
  // the operand side
  EXPECT(gemm_rows_args_check(E, at(kBase + 8), lda0, K0, W0, A1, lda1, K1, W1, O, ldo) == EGNN_EINVAL, "A0 + 8");
  EXPECT(gemm_rows_args_check(E, A0, lda0, K0, at(2 * kBase + 2), A1, lda1, K1, W1, O, ldo) == EGNN_EINVAL, "W0 + 2");
  EXPECT(gemm_rows_args_check(E, A0, lda0 + 4, K0, W0, A1, lda1, K1, W1, O, ldo) == EGNN_EINVAL, "lda0 %% 8");
  EXPECT(gemm_rows_args_check(E, A0, K0 - 8, K0, W0, A1, lda1, K1, W1, O, ldo) == EGNN_EINVAL, "lda0 < K0");
  if (K1) {
    EXPECT(gemm_rows_args_check(E, A0, lda0, K0, W0, at(3 * kBase + 4), lda1, K1, W1, O, ldo) == EGNN_EINVAL, "A1 + 4");
    EXPECT(gemm_rows_args_check(E, A0, lda0, K0, W0, A1, lda1, K1, at(4 * kBase + 8), O, ldo) == EGNN_EINVAL, "W1 + 8");
    EXPECT(gemm_rows_args_check(E, A0, lda0, K0, W0, A1, lda1, K1, nullptr, O, ldo) == EGNN_EINVAL, "A1 without W1");
    EXPECT(gemm_rows_args_check(E, A0, lda0, K0, W0, at(kBase + 2 * 72), lda0 + lda1, K1, W1, O, ldo) == EGNN_OK, "A1 as an aligned column view of A0");
  }
}

void sweep(int M, int N) {
  for (int E = 1; E <= 40000; ++E) {
    int BN, tiles_n, S, sps;
    plan_gemm_tn(E, M, N, BN, tiles_n, S, sps);
    const int total = (E + kGemmBK - 1) / kGemmBK;
    const bool ok = (BN == 128 || BN == 256) && tiles_n >= 1 && tiles_n * BN == N && S >= 1 && sps >= 1 &&
                    (long long)(S - 1) * sps < total &&      // every slice, the last one too, has at least one step
                    (long long)S * sps >= total &&           // and every step lies in a slice
                    egnn_gemm_tn_workspace_bytes(E, M, N) == (size_t)S * M * N * 4;
    ++g_checks;
    if (!ok) {
      ++g_failed;
      printf("FAILED sweep E=%d M=%d N=%d: BN=%d tiles_n=%d S=%d sps=%d\n", E, M, N, BN, tiles_n, S, sps);
      if (g_failed > 20) return;
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { printf("usage: gemm_plan_main <case file>\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
  std::set<std::pair<int, int>> mn;
  char line[256];
  int n_tn = 0, n_rows = 0;
  while (fgets(line, sizeof line, f)) {
    int v[8];
    if (sscanf(line, "tn %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6) == 7) {
      tn_case(v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
      mn.insert({v[1], v[2]});
      ++n_tn;
    } else if (sscanf(line, "rows %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7) == 8) {
      rows_case(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
      ++n_rows;
    } else {
      printf("FAILED: unreadable case line: %s", line);
      ++g_failed;
    }
  }
  fclose(f);
  for (const auto& p : mn) {
    printf("SWEEP %d %d\n", p.first, p.second);
    sweep(p.first, p.second);
  }
  EXPECT(egnn_gemm_tn_workspace_bytes(0, 256, 128) == 0 && egnn_gemm_tn_workspace_bytes(5, 255, 128) == 0 &&
             egnn_gemm_tn_workspace_bytes(5, 256, 64) == 0, "unsupported shapes report no workspace");
  printf("cases: %d tn, %d rows; %d checks, %d failed\n", n_tn, n_rows, g_checks, g_failed);
  if (g_failed == 0 && n_tn > 0 && n_rows > 0) printf("GEMM-PLAN-OK\n");
  return g_failed == 0 ? 0 : 1;
}

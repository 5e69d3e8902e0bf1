// Stand-alone test of the per-device "dynamic-LDS limit already raised" record (csrc/eval/lds_limit.h), built with
// -fsanitize=address,undefined by tests/test_lds_limit_host.py.  A fresh record answers "not yet" for every device it remembers;
// marking one device changes that device only; an index outside the table always answers "not yet"; two threads that mark the
// same device leave it marked.
#include <stdio.h>
#include <stdlib.h>

#include <thread>

#include "../../diffusion_model_amd/csrc/eval/lds_limit.h"

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

// static, as every record in the library
LdsLimitRecord fresh, one, outside, shared;

}  // namespace

int main() {
  static_assert(LdsLimitRecord::kDevices == 64, "the table remembers 64 devices");
  for (int d = 0; d < 64; ++d) CHECK(!fresh.is_raised(d), "a fresh record says device %d is raised", d);

  one.mark(0);
  CHECK(one.is_raised(0), "device 0 is not marked");
  for (int d = 1; d < 64; ++d) CHECK(!one.is_raised(d), "marking device 0 marked device %d", d);
  CHECK(!fresh.is_raised(0), "marking one record marked another");

  for (int d : {-1, 64}) {
    CHECK(!outside.is_raised(d), "device %d answers raised before any mark", d);
    outside.mark(d);
    CHECK(!outside.is_raised(d), "device %d answers raised after a mark", d);
  }
  for (int d = 0; d < 64; ++d) CHECK(!outside.is_raised(d), "a mark outside the table marked device %d", d);

  std::thread a([] { shared.mark(5); }), b([] { shared.mark(5); });
  a.join();
  b.join();
  CHECK(shared.is_raised(5), "two threads marked device 5 and it is not marked");
  for (int d = 0; d < 64; ++d) CHECK(d == 5 || !shared.is_raised(d), "two threads marking device 5 marked device %d", d);

  printf("LDS-LIMIT-OK\n");
  return 0;
}

// Which devices one kernel's dynamic-LDS limit has been raised on.  A kernel that needs more than 64 KiB of dynamic LDS must have
// its limit raised first, and the limit belongs to the function ON ONE DEVICE: a process may use several, so an entry keeps one
// static record per kernel and asks it about the current device (eval_device.h: raise_lds_limit).  Two host threads that meet on a
// device both raise the limit to the same value; the record only spares the repeated call.  No HIP here: the record is also
// checked by a stand-alone program under the sanitizers (tests/host/lds_limit_main.cpp).
#pragma once
#include <atomic>

namespace egnn {

struct LdsLimitRecord {
  static constexpr int kDevices = 64;   // devices remembered; an index outside always answers "not yet" (raised at every call)
  std::atomic<bool> raised[kDevices];   // a static record starts all false

  bool known(int device) const { return device >= 0 && device < kDevices; }
  bool is_raised(int device) const { return known(device) && raised[device].load(std::memory_order_acquire); }
  void mark(int device) {
    if (known(device)) raised[device].store(true, std::memory_order_release);
  }
};

}  // namespace egnn

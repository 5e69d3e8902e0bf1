// Shortest-path ring statistics on the device: for every angle (p, q) of every requested centre, the size of the smallest ring
// through it and the number of shortest closing paths, on the bond graph of a cluster batch or on the infinite lattice of periodic
// cells.  Definitions: rings_math.h (shared with the host statement, rings_host.cpp).  An extension beyond the reference.
//
// Every output is an integer, a level is always completed before anything is decided, and a site's count is a saturating sum that
// does not depend on the order of its terms: the results do not depend on which slot a site lands in, on the order of a frontier
// list or on scheduling, so they are bitwise identical from run to run and equal to the host statement's.
//
// The kernel trusts no entry it reads: a centre is checked against N, a row against E, a neighbour against N, a shift against
// {-1, 0, 1}, an angle range against n_angles.
#include "eval_device.h"
#include "rings_host.h"
#include "rings_math.h"

namespace egnn {

constexpr int kRingThreads = 256;

// ---- one search per workgroup -----------------------------------------------------------------------------------------------------
// Workgroup (m, p) runs the search of centre m from row position p (rings_math.h); p >= degree - 1 has nothing to do.  The labels
// live in an LDS hash table (open addressing, linear probing) of `slots` = ring_slots(max_sites) entries: the 64-bit entry is the
// site key with the level in its top byte, so ONE compare-and-swap labels a site, and whoever wins it appends the slot to the
// next frontier list (the lists hold slot numbers, uint16).  A level is three phases between barriers:
//   discovery: thread t takes the frontier sites t, t + 256, ... and tries to label every neighbour site at this level;
//   counts:    thread t takes the NEW sites t, t + 256, ...; each pulls the counts of its neighbours labelled one level below
//              (a lookup per bond; nobody inserts in this phase) -- no atomic, saturation by ring_sat_add;
//   targets:   thread q looks target q up if it has no size yet.
// A search that would label more than max_sites sites raises s_over: every thread stops inserting at its next bond, so at most
// 256 further entries land in the table, which has at least max(2 max_sites, 512) slots and therefore never fills.
//
// Dynamic LDS: slots * 12 B (entries, counts) + 2 * max_sites * 2 B (frontier lists): 112 KiB at max_sites = 4096 -- one
// workgroup per CU (160 KiB); 14 KiB at max_sites = 512, where eight searches share a CU.
__device__ __forceinline__ bool ring_bond(const int* __restrict__ atom, const int* __restrict__ shift, int e, int N, uint64_t from,
                                          uint64_t* to) {
  const int v = atom[e];
  if (v < 0 || v >= N) return false;
  if (!shift) { *to = ring_step(from, v, nullptr); return true; }
  const int32_t s[3] = {shift[3 * (size_t)e], shift[3 * (size_t)e + 1], shift[3 * (size_t)e + 2]};
  if (!ring_shift_ok(s[0]) || !ring_shift_ok(s[1]) || !ring_shift_ok(s[2])) return false;
  *to = ring_step(from, v, s);
  return true;
}

__device__ __forceinline__ int ring_find(const unsigned long long* entries, uint32_t mask, uint64_t key) {
  uint32_t s = ring_hash(key) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe, s = (s + 1u) & mask) {
    const unsigned long long cur = entries[s];
    if (cur == kRingEmpty) return -1;
    if ((cur & kRingKeyMask) == key) return (int)s;
  }
  return -1;
}

__global__ __launch_bounds__(kRingThreads) void rings_kernel(int N, const int* __restrict__ row_ptr, int E, const int* __restrict__ atom,
                                                             const int* __restrict__ shift, const int* __restrict__ type, int A, int M,
                                                             const int* __restrict__ centre, const int* __restrict__ angle_ptr,
                                                             int n_angles, int max_size, int max_sites, int slots,
                                                             int* __restrict__ size, int* __restrict__ count, int* __restrict__ overflow,
                                                             int* __restrict__ hist) {
  extern __shared__ unsigned long long s_entry[];                        // [slots]
  int* s_count = reinterpret_cast<int*>(s_entry + slots);                // [slots]
  uint16_t* s_list0 = reinterpret_cast<uint16_t*>(s_count + slots);      // [max_sites]
  uint16_t* s_list1 = s_list0 + max_sites;                               // [max_sites]
  __shared__ int s_size[kRingMaxDegree], s_cnt[kRingMaxDegree], s_bins[kRingMaxSize + 1];
  __shared__ int s_next, s_left, s_over;
  const int tid = threadIdx.x, m = blockIdx.x, p = blockIdx.y;
  if (m >= M) return;
  const int c = centre[m];
  if (c < 0 || c >= N) return;
  const int r0 = row_ptr[c], d = row_ptr[c + 1] - r0, base = angle_ptr[m];
  if (r0 < 0 || d < 0 || r0 > E - d) return;                              // uniform in the workgroup, as every exit below
  const long long n_mine = (long long)d * (d - 1) / 2;
  if (base < 0 || n_mine > (long long)n_angles - base) return;
  if (d > kRingMaxDegree) {   // reported like an overflow; nothing is searched (workgroup p = 0 writes)
    if (p == 0) {
      for (long long a = tid; a < n_mine; a += kRingThreads) { size[base + a] = -1; count[base + a] = 0; }
      if (tid == 0) overflow[m] = 1;
    }
    return;
  }
  if (p + 1 >= d) return;
  const int off = base + ring_angle_first(p, d) - (p + 1);               // angle (p, q) is entry off + q
  const uint32_t mask = (uint32_t)slots - 1u;
  const uint64_t centre_key = ring_key(c, 0, 0, 0);

  for (int s = tid; s < slots; s += kRingThreads) s_entry[s] = kRingEmpty;
  if (tid < kRingMaxDegree) { s_size[tid] = 0; s_cnt[tid] = 0; }
  if (tid <= kRingMaxSize) s_bins[tid] = 0;
  if (tid == 0) { s_next = 0; s_left = d - 1 - p; s_over = 0; }
  __syncthreads();
  uint64_t source = centre_key;
  const bool has_source = ring_bond(atom, shift, r0 + p, N, centre_key, &source) && source != centre_key;
  if (has_source && tid == 0) {
    const uint32_t s = ring_hash(source) & mask;
    s_entry[s] = ring_entry(source, 0);
    s_count[s] = 1;
    s_list0[0] = (uint16_t)s;
  }
  // thread q owns target q
  uint64_t target = centre_key;
  const bool has_target = tid > p && tid < d && ring_bond(atom, shift, r0 + tid, N, centre_key, &target) && target != centre_key;
  __syncthreads();
  if (has_target) {
    const int s = ring_find(s_entry, mask, target);
    if (s >= 0) { s_size[tid] = 2; s_cnt[tid] = s_count[s]; atomicSub(&s_left, 1); }
  }
  __syncthreads();

  uint16_t* cur = s_list0;
  uint16_t* nxt = s_list1;
  int n_cur = has_source ? 1 : 0, labelled = n_cur;
  for (int level = 1; level <= max_size - 2 && n_cur > 0 && s_left > 0; ++level) {   // uniform: read between barriers
    // discovery
    for (int f = tid; f < n_cur; f += kRingThreads) {
      const uint64_t key = s_entry[cur[f]] & kRingKeyMask;
      const int a = ring_key_atom(key);
      const int b0 = row_ptr[a];
      int deg = row_ptr[a + 1] - b0;
      if (b0 < 0 || deg < 0 || b0 > E - deg) deg = 0;
      for (int k = 0; k < deg; ++k) {
        if (*(volatile int*)&s_over) break;
        uint64_t nb;
        if (!ring_bond(atom, shift, b0 + k, N, key, &nb) || nb == centre_key) continue;
        const unsigned long long mine = ring_entry(nb, level);
        uint32_t s = ring_hash(nb) & mask;
        bool placed = false;
        for (uint32_t probe = 0; probe <= mask && !placed; ++probe, s = (s + 1u) & mask) {
          unsigned long long seen = *(volatile unsigned long long*)&s_entry[s];
          if (seen == kRingEmpty) {
            seen = atomicCAS(&s_entry[s], (unsigned long long)kRingEmpty, mine);
            if (seen == kRingEmpty) {   // labelled by this thread
              const int at = atomicAdd(&s_next, 1);
              if (labelled + at + 1 > max_sites) *(volatile int*)&s_over = 1;
              else nxt[at] = (uint16_t)s;
              placed = true;
            }
          }
          if ((seen & kRingKeyMask) == nb) placed = true;   // labelled before, at this level or a lower one
        }
        if (!placed) *(volatile int*)&s_over = 1;           // a full table: cannot happen below max_sites labels
      }
    }
    __syncthreads();
    if (s_over) break;
    const int n_new = s_next;
    // counts, by pulling
    for (int f = tid; f < n_new; f += kRingThreads) {
      const int slot = nxt[f];
      const uint64_t key = s_entry[slot] & kRingKeyMask;
      const int a = ring_key_atom(key);
      const int b0 = row_ptr[a];
      int deg = row_ptr[a + 1] - b0;
      if (b0 < 0 || deg < 0 || b0 > E - deg) deg = 0;
      int sum = 0;
      for (int k = 0; k < deg; ++k) {
        uint64_t nb;
        if (!ring_bond(atom, shift, b0 + k, N, key, &nb) || nb == centre_key) continue;
        const int t = ring_find(s_entry, mask, nb);
        if (t >= 0 && ring_entry_level(s_entry[t]) == level - 1) sum = ring_sat_add(sum, s_count[t]);
      }
      s_count[slot] = sum;
    }
    __syncthreads();
    if (tid == 0) s_next = 0;
    if (has_target && s_size[tid] == 0) {
      const int s = ring_find(s_entry, mask, target);
      if (s >= 0) { s_size[tid] = level + 2; s_cnt[tid] = s_count[s]; atomicSub(&s_left, 1); }
    }
    __syncthreads();
    labelled += n_new;
    n_cur = n_new;
    uint16_t* t = cur; cur = nxt; nxt = t;
  }
  const bool over = s_over != 0;   // nobody writes s_over after the last barrier of the loop
  if (tid > p && tid < d) {
    size[off + tid] = over ? -1 : s_size[tid];
    count[off + tid] = over ? 0 : s_cnt[tid];
    if (!over && hist) atomicAdd(&s_bins[s_size[tid]], 1);
  }
  if (over && tid == 0) overflow[m] = 1;   // every overflowed search of the centre stores the same value
  if (over || !hist) return;
  __syncthreads();
  const int tc = type[c];
  if (tid <= max_size && tc >= 0 && tc < A && s_bins[tid]) atomicAdd(&hist[(size_t)tc * (max_size + 1) + tid], s_bins[tid]);
}

}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_rings(void* stream, int N, const int32_t* d_row_ptr, int E, const int32_t* d_atom, const int32_t* d_shift, const int32_t* d_type,
               int A, int M, const int32_t* d_centre, const int32_t* d_angle_ptr, int n_angles, int max_size, int max_sites, int32_t* d_size,
               int32_t* d_count, int32_t* d_overflow, int32_t* d_hist, const int32_t* row_ptr, const int32_t* atom, const int32_t* shift,
               const int32_t* centre) {
  const char* who = "egnn_rings";
  if (int rc = rings_common_check(who, N, d_row_ptr, E, d_atom, d_type, A, M, d_centre, d_angle_ptr, n_angles, max_size, max_sites, d_size,
                                  d_count, d_overflow))
    return rc;
  if (int rc = rings_lists_check(who, N, row_ptr, E, atom, shift, M, centre)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int slots = ring_slots(max_sites);
  const size_t lds = (size_t)slots * (sizeof(uint64_t) + sizeof(int32_t)) + 2 * (size_t)max_sites * sizeof(uint16_t);
  // up to 112 KiB beside 0.5 KiB of static LDS; a CU has 160 KiB
  static LdsLimitRecord raised;
  if (int rc = raise_lds_limit(raised, &rings_kernel, (size_t)ring_slots(kRingMaxSites) * 12 + 4 * (size_t)kRingMaxSites)) return rc;
  if (M > 0) EGNN_HIP(hipMemsetAsync(d_overflow, 0, sizeof(int32_t) * (size_t)M, st));
  if (n_angles > 0) {   // a centre the kernel refuses (outside N, a row outside E) leaves zeros
    EGNN_HIP(hipMemsetAsync(d_size, 0, sizeof(int32_t) * (size_t)n_angles, st));
    EGNN_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t) * (size_t)n_angles, st));
  }
  if (d_hist) EGNN_HIP(hipMemsetAsync(d_hist, 0, sizeof(int32_t) * (size_t)A * (max_size + 1), st));
  if (M > 0)
    hipLaunchKernelGGL(rings_kernel, dim3(M, kRingMaxDegree - 1), dim3(kRingThreads), lds, st, N, d_row_ptr, E, d_atom, d_shift, d_type, A, M,
                       d_centre, d_angle_ptr, n_angles, max_size, max_sites, slots, d_size, d_count, d_overflow, d_hist);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // extern "C"

// Host side of the ring statistics: the argument checks of the device entry (rings.hip) and the host statement egnn_rings_host --
// one level-by-level search per (centre, row position) on the CPU through rings_math.h, the text the kernel compiles.  No HIP
// call, no device code: checked (and run under the sanitizers) on a machine without a GPU.
#include <string.h>

#include <vector>

#include "rings_host.h"
#include "rings_math.h"

namespace egnn {

int rings_common_check(const char* who, int N, const void* row_ptr, int E, const void* atom, const void* type, int A, int M,
                       const void* centre, const void* angle_ptr, int n_angles, int max_size, int max_sites, const void* size,
                       const void* count, const void* overflow) {
  if (max_size < kRingMinSize || max_size > kRingMaxSize) {
    set_error("%s: max_size %d (%d <= max_size <= %d)", who, max_size, kRingMinSize, kRingMaxSize);
    return EGNN_EINVAL;
  }
  if (max_sites < 1 || max_sites > kRingMaxSites) {
    set_error("%s: max_sites %d (1 <= max_sites <= %d)", who, max_sites, kRingMaxSites);
    return EGNN_EINVAL;
  }
  if (N < 1 || E < 0 || A < 1 || M < 0 || n_angles < 0) {
    set_error("bad %s arguments (N >= 1, E >= 0, A >= 1, M >= 0, n_angles >= 0)", who);
    return EGNN_EINVAL;
  }
  if (!row_ptr || !type || !angle_ptr || !size || !count || !overflow || (E > 0 && !atom) || (M > 0 && !centre)) {
    set_error("bad %s arguments (row_ptr, atom, type, centre, angle_ptr, size, count and overflow given)", who);
    return EGNN_EINVAL;
  }
  return EGNN_OK;
}

int rings_lists_check(const char* who, int N, const int32_t* row_ptr, int E, const int32_t* atom, const int32_t* shift, int M,
                      const int32_t* centre) {
  if (centre)
    for (int m = 0; m < M; ++m)
      if (centre[m] < 0 || centre[m] >= N) {
        set_error("%s: centre %d names atom %d outside the %d atoms", who, m, centre[m], N);
        return EGNN_EINVAL;
      }
  if (row_ptr) {
    bool ok = row_ptr[0] == 0 && row_ptr[N] == E;
    for (int i = 0; i < N && ok; ++i) ok = row_ptr[i + 1] >= row_ptr[i];
    if (!ok) { set_error("%s: row_ptr must start at 0, not decrease and end at E = %d (a non-monotone row_ptr)", who, E); return EGNN_EINVAL; }
  }
  if (atom)
    for (int e = 0; e < E; ++e)
      if (atom[e] < 0 || atom[e] >= N) { set_error("%s: bond %d names neighbour %d outside [0, %d)", who, e, atom[e], N); return EGNN_EINVAL; }
  if (shift)
    for (int e = 0; e < E; ++e)
      if (!ring_shift_ok(shift[3 * (size_t)e]) || !ring_shift_ok(shift[3 * (size_t)e + 1]) || !ring_shift_ok(shift[3 * (size_t)e + 2])) {
        set_error("%s: bond %d has a shift component outside {-1, 0, 1}", who, e);
        return EGNN_EINVAL;
      }
  return EGNN_OK;
}

namespace {

// the labels of one search: open addressing over the entries of rings_math.h, cleared slot by slot after the search
struct RingTable {
  std::vector<uint64_t> entry;
  std::vector<int32_t> count;
  std::vector<int> used;
  uint32_t mask;
  explicit RingTable(int slots) : entry(slots, kRingEmpty), count(slots, 0), mask((uint32_t)slots - 1u) { used.reserve(slots); }
  int find(uint64_t key) const {
    for (uint32_t s = ring_hash(key) & mask;; s = (s + 1u) & mask) {
      if (entry[s] == kRingEmpty) return -1;
      if ((entry[s] & kRingKeyMask) == key) return (int)s;
    }
  }
  int insert(uint64_t key, int level) {   // the key is not in the table
    uint32_t s = ring_hash(key) & mask;
    while (entry[s] != kRingEmpty) s = (s + 1u) & mask;
    entry[s] = ring_entry(key, level);
    used.push_back((int)s);
    return (int)s;
  }
  void clear() {
    for (int s : used) entry[s] = kRingEmpty;
    used.clear();
  }
};

}  // namespace
}  // namespace egnn

using namespace egnn;

extern "C" {

int egnn_rings_host(int N, const int32_t* row_ptr, int E, const int32_t* atom, const int32_t* shift, const int32_t* type, int A, int M,
                    const int32_t* centre, const int32_t* angle_ptr, int n_angles, int max_size, int max_sites, int32_t* size,
                    int32_t* count, int32_t* overflow, int32_t* hist) {
  const char* who = "egnn_rings_host";
  if (int rc = rings_common_check(who, N, row_ptr, E, atom, type, A, M, centre, angle_ptr, n_angles, max_size, max_sites, size, count, overflow))
    return rc;
  if (int rc = rings_lists_check(who, N, row_ptr, E, atom, shift, M, centre)) return rc;
  for (int i = 0; i < N; ++i)
    if (type[i] < 0 || type[i] >= A) { set_error("%s: atom %d has type %d outside [0, %d)", who, i, type[i], A); return EGNN_EINVAL; }
  if (angle_ptr[0] != 0 || angle_ptr[M] != n_angles) { set_error("%s: angle_ptr must run from 0 to n_angles = %d", who, n_angles); return EGNN_EINVAL; }
  for (int m = 0; m < M; ++m) {
    const int64_t d = row_ptr[centre[m] + 1] - row_ptr[centre[m]];
    if ((int64_t)angle_ptr[m + 1] - angle_ptr[m] != d * (d - 1) / 2) {
      set_error("%s: angle_ptr gives centre %d (degree %lld) %lld angles", who, m, (long long)d, (long long)angle_ptr[m + 1] - angle_ptr[m]);
      return EGNN_EINVAL;
    }
  }

  const int bins = max_size + 1;
  if (hist) memset(hist, 0, sizeof(int32_t) * (size_t)A * bins);
  RingTable table(ring_slots(max_sites));
  std::vector<int> frontier, next;
  for (int m = 0; m < M; ++m) {
    const int c = centre[m], r0 = row_ptr[c], d = row_ptr[c + 1] - r0, base = angle_ptr[m];
    overflow[m] = 0;
    if (d > kRingMaxDegree) {
      for (int a = base; a < angle_ptr[m + 1]; ++a) { size[a] = -1; count[a] = 0; }
      overflow[m] = 1;
      continue;
    }
    const uint64_t centre_key = ring_key(c, 0, 0, 0);
    for (int p = 0; p + 1 < d; ++p) {
      const int off = base + ring_angle_first(p, d) - (p + 1);   // angle (p, q) is entry off + q
      for (int q = p + 1; q < d; ++q) { size[off + q] = 0; count[off + q] = 0; }
      const uint64_t source = ring_step(centre_key, atom[r0 + p], shift ? shift + 3 * (size_t)(r0 + p) : nullptr);
      int labelled = 0, left = d - 1 - p;
      bool over = false;
      frontier.clear();
      if (source != centre_key) {
        const int s = table.insert(source, 0);
        table.count[s] = 1;
        frontier.push_back(s);
        labelled = 1;
        over = labelled > max_sites;
      }
      auto settle = [&](int level) {   // targets labelled at this level
        for (int q = p + 1; q < d; ++q) {
          if (size[off + q]) continue;
          const uint64_t target = ring_step(centre_key, atom[r0 + q], shift ? shift + 3 * (size_t)(r0 + q) : nullptr);
          const int s = target == centre_key ? -1 : table.find(target);
          if (s < 0) continue;
          size[off + q] = level + 2;
          count[off + q] = table.count[s];
          --left;
        }
      };
      if (!over) settle(0);
      for (int level = 1; level <= max_size - 2 && left > 0 && !frontier.empty() && !over; ++level) {
        next.clear();
        for (int f : frontier) {   // discovery
          const uint64_t key = table.entry[f] & kRingKeyMask;
          const int a = ring_key_atom(key);
          for (int e = row_ptr[a]; e < row_ptr[a + 1]; ++e) {
            const uint64_t nb = ring_step(key, atom[e], shift ? shift + 3 * (size_t)e : nullptr);
            if (nb == centre_key || table.find(nb) >= 0) continue;
            next.push_back(table.insert(nb, level));
            if (labelled + (int)next.size() > max_sites) over = true;   // the table holds 2 max_sites: stop before it fills
            if (over) break;
          }
          if (over) break;
        }
        if (over) break;
        labelled += (int)next.size();
        for (int s : next) {   // counts, by pulling
          const uint64_t key = table.entry[s] & kRingKeyMask;
          const int a = ring_key_atom(key);
          int sum = 0;
          for (int e = row_ptr[a]; e < row_ptr[a + 1]; ++e) {
            const uint64_t nb = ring_step(key, atom[e], shift ? shift + 3 * (size_t)e : nullptr);
            const int t = nb == centre_key ? -1 : table.find(nb);
            if (t >= 0 && ring_entry_level(table.entry[t]) == level - 1) sum = ring_sat_add(sum, table.count[t]);
          }
          table.count[s] = sum;
        }
        settle(level);
        frontier.swap(next);
      }
      table.clear();
      if (over) {
        for (int q = p + 1; q < d; ++q) { size[off + q] = -1; count[off + q] = 0; }
        overflow[m] = 1;
      } else if (hist) {
        for (int q = p + 1; q < d; ++q) ++hist[(size_t)type[c] * bins + size[off + q]];
      }
    }
  }
  return EGNN_OK;
}

}  // extern "C"

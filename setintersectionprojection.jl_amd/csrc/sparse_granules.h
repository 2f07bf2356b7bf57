// Which 2 MiB granules of a sparse array are backed by memory (DeviceMemory::alloc_sparse, device_memory.h).
// (tests/test_device_memory_cpu.py compares it with a restatement by granule index, on the CPU.)
// No HIP header: this file compiles with a plain host compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace sipx {

constexpr size_t SPARSE_GRAN = 2ull << 20;      // the native large page

inline size_t sparse_round_up(size_t bytes) { return (bytes + SPARSE_GRAN - 1) / SPARSE_GRAN * SPARSE_GRAN; }

// ranges: [first, last) in BYTES of the array's address space.  Each one that holds a byte is widened to whole granules and
// clipped to the rounded total; what comes back is sorted, and ranges that overlap or touch are one.
inline std::vector<std::pair<size_t, size_t>> sparse_granule_ranges(size_t total_bytes, std::vector<std::pair<size_t, size_t>> ranges) {
  const size_t total = sparse_round_up(total_bytes);
  for (auto& r : ranges) {
    if (r.second <= r.first) { r = {0, 0}; continue; }      // (empty: no granule, wherever it lies)
    r.first = r.first / SPARSE_GRAN * SPARSE_GRAN;
    r.second = std::min(total, sparse_round_up(r.second));
  }
  std::sort(ranges.begin(), ranges.end());
  std::vector<std::pair<size_t, size_t>> merged;
  for (const auto& r : ranges) {
    if (r.second <= r.first) continue;
    if (!merged.empty() && r.first <= merged.back().second) merged.back().second = std::max(merged.back().second, r.second);
    else merged.push_back(r);
  }
  return merged;
}

}  // namespace sipx

// Runs sparse_granule_ranges (csrc/sparse_granules.h) on cases read from stdin, one answer line per case
// (tests/test_device_memory_cpu.py compares the lines with a restatement by granule index).
// A case is a line of integers: total_bytes n first_1 last_1 ... first_n last_n  -> the merged ranges, "first last" pairs in bytes
#include <cstdio>
#include <iostream>
#include <utility>
#include <vector>

#include "sparse_granules.h"

int main() {
  unsigned long long total = 0;
  while (std::cin >> total) {
    size_t n = 0;
    std::cin >> n;
    std::vector<std::pair<size_t, size_t>> ranges(n);
    for (auto& r : ranges) {
      unsigned long long a = 0, b = 0;
      std::cin >> a >> b;
      r = {(size_t)a, (size_t)b};
    }
    const auto merged = sipx::sparse_granule_ranges((size_t)total, ranges);
    std::printf("%zu", merged.size());
    for (const auto& r : merged) std::printf(" %zu %zu", r.first, r.second);
    std::printf("\n");
  }
  return 0;
}

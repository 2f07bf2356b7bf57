// Touching the pages of a host destination before a large device-to-host copy (sipx_download).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

#include "env_knobs.h"

namespace sipx {

// A device-to-host copy into memory the caller has just allocated spends most of its time in page faults (one per 4 KiB, taken
// one after the other by the copy's staging thread: 1 GiB arrives in 68 ms, in 20 ms once the pages exist -- round 5).  The
// destination of a large download is therefore touched first, by several threads at once: one write per page makes the kernel
// map it, and the copy that follows overwrites every byte.  (A destination that already has its pages loses a few hundred
// microseconds per GiB to this.)
inline void host_prefault(void* p, size_t bytes) {
  constexpr size_t PAGE = 4096, MIN_BYTES = 8u << 20;
  int nthreads = env_knobs().prefault_threads;                      // SIPX_PREFAULT_THREADS (0: off)
  if (nthreads < 0) {
    const unsigned hc = std::thread::hardware_concurrency();
    nthreads = (int)std::min<unsigned>(16u, hc > 1 ? hc / 2 : 1u);      // (9 GiB: 0.64 s without, 0.34 / 0.27 s with 4 / 16 threads)
  }
  if (!p || bytes < MIN_BYTES || nthreads < 1) return;
  char* base = static_cast<char*>(p);
  const size_t first = (PAGE - (reinterpret_cast<uintptr_t>(base) & (PAGE - 1))) & (PAGE - 1);      // first page boundary inside
  if (first >= bytes) return;
  const size_t npages = (bytes - first + PAGE - 1) / PAGE;
  auto touch = [base, first, npages, bytes](size_t a, size_t b) {
    for (size_t k = a; k < b && k < npages; ++k) {
      volatile char* q = base + first + k * PAGE;
      if ((size_t)(q - base) < bytes) *q = 0;
    }
  };
  std::vector<std::thread> th;
  const size_t per = (npages + (size_t)nthreads - 1) / (size_t)nthreads;
  for (int t = 1; t < nthreads; ++t) th.emplace_back(touch, (size_t)t * per, (size_t)(t + 1) * per);
  base[0] = 0;
  touch(0, per);
  for (auto& t : th) t.join();
}

}  // namespace sipx

// DeviceMemory (device_memory.h): the only unit of csrc/ that allocates or frees device memory.
#include "device_memory.h"

#include <algorithm>
#include <cstdio>

#include "sipx_common.h"
#include "sparse_granules.h"

namespace sipx {

DeviceMemory::~DeviceMemory() {
  for (auto b = blocks_.rbegin(); b != blocks_.rend(); ++b) free_block(*b);
}

void* DeviceMemory::alloc_bytes(size_t bytes, Mem kind, bool on_stream, hipStream_t stream) {
  void* p = nullptr;
  if (bytes == 0) return p;
  SIPX_HIP(hipMalloc(&p, bytes));
  blocks_.emplace_back();
  Block& b = blocks_.back();
  b.p = p;
  b.bytes = bytes;
  b.state = kind == Mem::State;
  bytes_ += (long long)bytes;
  if (kind == Mem::NoFill) return p;
  if (on_stream) {
    // (a projector fills on its own stream: a fill on the null stream is not ordered against a non-blocking stream -- the
    //  initialisation kernel of the search state that follows would race with it, and a rank whose state came out all zero takes
    //  other decisions than the ranks it shares every collective with)
    SIPX_HIP(hipMemsetAsync(p, 0, bytes, stream));
  } else {
    // hipMemset is queued on the NULL stream; the engine stream is non-blocking, so wait here or the
    // zero-fill may land after kernels of the engine stream have already written the buffer.
    SIPX_HIP(hipMemset(p, 0, bytes));
    SIPX_HIP(hipStreamSynchronize(nullptr));
  }
  return p;
}

void* DeviceMemory::alloc_sparse(size_t total_bytes, const std::vector<std::pair<size_t, size_t>>& ranges, int device, Mem kind) {
  const size_t total = sparse_round_up(total_bytes);
  const std::vector<std::pair<size_t, size_t>> merged = sparse_granule_ranges(total_bytes, ranges);
  void* base = nullptr;
  SIPX_HIP(hipMemAddressReserve(&base, total, SPARSE_GRAN, nullptr, 0));
  blocks_.emplace_back();
  Block& blk = blocks_.back();      // (in the table from here on: a failure below leaves the granules mapped so far to the destructor)
  blk.p = base;
  blk.sparse = true;
  blk.state = kind == Mem::State;
  blk.reserved = total;
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = device;
  hipMemAccessDesc acc = {};
  acc.location.type = hipMemLocationTypeDevice;
  acc.location.id = device;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  // Every mapping of a reservation has the SAME size, one granule: hipMemSetAccess of this runtime (ROCm 7.2) answers "invalid
  // argument" for a mapping whose size differs from the others inside one reservation (4 + 4 + 2 MiB fails at the third,
  // 2 + 4 at the second; uniform sizes are fine).  2 MiB is the native large page.
  for (const auto& r : merged) {
    for (size_t off = r.first; off < r.second; off += SPARSE_GRAN) {
      const size_t len = SPARSE_GRAN;
      auto chk = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return;
        char msg[256];
        std::snprintf(msg, sizeof msg, "sparse array: %s failed (%s): reservation %zu bytes at %p, granule at %zu of range [%zu, %zu)", what,
                      hipGetErrorString(e), total, base, off, r.first, r.second);
        throw std::runtime_error(msg);
      };
      hipMemGenericAllocationHandle_t h;
      chk(hipMemCreate(&h, len, &prop, 0), "hipMemCreate");
      if (hipError_t e = hipMemMap((char*)base + off, len, 0, h, 0); e != hipSuccess) {
        (void)hipMemRelease(h);
        chk(e, "hipMemMap");
      }
      blk.offsets.push_back(off);
      blk.handles.push_back(h);
      blk.bytes += len;
      bytes_ += (long long)len;
      chk(hipMemSetAccess((char*)base + off, len, &acc, 1), "hipMemSetAccess");
    }
    if (kind != Mem::NoFill) SIPX_HIP(hipMemset((char*)base + r.first, 0, r.second - r.first));
  }
  SIPX_HIP(hipStreamSynchronize(nullptr));
  return base;
}

void DeviceMemory::zero_block(const Block& b, hipStream_t stream) {
  if (!b.sparse) {
    SIPX_HIP(hipMemsetAsync(b.p, 0, b.bytes, stream));
    return;
  }
  for (size_t off : b.offsets) SIPX_HIP(hipMemsetAsync((char*)b.p + off, 0, SPARSE_GRAN, stream));
}

void DeviceMemory::free_block(const Block& b) {
  if (!b.sparse) {
    (void)hipFree(b.p);
    return;
  }
  for (size_t k = 0; k < b.offsets.size(); ++k) {
    (void)hipMemUnmap((char*)b.p + b.offsets[k], SPARSE_GRAN);
    (void)hipMemRelease(b.handles[k]);
  }
  (void)hipMemAddressFree(b.p, b.reserved);
}

std::vector<DeviceMemory::Block>::iterator DeviceMemory::find(void* p, const char* what) {
  auto it = std::find_if(blocks_.begin(), blocks_.end(), [p](const Block& b) { return b.p == p; });
  if (it == blocks_.end()) throw std::runtime_error(std::string("internal: ") + what + " of an allocation this owner did not make");
  return it;
}

void DeviceMemory::zero_state(hipStream_t stream) {
  for (const Block& b : blocks_)
    if (b.state) zero_block(b, stream);
}

void DeviceMemory::zero(void* p, hipStream_t stream) {
  if (p) zero_block(*find(p, "zero-fill"), stream);
}

void DeviceMemory::release(void* p) {
  if (!p) return;
  auto it = find(p, "release");
  bytes_ -= (long long)it->bytes;
  free_block(*it);
  blocks_.erase(it);
}

}  // namespace sipx

// Device memory, one owner per context: DeviceMemory hands out device arrays, remembers every one of them and frees them in
// its destructor, the latest first.  The engine keeps one for everything a context holds, a projector one for its own buffers, and a function that
// needs temporaries a local one -- so a throw frees them.  Allocate, zero-fill of the state (sipx_reset), byte count and free
// all walk this one table; nothing else in csrc/ calls hipMalloc, hipFree or the virtual-memory functions.
// No mutex and no global: an owner is used by one thread at a time.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>
#include <vector>

namespace sipx {

enum class Mem {
  NoFill,      // whatever the allocator returns
  Zeroed,      // zero-filled before alloc returns
  State        // zero-filled, and again by every zero_state(): what a solve leaves behind in it must not reach the next one
};

class DeviceMemory {
 public:
  DeviceMemory() = default;
  DeviceMemory(const DeviceMemory&) = delete;
  DeviceMemory& operator=(const DeviceMemory&) = delete;
  ~DeviceMemory();

  // count elements (nullptr for none)
  template <typename T>
  T* alloc(size_t count, Mem kind = Mem::Zeroed) { return static_cast<T*>(alloc_bytes(count * sizeof(T), kind, false, nullptr)); }
  // ... zero-filled on `stream` instead of the null stream, without waiting for it
  template <typename T>
  T* alloc_zeroed_on(size_t count, hipStream_t stream) { return static_cast<T*>(alloc_bytes(count * sizeof(T), Mem::Zeroed, true, stream)); }

  // SPARSE arrays (slab-decomposed contexts): the array keeps its GLOBAL index space -- the whole range is reserved in the
  // virtual address space, so every kernel indexes it exactly as before -- but only the element ranges a rank touches (its planes,
  // the halo planes around them) are backed by memory (hipMemAddressReserve / hipMemCreate / hipMemMap, 2 MiB granules).  A rank of
  // eight then holds an eighth of every N-vector (plus three planes) instead of all of it: the decomposition grows the problem that
  // fits, not only its speed.  An access outside the mapped ranges faults instead of reading stale data.
  // ranges: [first, last) in BYTES of the array's address space (sparse_granules.h); returns the base of the reservation,
  // zero-filled where mapped
  void* alloc_sparse(size_t total_bytes, const std::vector<std::pair<size_t, size_t>>& ranges, int device, Mem kind = Mem::Zeroed);

  void zero_state(hipStream_t stream);         // queues the zero-fill of every Mem::State allocation (a sparse one: its mapped granules)
  void zero(void* p, hipStream_t stream);      // ... of this one, whatever its kind
  void release(void* p);                       // frees one allocation ahead of the owner (nullptr: nothing)
  long long bytes() const { return bytes_; }   // live bytes (a sparse array counts its mapped granules)

 private:
  struct Block {
    void* p = nullptr;
    size_t bytes = 0;                                          // plain: of the allocation; sparse: of the mapped granules
    bool state = false, sparse = false;
    size_t reserved = 0;                                       // sparse: bytes of the reservation
    std::vector<size_t> offsets;                               // sparse: byte offset of every mapped granule ...
    std::vector<hipMemGenericAllocationHandle_t> handles;      // ... and its memory
  };
  void* alloc_bytes(size_t bytes, Mem kind, bool on_stream, hipStream_t stream);
  static void zero_block(const Block& b, hipStream_t stream);
  static void free_block(const Block& b);
  std::vector<Block>::iterator find(void* p, const char* what);
  std::vector<Block> blocks_;      // in the order of allocation (a context holds a few dozen)
  long long bytes_ = 0;
};

}  // namespace sipx

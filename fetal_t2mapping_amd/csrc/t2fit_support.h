// t2fit_support.h -- host-side support every translation unit of libt2fit_hip.so shares: the workgroup size, the small
// size / alignment helpers and the cache of device scratch buffers.  (Device-side reductions and float keys are NOT
// shared: each unit's summation order and bit patterns are pinned by its own bit-identity tests.)
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

namespace t2fit {

constexpr int kBlock = 256;  // lanes of a workgroup, every kernel of the library unless it says otherwise

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
template <class T> constexpr T ceil_div(T a, T b) { return (a + b - 1) / b; }

// Scratch kept between calls: one device buffer per (device, stream, use), grown on demand.  Launches on one stream run
// one after the other, so they may share a buffer; launches on different streams may overlap and must not (kernels keep
// live state in it).  t2fit_destroy gives back the buffers of its context's streams (scratch_release_stream); buffers of
// caller-owned streams live as long as the process.
enum ScratchUse : int {
  kScratchRing,      // fit: global part of the correction-pair ring (one-wave-workgroup kernels, Rician likelihood)
  kScratchRoiErode,  // ROI statistics: the erosion's second buffer
  kScratchRoiStats,  // ROI statistics: the sort's tables and segments
  kScratchComponents,  // component selection table: the best key, the counts of the kept per chunk
};
struct ScratchCache {
  struct Entry { int device; hipStream_t stream; int use; void* p; size_t bytes; };
  std::mutex mutex;
  std::vector<Entry> entries;
  static ScratchCache& get() { static ScratchCache c; return c; }
};

template <class T> hipError_t scratch_get(hipStream_t st, ScratchUse use, size_t bytes, T** out) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  ScratchCache& cache = ScratchCache::get();
  std::lock_guard<std::mutex> g(cache.mutex);
  ScratchCache::Entry* r = nullptr;
  for (ScratchCache::Entry& c : cache.entries)
    if (c.device == dev && c.stream == st && c.use == use) r = &c;
  if (!r) {
    cache.entries.push_back(ScratchCache::Entry{dev, st, use, nullptr, 0});
    r = &cache.entries.back();
  }
  if (r->bytes < bytes) {
    if (r->p) {  // (a kernel queued earlier on this stream may still be using it)
      if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
      (void)hipFree(r->p);
      r->p = nullptr;
      r->bytes = 0;
    }
    if ((e = hipMalloc(&r->p, bytes)) != hipSuccess) return e;
    r->bytes = bytes;
  }
  *out = static_cast<T*>(r->p);
  return hipSuccess;
}

// the stream is about to be destroyed (and has been synchronised): every use cached for it goes
inline void scratch_release_stream(int device, hipStream_t st) {
  ScratchCache& cache = ScratchCache::get();
  std::lock_guard<std::mutex> g(cache.mutex);
  for (size_t i = cache.entries.size(); i-- > 0;)
    if (cache.entries[i].device == device && cache.entries[i].stream == st) {
      if (cache.entries[i].p) (void)hipFree(cache.entries[i].p);
      cache.entries.erase(cache.entries.begin() + i);
    }
}

}  // namespace t2fit

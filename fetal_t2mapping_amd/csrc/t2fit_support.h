// t2fit_support.h -- host-side support every translation unit of libt2fit_hip.so shares: the workgroup size, the small
// size / alignment helpers, the workspace check and the cache of device scratch buffers; and two device one-liners.
//
// Device code is shared where several units ran the same text, and only there; every unit is compiled by one command with
// one set of flags and without relocatable device code, so a function moved into a header compiles to what it did:
//   t2fit_affine.h   the coordinate rules, the metric's sample and the resampling sample (register, resample, ffd)
//   t2fit_mattes.h   the Parzen window, the bin of a voxel, the histogram deposit, the uint64 zero kernel (register, ffd, n4)
//   t2fit_reduce.h   the 256-fan tree over rows of partials: kernel, plan, launches (register, n4, seg)
//   here             the wave butterfly and the finite test (register, ffd, n4, seg, sr_robust)
//   t2fit_bspline.h  the node and weights of a voxel index, the selected tap of a row kernel (n4, ffd)
// Reductions and float keys whose text differs are deliberately NOT shared: each one's summation order and bit patterns
// are pinned by its own unit's bit-identity tests, and merging two would change one of them.  These are t2fit_denoise.hip's
// wave_sum, t2fit_roi.hip's block tree and float keys, t2fit_boot.hip's keys and the two 1024-lane scans.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "t2fit_error.h"

namespace t2fit {

constexpr int kBlock = 256;  // lanes of a workgroup, every kernel of the library unless it says otherwise

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }  // a: a power of two
constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
template <class T> constexpr T ceil_div(T a, T b) { return (a + b - 1) / b; }

// the workspace of the entry point `who`: there, aligned to 256 bytes and at least `need` bytes, the figure bytes_fn reports
inline int check_workspace(const std::string& who, const void* ws, size_t bytes, size_t need, const char* bytes_fn) {
  if (!ws) return fail(T2FIT_E_INVALID, who + ": workspace_dev is NULL");
  if (misaligned(ws, 256)) return fail(T2FIT_E_INVALID, who + ": workspace_dev is not aligned to 256 bytes");
  if (bytes < need)
    return fail(T2FIT_E_INVALID, who + ": workspace too small: " + std::to_string(bytes) + " bytes given, " + std::to_string(need) + " needed (" +
                                     bytes_fn + ")");
  return T2FIT_OK;
}

// ---- device: the two one-liners of the float64 sums (register, ffd, n4, seg, sr_robust)
// every lane ends with the halving tree of the wave's 64 values
__device__ inline double wave_butterfly(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
  return v;
}

__device__ inline bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

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

// t2fit_masks.hip -- gfx950 kernels and C ABI of the two side features around a fit (include/t2fit.h): the union of the
// stacks' masks with its ordered flat indices (t2fit_union_mask_dev) and the per-label statistics of a map over the
// phantom's vials (t2fit_label_stats_dev).  Streaming kernels, grid = ceil(N / tile) >> 256 CUs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "t2fit_error.h"
#include "t2fit_support.h"

namespace {

using t2fit::fail;
using t2fit::kBlock;

// ---- union mask + ordered flat indices (run_t2mapping.py:383-384,412,421) ----------------------
constexpr int kScanItems = 4;                      // voxels per lane
constexpr int kScanTile = kBlock * kScanItems;     // voxels per workgroup

__device__ __forceinline__ uint8_t union_at(const uint8_t* __restrict__ masks, int n_masks, int64_t n_vox, int64_t v) {
  uint8_t any = 0;
  for (int j = 0; j < n_masks; ++j) any |= masks[(int64_t)j * n_vox + v] != 0;
  return any;
}

__global__ __launch_bounds__(kBlock) void mask_count_kernel(const uint8_t* __restrict__ masks, int n_masks,
                                                            int64_t n_vox, uint8_t* __restrict__ mask_out,
                                                            int64_t* __restrict__ tile_counts) {
  __shared__ int wave_sum[kBlock / 64];
  const int64_t v0 = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  int cnt = 0;
  for (int q = 0; q < kScanItems; ++q) {
    const int64_t v = v0 + q;
    if (v < n_vox) {
      const uint8_t u = union_at(masks, n_masks, n_vox, v);
      mask_out[v] = u;
      cnt += u;
    }
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < kBlock / 64; ++w) s += wave_sum[w];
    tile_counts[blockIdx.x] = s;
  }
}

// exclusive scan of the per-tile counts by one workgroup (tiles <= N/1024: tens of thousands)
__global__ __launch_bounds__(1024) void tile_scan_kernel(int64_t* tile_counts, int64_t n_tiles, int64_t* total_out) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (n_tiles + 1023) / 1024;
  const int64_t lo = (int64_t)t * per;
  const int64_t hi = lo + per < n_tiles ? lo + per : n_tiles;
  int64_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += tile_counts[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
    int64_t add = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int64_t run = t == 0 ? 0 : part[t - 1];
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t c = tile_counts[i];
    tile_counts[i] = run;
    run += c;
  }
  if (t == 1023) *total_out = part[1023];
}

__global__ __launch_bounds__(kBlock) void mask_write_kernel(const uint8_t* __restrict__ mask, int64_t n_vox,
                                                            const int64_t* __restrict__ tile_offsets,
                                                            int64_t* __restrict__ idx_out) {
  __shared__ int wave_sum[kBlock / 64];
  const int64_t v0 = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint8_t f[kScanItems];
  int cnt = 0;
  for (int q = 0; q < kScanItems; ++q) {
    const int64_t v = v0 + q;
    f[q] = v < n_vox ? mask[v] : 0;
    cnt += f[q];
  }
  // exclusive prefix of cnt within the wave, then across the 4 waves
  int incl = cnt;
  const int l = threadIdx.x & 63;
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off, 64);
    if (l >= off) incl += up;
  }
  if (l == 63) wave_sum[threadIdx.x >> 6] = incl;
  __syncthreads();
  int wave_off = 0;
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) wave_off += wave_sum[w];
  int64_t pos = tile_offsets[blockIdx.x] + wave_off + (incl - cnt);
  for (int q = 0; q < kScanItems; ++q)
    if (f[q]) idx_out[pos++] = v0 + q;
}

// ---- per-label statistics of a map (utils/t2map_utils.py:43-53: nanmean / nanstd per vial) -------
// Two rounds, numpy's own algorithm: mean first, then the mean of squared deviations from it (a
// constant region gives exactly 0).  Deterministic: each thread tallies its strided share of the
// workgroup's contiguous span into its own LDS column (one slot per label), columns are combined by a
// fixed tree, and the per-workgroup partials are added in workgroup order by one thread per label.
constexpr int kMaxLabels = 32;  // 2 * 32 * 256 doubles of LDS = 128 KiB (the NIST phantom has 14 vials)

template <bool kSecond>
__global__ __launch_bounds__(kBlock) void label_partial_kernel(const float* __restrict__ map,
                                                               const int32_t* __restrict__ label, int64_t n_vox,
                                                               int n_labels, int64_t span, const double* __restrict__ mean,
                                                               double* __restrict__ part_sum, int64_t* __restrict__ part_cnt) {
  extern __shared__ double acc[];  // [n_labels][kBlock] sums, then [n_labels][kBlock] counts (as double)
  double* cnt = acc + (size_t)n_labels * kBlock;
  const int tid = threadIdx.x;
  for (int l = 0; l < n_labels; ++l) { acc[l * kBlock + tid] = 0.0; cnt[l * kBlock + tid] = 0.0; }
  const int64_t lo = (int64_t)blockIdx.x * span;
  const int64_t hi = lo + span < n_vox ? lo + span : n_vox;
  for (int64_t v = lo + tid; v < hi; v += kBlock) {
    const int32_t l = label[v] - 1;
    const float x = map[v];
    if (l >= 0 && l < n_labels && x == x) {  // NaN values are skipped, as nanmean / nanstd do
      double t = (double)x;
      if (kSecond) { t -= mean[l]; t *= t; }
      acc[l * kBlock + tid] += t;
      cnt[l * kBlock + tid] += 1.0;
    }
  }
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if (tid < off)
      for (int l = 0; l < n_labels; ++l) {
        acc[l * kBlock + tid] += acc[l * kBlock + tid + off];
        cnt[l * kBlock + tid] += cnt[l * kBlock + tid + off];
      }
    __syncthreads();
  }
  if (tid < n_labels) {
    part_sum[(size_t)blockIdx.x * n_labels + tid] = acc[tid * kBlock];
    part_cnt[(size_t)blockIdx.x * n_labels + tid] = (int64_t)cnt[tid * kBlock];
  }
}

// kSecond = false: mean_out = sum / count; true: std_out = sqrt(sum of squared deviations / count)
template <bool kSecond>
__global__ void label_final_kernel(const double* __restrict__ part_sum, const int64_t* __restrict__ part_cnt, int n_blocks,
                                   int n_labels, double* __restrict__ out, int64_t* __restrict__ count_out) {
  const int l = threadIdx.x;
  if (l >= n_labels) return;
  double s = 0.0;
  int64_t c = 0;
  for (int b = 0; b < n_blocks; ++b) { s += part_sum[(size_t)b * n_labels + l]; c += part_cnt[(size_t)b * n_labels + l]; }
  const double m = c > 0 ? s / (double)c : (double)NAN;  // numpy: mean of an empty slice is NaN
  out[l] = kSecond ? sqrt(m) : m;
  if (count_out) count_out[l] = c;
}

}  // namespace

extern "C" {

int t2fit_union_mask_dev(const uint8_t* masks_dev, int n_masks, int64_t n_vox, uint8_t* mask_out, int64_t* idx_out,
                         int64_t* count_out, void* stream) {
  if (!masks_dev || !mask_out || !idx_out || !count_out) return fail(T2FIT_E_INVALID, "NULL pointer");
  if (n_masks < 1 || n_vox < 0) return fail(T2FIT_E_INVALID, "n_masks < 1 or n_vox < 0");
  hipStream_t st = (hipStream_t)stream;
  if (n_vox == 0) {
    T2_HIP(hipMemsetAsync(count_out, 0, sizeof(int64_t), st));
    return T2FIT_OK;
  }
  const int64_t n_tiles = (n_vox + kScanTile - 1) / kScanTile;
  if (n_tiles > 0x7fffffffLL) return fail(T2FIT_E_INVALID, "n_vox too large");
  int64_t* tiles = nullptr;
  T2_HIP(hipMallocAsync((void**)&tiles, (size_t)n_tiles * sizeof(int64_t), st));
  hipLaunchKernelGGL(mask_count_kernel, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, masks_dev, n_masks, n_vox, mask_out, tiles);
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, st, tiles, n_tiles, count_out);
  hipLaunchKernelGGL(mask_write_kernel, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, (const uint8_t*)mask_out, n_vox,
                     (const int64_t*)tiles, idx_out);
  T2_HIP(hipGetLastError());
  T2_HIP(hipFreeAsync(tiles, st));
  return T2FIT_OK;
}

int t2fit_label_stats_dev(const float* map_dev, const int32_t* label_dev, int64_t n_vox, int n_labels, double* mean_out,
                          double* std_out, int64_t* count_out, void* stream) {
  if (!map_dev || !label_dev || !mean_out || !std_out) return fail(T2FIT_E_INVALID, "NULL pointer");
  if (n_vox < 0 || n_labels < 1 || n_labels > kMaxLabels) return fail(T2FIT_E_INVALID, "n_vox < 0 or n_labels outside 1..32");
  hipStream_t st = (hipStream_t)stream;
  const int n_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (n_vox + 8 * kBlock - 1) / (8 * kBlock)));
  const int64_t span = (n_vox + n_blocks - 1) / n_blocks;
  double* part_sum = nullptr;
  int64_t* part_cnt = nullptr;
  T2_HIP(hipMallocAsync((void**)&part_sum, (size_t)n_blocks * n_labels * sizeof(double), st));
  T2_HIP(hipMallocAsync((void**)&part_cnt, (size_t)n_blocks * n_labels * sizeof(int64_t), st));
  const size_t lds = (size_t)2 * n_labels * kBlock * sizeof(double);
  auto k1 = label_partial_kernel<false>;
  auto k2 = label_partial_kernel<true>;
  T2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  T2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k2), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k1, dim3(n_blocks), dim3(kBlock), lds, st, map_dev, label_dev, n_vox, n_labels, span,
                     (const double*)nullptr, part_sum, part_cnt);
  hipLaunchKernelGGL(label_final_kernel<false>, dim3(1), dim3(kMaxLabels), 0, st, (const double*)part_sum,
                     (const int64_t*)part_cnt, n_blocks, n_labels, mean_out, count_out);
  hipLaunchKernelGGL(k2, dim3(n_blocks), dim3(kBlock), lds, st, map_dev, label_dev, n_vox, n_labels, span,
                     (const double*)mean_out, part_sum, part_cnt);
  hipLaunchKernelGGL(label_final_kernel<true>, dim3(1), dim3(kMaxLabels), 0, st, (const double*)part_sum,
                     (const int64_t*)part_cnt, n_blocks, n_labels, std_out, (int64_t*)nullptr);
  T2_HIP(hipGetLastError());
  T2_HIP(hipFreeAsync(part_sum, st));
  T2_HIP(hipFreeAsync(part_cnt, st));
  return T2FIT_OK;
}

}  // extern "C"

// t2fit_roi.hip -- gfx950 kernels and C ABI of the in-vivo atlas ROI statistics (include/t2fit.h:
// t2fit_roi_erode_dev, t2fit_roi_stats_dev).  Replaces the per-label loops of utils/ada_utils.py:130-216, :885-968
// (binary_erosion + fancy-index gather + np.mean / np.std / np.median per atlas label).
//
// The per-label masks (tissue == T) & (atlas == L) of one atlas are disjoint, so eroding each of them is ONE stencil pass
// over the integer class volume cls = (tissue == T) ? atlas : 0: a voxel keeps its class iff every neighbour of the
// structuring element lies inside the volume and has the same class (out of volume = background, scipy's border_value 0).
// The statistics are then a segmented reduction: a stable counting sort of the map values by class (voxel order inside a
// class is kept, so every result is a function of the data alone), numpy's two-round mean / std in a fixed tree per
// segment, and an exact median by radix select on the order-preserving uint32 image of the floats.
// Nothing here shares a header with the fit kernels except the error plumbing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "t2fit_error.h"
#include "t2fit_support.h"

namespace {

using t2fit::kBlock;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxRoiLabels = 256;  // one 8-bit digit: the classes 1..256 are the keys 0..255 of the counting sort

// ---- erosion ------------------------------------------------------------------------------------------------------
// A workgroup owns a tile of kTZ x kTY x kTX voxels (x innermost) and stages the class of tile + halo in LDS as uint16
// (classes are 0..256), tissue already applied, so the stencil reads one array.  A row holds kPadX - 1 unused entries,
// the left halo, the kTX interior entries (8-byte aligned: four classes are one 64-bit LDS read) and the right halo.
// A thread tests four consecutive voxels at a time on packed pairs of classes: acc |= neighbour ^ centre, survivor iff 0.
// (10 x 18 rows of 144 B = 25.3 KiB of LDS: six workgroups per CU; HBM traffic 8 B read + 4 B written per voxel, the
// halo re-reads -- (66/64)(18/16)(10/8) = 1.45 x -- come from L2.)
constexpr int kTX = 64, kTY = 16, kTZ = 8;
constexpr int kPadX = 4;
constexpr int kRow = kTX + 2 * kPadX;
constexpr int kRowsY = kTY + 2;
constexpr int kRows = kRowsY * (kTZ + 2);
constexpr int kQuads = kTX / 4;
constexpr int kStageItems = kQuads + 2;  // per row: kQuads 4-voxel loads of the interior, left halo, right halo

struct ErodeArgs {
  const int32_t* label;
  const int32_t* tissue;  // or nullptr
  int32_t tissue_value;
  int nz, ny, nx;
  int n_labels;
  int vec;  // rows are 16-byte aligned in every buffer: 128-bit loads and stores
  int tiles_x, tiles_y;
  int32_t* out;
};

__device__ inline uint32_t roi_class(int32_t lab, int32_t tis, bool has_tissue, int32_t tissue_value, int n_labels) {
  return (lab >= 1 && lab <= n_labels && (!has_tissue || tis == tissue_value)) ? (uint32_t)lab : 0u;
}

// iterations = 0: the class volume alone
__global__ __launch_bounds__(kBlock) void roi_class_kernel(const int32_t* __restrict__ label, const int32_t* __restrict__ tissue,
                                                           int32_t tissue_value, int64_t n_vox, int n_labels,
                                                           int32_t* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v < n_vox) out[v] = (int32_t)roi_class(label[v], tissue ? tissue[v] : 0, tissue != nullptr, tissue_value, n_labels);
}

template <int CONN>
__global__ __launch_bounds__(kBlock) void roi_erode_kernel(const ErodeArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t cls[kRows * kRow];
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int bx = b % a.tiles_x;
  b /= a.tiles_x;
  const int by = b % a.tiles_y;
  const int bz = b / a.tiles_y;
  const int x0 = bx * kTX, y0 = by * kTY, z0 = bz * kTZ;
  const bool has_t = a.tissue != nullptr;

  for (int item = tid; item < kRows * kStageItems; item += kBlock) {
    const int r = item / kStageItems, k = item - r * kStageItems;
    const int rz = r / kRowsY, ry = r - rz * kRowsY;
    const int y = y0 + ry - 1, z = z0 + rz - 1;
    const bool row_in = y >= 0 && y < a.ny && z >= 0 && z < a.nz;
    const int64_t base = row_in ? ((int64_t)z * a.ny + y) * a.nx : 0;
    uint16_t* row = cls + r * kRow;
    if (k < kQuads) {
      const int x = x0 + 4 * k;
      uint32_t c[4] = {0u, 0u, 0u, 0u};
      if (row_in && x < a.nx) {
        if (a.vec) {  // nx % 4 == 0: the four voxels are all inside
          const int4 L = *reinterpret_cast<const int4*>(a.label + base + x);
          const int4 T = has_t ? *reinterpret_cast<const int4*>(a.tissue + base + x) : make_int4(0, 0, 0, 0);
          c[0] = roi_class(L.x, T.x, has_t, a.tissue_value, a.n_labels);
          c[1] = roi_class(L.y, T.y, has_t, a.tissue_value, a.n_labels);
          c[2] = roi_class(L.z, T.z, has_t, a.tissue_value, a.n_labels);
          c[3] = roi_class(L.w, T.w, has_t, a.tissue_value, a.n_labels);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (x + j < a.nx)
              c[j] = roi_class(a.label[base + x + j], has_t ? a.tissue[base + x + j] : 0, has_t, a.tissue_value, a.n_labels);
        }
      }
      *reinterpret_cast<uint2*>(row + kPadX + 4 * k) = make_uint2(c[0] | (c[1] << 16), c[2] | (c[3] << 16));
    } else {
      const bool left = k == kQuads;
      const int x = left ? x0 - 1 : x0 + kTX;
      uint32_t c = 0u;
      if (row_in && x >= 0 && x < a.nx)
        c = roi_class(a.label[base + x], has_t ? a.tissue[base + x] : 0, has_t, a.tissue_value, a.n_labels);
      row[left ? kPadX - 1 : kPadX + kTX] = (uint16_t)c;
    }
  }
  __syncthreads();

  for (int item = tid; item < kTZ * kTY * kQuads; item += kBlock) {
    const int q = item % kQuads, ly = (item / kQuads) % kTY, lz = item / (kQuads * kTY);
    const int x = x0 + 4 * q, y = y0 + ly, z = z0 + lz;
    if (x >= a.nx || y >= a.ny || z >= a.nz) continue;
    const uint16_t* c = cls + ((lz + 1) * kRowsY + (ly + 1)) * kRow + kPadX + 4 * q;
    const uint2 C = *reinterpret_cast<const uint2*>(c);  // classes of voxels (0, 1) and (2, 3), low half first
    uint32_t acc01 = 0u, acc23 = 0u;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz) {
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const int rem = CONN - (dz < 0 ? -dz : dz) - (dy < 0 ? -dy : dy);  // how far this row's neighbours may go in x
        if (rem < 0) continue;
        const uint16_t* n = c + (dz * kRowsY + dy) * kRow;
        const uint2 N = (dz == 0 && dy == 0) ? C : *reinterpret_cast<const uint2*>(n);
        if (dz != 0 || dy != 0) {
          acc01 |= N.x ^ C.x;
          acc23 |= N.y ^ C.y;
        }
        if (rem >= 1) {
          const uint32_t L = n[-1], R = n[4];
          acc01 |= ((N.x << 16) | L) ^ C.x;           // neighbours at x - 1
          acc23 |= ((N.y << 16) | (N.x >> 16)) ^ C.y;
          acc01 |= ((N.x >> 16) | (N.y << 16)) ^ C.x;  // neighbours at x + 1
          acc23 |= ((N.y >> 16) | (R << 16)) ^ C.y;
        }
      }
    }
    int4 o;
    o.x = (acc01 & 0xffffu) ? 0 : (int32_t)(C.x & 0xffffu);
    o.y = (acc01 >> 16) ? 0 : (int32_t)(C.x >> 16);
    o.z = (acc23 & 0xffffu) ? 0 : (int32_t)(C.y & 0xffffu);
    o.w = (acc23 >> 16) ? 0 : (int32_t)(C.y >> 16);
    int32_t* dst = a.out + ((int64_t)z * a.ny + y) * a.nx + x;
    if (a.vec) {
      *reinterpret_cast<int4*>(dst) = o;
    } else {
      dst[0] = o.x;
      if (x + 1 < a.nx) dst[1] = o.y;
      if (x + 2 < a.nx) dst[2] = o.z;
      if (x + 3 < a.nx) dst[3] = o.w;
    }
  }
}

// ---- wave helpers -------------------------------------------------------------------------------------------------
// The lanes of the wave, among the `active` ones, whose 8-bit key equals this lane's (meaningless on an inactive lane).
// Every lane of the wave calls it.  Eight ballots, no loop over the distinct keys: the cost does not depend on the data.
__device__ inline unsigned long long wave_match8(unsigned key, bool active) {
  unsigned long long m = __ballot(active);
#pragma unroll
  for (int bit = 0; bit < 8; ++bit) {
    const bool on = (key >> bit) & 1u;
    const unsigned long long s = __ballot(on);
    m &= on ? s : ~s;
  }
  return m;
}

__device__ inline unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// exclusive prefix of v over the 256 threads of the workgroup (thread order) and the total; wsum: kWaves words of LDS
__device__ inline unsigned block_excl_scan(unsigned v, unsigned* wsum, unsigned* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned incl = v;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  __syncthreads();  // wsum may still be read from an earlier call
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  unsigned before = 0, all = 0;
  for (int i = 0; i < kWaves; ++i) {
    const unsigned s = wsum[i];
    if (i < w) before += s;
    all += s;
  }
  *total = all;
  return before + incl - v;
}

// ---- stable partition by label: counting sort on one 8-bit digit -----------------------------------------------------
// The unit of the sort is a WAVE: unit u walks the voxels [u * span, (u + 1) * span) 64 at a time, so "unit, then
// position" is voxel order.  part_*[label][unit] (label-major: the scan over units reads contiguously).

// step 1: per-unit counts of each label: all ROI voxels, and those whose map value is not NaN
__global__ __launch_bounds__(kBlock) void roi_hist_kernel(const float* __restrict__ map, const int32_t* __restrict__ roi,
                                                          int64_t n_vox, int n_labels, int64_t span, unsigned n_units,
                                                          unsigned* __restrict__ part_valid, unsigned* __restrict__ part_all) {
  __shared__ unsigned h[kWaves][2][kMaxRoiLabels];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i = lane; i < kMaxRoiLabels; i += 64) { h[w][0][i] = 0u; h[w][1][i] = 0u; }
  __syncthreads();
  const unsigned unit = blockIdx.x * kWaves + w;
  const int64_t lo = unit < n_units ? (int64_t)unit * span : 0;
  const int64_t hi = unit < n_units ? (lo + span < n_vox ? lo + span : n_vox) : 0;
  for (int64_t v = lo; v < hi; v += 64) {  // wave-uniform
    const int64_t i = v + lane;
    const int32_t l = i < hi ? roi[i] : 0;
    const bool act = l >= 1 && l <= n_labels;
    if (__ballot(act) == 0ull) continue;
    const float x = act ? map[i] : 0.0f;
    const unsigned long long ok = __ballot(act && x == x);
    const unsigned long long m = wave_match8((unsigned)(l - 1), act);
    if (act && (m & lanes_below(lane)) == 0ull) {  // the group's first lane adds the group's counts: this wave's own row
      atomicAdd(&h[w][1][l - 1], (unsigned)__popcll(m));
      atomicAdd(&h[w][0][l - 1], (unsigned)__popcll(m & ok));
    }
  }
  __syncthreads();
  if (unit < n_units)
    for (int i = lane; i < n_labels; i += 64) {
      part_valid[(size_t)i * n_units + unit] = h[w][0][i];
      part_all[(size_t)i * n_units + unit] = h[w][1][i];
    }
}

// step 2a: one workgroup per label: part_valid[label][*] becomes its exclusive prefix over the units; totals out
__global__ __launch_bounds__(kBlock) void roi_scan_kernel(unsigned* __restrict__ part_valid, const unsigned* __restrict__ part_all,
                                                          unsigned n_units, unsigned* __restrict__ seg_len,
                                                          int64_t* __restrict__ count_out, int64_t* __restrict__ valid_out) {
  __shared__ unsigned wsum[kWaves];
  const int l = blockIdx.x, tid = threadIdx.x;
  unsigned* pv = part_valid + (size_t)l * n_units;
  const unsigned* pa = part_all + (size_t)l * n_units;
  const unsigned per = (n_units + kBlock - 1) / kBlock;
  const unsigned lo = (unsigned)tid * per < n_units ? (unsigned)tid * per : n_units;
  const unsigned hi = lo + per < n_units ? lo + per : n_units;
  unsigned sv = 0, sa = 0;
  for (unsigned u = lo; u < hi; ++u) { sv += pv[u]; sa += pa[u]; }
  unsigned total_v = 0, total_a = 0;
  unsigned run = block_excl_scan(sv, wsum, &total_v);
  (void)block_excl_scan(sa, wsum, &total_a);
  for (unsigned u = lo; u < hi; ++u) {
    const unsigned c = pv[u];
    pv[u] = run;
    run += c;
  }
  if (tid == 0) {
    seg_len[l] = total_v;
    count_out[l] = (int64_t)total_a;
    if (valid_out) valid_out[l] = (int64_t)total_v;
  }
}

// step 2b: exclusive prefix over the labels: seg_begin[0 .. n_labels]
__global__ __launch_bounds__(kBlock) void roi_seg_begin_kernel(const unsigned* __restrict__ seg_len, int n_labels,
                                                               unsigned* __restrict__ seg_begin) {
  __shared__ unsigned wsum[kWaves];
  const int tid = threadIdx.x;
  unsigned total = 0;
  const unsigned ex = block_excl_scan(tid < n_labels ? seg_len[tid] : 0u, wsum, &total);
  if (tid < n_labels) seg_begin[tid] = ex;
  if (tid == 0) seg_begin[n_labels] = total;
}

// step 3: every unit writes the map value of each of its ROI voxels to its label's segment, in voxel order.  The rank of a
// voxel among its wave's voxels of the same label comes from the match mask (lanes below it); the wave's cursor of that
// label -- private to the wave, advanced by the group's first lane by the group's size -- carries the rank over the
// wave's iterations.  No cursor is shared between waves: the position of a value is a function of the data alone.
__global__ __launch_bounds__(kBlock) void roi_scatter_kernel(const float* __restrict__ map, const int32_t* __restrict__ roi,
                                                             int64_t n_vox, int n_labels, int64_t span, unsigned n_units,
                                                             const unsigned* __restrict__ part_valid,
                                                             const unsigned* __restrict__ seg_begin, float* __restrict__ seg,
                                                             unsigned seg_cap) {
  __shared__ unsigned cur[kWaves][kMaxRoiLabels];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned unit = blockIdx.x * kWaves + w;
  if (unit < n_units)
    for (int i = lane; i < n_labels; i += 64) cur[w][i] = seg_begin[i] + part_valid[(size_t)i * n_units + unit];
  __syncthreads();
  const int64_t lo = unit < n_units ? (int64_t)unit * span : 0;
  const int64_t hi = unit < n_units ? (lo + span < n_vox ? lo + span : n_vox) : 0;
  for (int64_t v = lo; v < hi; v += 64) {  // wave-uniform
    const int64_t i = v + lane;
    const int32_t l = i < hi ? roi[i] : 0;
    const bool act = l >= 1 && l <= n_labels;
    if (__ballot(act) == 0ull) continue;
    const float x = act ? map[i] : 0.0f;
    const bool ok = act && x == x;  // NaN values are dropped here (counted apart by step 1)
    if (__ballot(ok) == 0ull) continue;
    const unsigned long long m = wave_match8((unsigned)(l - 1), ok);
    const int first = ok ? __ffsll((long long)m) - 1 : lane;
    unsigned at = 0u;
    if (ok && first == lane) at = atomicAdd(&cur[w][l - 1], (unsigned)__popcll(m));
    at = __shfl(at, first, 64);
    if (ok) {
      const unsigned pos = at + (unsigned)__popcll(m & lanes_below(lane));
      if (pos < seg_cap) seg[pos] = x;
    }
  }
}

// ---- per-label statistics over the segments ------------------------------------------------------------------------
// mean, std: numpy's two rounds (mean first, then the mean of squared deviations from it: a constant region gives
// exactly 0), float64, one workgroup per label: thread t sums elements t, t + 256, ... in that order, the 256 sums are
// combined by a fixed tree.  Nothing depends on the grid or on where the workgroup ran.
__device__ inline double block_tree_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if (tid < off) sh[tid] += sh[tid + off];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(kBlock) void roi_moments_kernel(const float* __restrict__ seg, const unsigned* __restrict__ seg_begin,
                                                             double* __restrict__ mean_out, double* __restrict__ std_out) {
  __shared__ double sh[kBlock];
  const int l = blockIdx.x, tid = threadIdx.x;
  const unsigned b = seg_begin[l], n = seg_begin[l + 1] - b;
  if (n == 0u) {  // numpy: mean of an empty slice is NaN
    if (tid == 0) { mean_out[l] = (double)NAN; std_out[l] = (double)NAN; }
    return;
  }
  const float* p = seg + b;
  double s = 0.0;
#pragma unroll 8
  for (unsigned i = tid; i < n; i += kBlock) s += (double)p[i];
  const double mean = block_tree_sum(s, sh) / (double)n;
  double s2 = 0.0;
#pragma unroll 8
  for (unsigned i = tid; i < n; i += kBlock) {
    const double d = (double)p[i] - mean;
    s2 += d * d;
  }
  const double var = block_tree_sum(s2, sh) / (double)n;
  if (tid == 0) { mean_out[l] = mean; std_out[l] = sqrt(var); }
}

// median: exact, by radix select on the order-preserving uint32 image of the float (negatives: all bits flipped, the
// others: sign bit flipped), four passes of 8 bits from the top.  Two ranks are selected at once, (n - 1) / 2 and n / 2
// (the same for odd n); as long as both lie in the same bins they share one histogram, and from the pass after the one
// in which they part each has its own.  Per pass every wave tallies into its own 256-bin row, equal digits of a wave
// grouped first (wave_match8), so a region whose values share their top bytes costs one LDS add per wave, not 64.
__device__ inline unsigned roi_float_key(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}

__device__ inline float roi_key_float(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__global__ __launch_bounds__(kBlock) void roi_median_kernel(const float* __restrict__ seg, const unsigned* __restrict__ seg_begin,
                                                            double* __restrict__ median_out) {
  __shared__ unsigned h[kWaves][2][256];
  __shared__ unsigned wsum[kWaves];
  __shared__ unsigned sel[2][2];  // per rank: the bin it falls into, its rank inside that bin
  const int l = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const unsigned b = seg_begin[l], n = seg_begin[l + 1] - b;
  if (n == 0u) {
    if (tid == 0) median_out[l] = (double)NAN;
    return;
  }
  const float* p = seg + b;
  unsigned rank[2] = {(n - 1u) / 2u, n / 2u};
  unsigned prefix[2] = {0u, 0u};  // the key bits decided so far
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const bool two = prefix[0] != prefix[1];  // workgroup-uniform
    for (int i = tid; i < kWaves * 2 * 256; i += kBlock) (&h[0][0][0])[i] = 0u;
    __syncthreads();
    for (unsigned base = 0; base < n; base += kBlock) {  // workgroup-uniform trip count
      const unsigned i = base + (unsigned)tid;
      const bool in = i < n;
      const unsigned key = in ? roi_float_key(p[i]) : 0u;
      const unsigned top = pass ? key >> (shift + 8) : 0u;
      const unsigned digit = (key >> shift) & 255u;
      for (int s = 0; s < (two ? 2 : 1); ++s) {
        const bool act = in && top == prefix[s];
        if (__ballot(act) == 0ull) continue;
        const unsigned long long m = wave_match8(digit, act);
        if (act && (m & lanes_below(lane)) == 0ull) atomicAdd(&h[w][s][digit], (unsigned)__popcll(m));
      }
    }
    __syncthreads();
    for (int s = 0; s < (two ? 2 : 1); ++s) {
      const unsigned t = h[0][s][tid] + h[1][s][tid] + h[2][s][tid] + h[3][s][tid];
      unsigned total = 0;
      const unsigned ex = block_excl_scan(t, wsum, &total);
      for (int r = 0; r < 2; ++r)
        if ((two ? r == s : true) && rank[r] >= ex && rank[r] < ex + t) {
          sel[r][0] = (unsigned)tid;
          sel[r][1] = rank[r] - ex;
        }
    }
    __syncthreads();
    for (int r = 0; r < 2; ++r) {
      prefix[r] = (prefix[r] << 8) | sel[r][0];
      rank[r] = sel[r][1];
    }
    __syncthreads();
  }
  if (tid == 0) median_out[l] = 0.5 * ((double)roi_key_float(prefix[0]) + (double)roi_key_float(prefix[1]));
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// (the erosion's second buffer and the sort's tables and segments are kept between calls: the scratch cache of
// t2fit_support.h)
using namespace t2fit;

}  // namespace

extern "C" {

int t2fit_roi_erode_dev(const int32_t* label_dev, const int32_t* tissue_dev, int32_t tissue_value, int nz, int ny, int nx,
                        int n_labels, int connectivity, int iterations, int32_t* roi_out, void* stream) {
  if (!label_dev || !roi_out) return fail(T2FIT_E_INVALID, "t2fit_roi_erode_dev: label_dev / roi_out is NULL");
  if (nz < 1 || ny < 1 || nx < 1) return fail(T2FIT_E_INVALID, "t2fit_roi_erode_dev: nz, ny, nx must be positive");
  if (n_labels < 1 || n_labels > kMaxRoiLabels) return fail(T2FIT_E_INVALID, "t2fit_roi_erode_dev: n_labels outside 1..256");
  if (connectivity < 1 || connectivity > 3) return fail(T2FIT_E_INVALID, "t2fit_roi_erode_dev: connectivity outside 1..3");
  if (iterations < 0 || iterations > 8) return fail(T2FIT_E_INVALID, "t2fit_roi_erode_dev: iterations outside 0..8");
  const int64_t plane = (int64_t)nz * ny;
  if (plane >= (1LL << 32) || plane * nx >= (1LL << 32))
    return fail(T2FIT_E_INVALID, "t2fit_roi_erode_dev: nz * ny * nx must be below 2^32");
  if (roi_out == label_dev || roi_out == tissue_dev)
    return fail(T2FIT_E_INVALID, "t2fit_roi_erode_dev: roi_out must not be an input (the pass is a stencil)");
  const int64_t n_vox = plane * nx;
  hipStream_t st = (hipStream_t)stream;
  if (iterations == 0) {
    hipLaunchKernelGGL(roi_class_kernel, dim3((unsigned)((n_vox + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, label_dev,
                       tissue_dev, tissue_value, n_vox, n_labels, roi_out);
    T2_HIP(hipGetLastError());
    return T2FIT_OK;
  }
  int32_t* tmp = nullptr;
  if (iterations > 1) {
    char* p = nullptr;
    T2_HIP(scratch_get(st, kScratchRoiErode, (size_t)n_vox * sizeof(int32_t), &p));
    tmp = reinterpret_cast<int32_t*>(p);
  }
  ErodeArgs a{};
  a.nz = nz; a.ny = ny; a.nx = nx;
  a.n_labels = n_labels;
  a.tiles_x = (nx + kTX - 1) / kTX;
  a.tiles_y = (ny + kTY - 1) / kTY;
  const int64_t tiles = (int64_t)a.tiles_x * a.tiles_y * ((nz + kTZ - 1) / kTZ);  // < 2^31: n_vox < 2^32, a tile has >= 8 rows of z or y
  if (tiles > 0x7fffffffLL) return fail(T2FIT_E_INVALID, "t2fit_roi_erode_dev: volume too large for one launch");
  auto kernel = connectivity == 1 ? roi_erode_kernel<1> : connectivity == 2 ? roi_erode_kernel<2> : roi_erode_kernel<3>;
  const int32_t* src = label_dev;
  for (int pass = 1; pass <= iterations; ++pass) {  // the last pass writes roi_out; the ones before alternate with tmp
    int32_t* dst = ((iterations - pass) % 2 == 0) ? roi_out : tmp;
    a.label = src;
    a.tissue = pass == 1 ? tissue_dev : nullptr;  // later passes erode the class volume itself
    a.tissue_value = tissue_value;
    a.out = dst;
    a.vec = (nx % 4 == 0 && aligned16(a.label) && aligned16(a.out) && (!a.tissue || aligned16(a.tissue))) ? 1 : 0;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(kBlock), 0, st, a);
    T2_HIP(hipGetLastError());
    src = dst;
  }
  return T2FIT_OK;
}

int t2fit_roi_stats_dev(const float* map_dev, const int32_t* roi_dev, int64_t n_vox, int n_labels, double* mean_out,
                        double* std_out, double* median_out, int64_t* count_out, int64_t* valid_out, void* stream) {
  if (!map_dev || !roi_dev || !mean_out || !std_out || !count_out)
    return fail(T2FIT_E_INVALID, "t2fit_roi_stats_dev: map_dev / roi_dev / mean_out / std_out / count_out is NULL");
  if (n_vox < 1) return fail(T2FIT_E_INVALID, "t2fit_roi_stats_dev: n_vox must be positive");
  if (n_vox >= (1LL << 32)) return fail(T2FIT_E_INVALID, "t2fit_roi_stats_dev: n_vox must be below 2^32");
  if (n_labels < 1 || n_labels > kMaxRoiLabels) return fail(T2FIT_E_INVALID, "t2fit_roi_stats_dev: n_labels outside 1..256");
  hipStream_t st = (hipStream_t)stream;
  // a unit (one wave) walks `span` consecutive voxels: 8192, more for volumes beyond 2^27 voxels (at most 16384 units)
  int64_t span = (n_vox + 16383) / 16384;
  span = span < 8192 ? 8192 : (span + 63) / 64 * 64;
  const unsigned n_units = (unsigned)((n_vox + span - 1) / span);
  const unsigned n_blocks = (n_units + kWaves - 1) / kWaves;
  const size_t part_b = align_up((size_t)n_labels * n_units * sizeof(unsigned), 16);
  const size_t len_b = align_up((size_t)(kMaxRoiLabels + 1) * sizeof(unsigned), 16);
  char* base = nullptr;
  T2_HIP(scratch_get(st, kScratchRoiStats, 2 * part_b + 2 * len_b + (size_t)n_vox * sizeof(float), &base));
  unsigned* part_valid = reinterpret_cast<unsigned*>(base);
  unsigned* part_all = reinterpret_cast<unsigned*>(base + part_b);
  unsigned* seg_len = reinterpret_cast<unsigned*>(base + 2 * part_b);
  unsigned* seg_begin = reinterpret_cast<unsigned*>(base + 2 * part_b + len_b);
  float* seg = reinterpret_cast<float*>(base + 2 * part_b + 2 * len_b);
  hipLaunchKernelGGL(roi_hist_kernel, dim3(n_blocks), dim3(kBlock), 0, st, map_dev, roi_dev, n_vox, n_labels, span, n_units,
                     part_valid, part_all);
  hipLaunchKernelGGL(roi_scan_kernel, dim3((unsigned)n_labels), dim3(kBlock), 0, st, part_valid, (const unsigned*)part_all,
                     n_units, seg_len, count_out, valid_out);
  hipLaunchKernelGGL(roi_seg_begin_kernel, dim3(1), dim3(kBlock), 0, st, (const unsigned*)seg_len, n_labels, seg_begin);
  hipLaunchKernelGGL(roi_scatter_kernel, dim3(n_blocks), dim3(kBlock), 0, st, map_dev, roi_dev, n_vox, n_labels, span, n_units,
                     (const unsigned*)part_valid, (const unsigned*)seg_begin, seg, (unsigned)n_vox);
  hipLaunchKernelGGL(roi_moments_kernel, dim3((unsigned)n_labels), dim3(kBlock), 0, st, (const float*)seg,
                     (const unsigned*)seg_begin, mean_out, std_out);
  if (median_out)
    hipLaunchKernelGGL(roi_median_kernel, dim3((unsigned)n_labels), dim3(kBlock), 0, st, (const float*)seg,
                       (const unsigned*)seg_begin, median_out);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

}  // extern "C"

// t2fit_register.hip -- gfx950 kernels and C ABI of the rigid registration's device half (include/t2fit.h:
// t2fit_register_workspace_bytes, t2fit_register_sums_dev, t2fit_shrink_dev, t2fit_shrink_mask_dev).  Stands for the
// metric evaluation inside the reference's registration_itk (utils/qmri_utils.py:167-221: correlation metric, masks,
// linear interpolator); the optimizer stays on the host (fetal_t2mapping_amd/_register.py, which also states every
// kernel here in numpy).  The correlation-ratio half of the affine registration (t2fit_register_bin_dev,
// t2fit_register_binned_sums_dev, t2fit_register_sums_lut_dev) lives here too: same bricks, same tree; and so does Mattes
// mutual information (t2fit_register_joint_hist_dev, t2fit_register_mi_gradient_dev).
//
//   register_sums_kernel    a workgroup owns a brick of 64 x 4 x 8 fixed voxels: lanes along x (coalesced fixed and mask
//                           reads; the eight moving taps of neighbouring lanes are neighbours along the image of the
//                           fixed x axis), a wave per y, every lane walks its 8 voxels in z.  43 float64 accumulators
//                           per lane; the wave adds them with a fixed xor butterfly (32, 16, .. 1: lane 0 holds the
//                           halving tree), the four waves meet in LDS, and 43 lanes store the brick's slab.
//                           <kFromLut>: f is lut[bin] of a uint8 bin volume instead of the fixed sample, nothing else
//                           differs.  <kFromMi>: 12 accumulators, (c g_a) u_j with c from the table T[n_f][n_m], which the
//                           workgroup stages in LDS once; a voxel gathers four consecutive entries of one row.
//   svr_sums_kernel         slice-to-volume registration (t2fit_svr_sums_dev): the same 43 sums for every slice of every
//                           stack in one launch, each slice under the affine of its record in a device table.  A workgroup
//                           owns a brick of 64 x 32 voxels of one slice; a lane adds 8 rows before the butterfly, so the
//                           cross-lane exchange is paid once per 8 voxels as in the volume's kernel.
//   register_joint_hist_kernel  the joint histogram of Mattes mutual information: a workgroup walks bricks (a grid stride)
//                           and adds the four fixed-point window weights of every counted voxel into its own uint64 table
//                           in LDS with 64-bit integer LDS atomics, then adds the table's nonzero entries to global memory
//                           with 64-bit integer atomics.  Integer adds are exact in any order.
//   register_binned_kernel  the same brick; a lane keeps the (bin, m) of its 8 voxels in registers.  The bins present in a
//                           wave are one 64-bit word (an OR butterfly of 1 << bin); only those run the sum's butterfly --
//                           an absent bin's column values are all +0.0 and so is their tree.  The counts are whole
//                           numbers below 2^53, exact in any order: popcounts of ballots stand for their tree.
//   tree_reduce_kernel      (t2fit_reduce.h) one pass of the tree over the slabs: a workgroup adds 256 consecutive values
//                           of one sum by halving in LDS.  Passes repeat until one value per sum is left.
//   shrink kernels          a pyramid level: the mean (the "any") of s^3 blocks, one thread per output voxel.
// The order of every floating-point addition is a function of the sizes alone; there is no floating-point atomic
// anywhere (the histogram's integer atomics are the only atomics).  Compiled with
// -ffp-contract=off: every multiply and add rounds once, as numpy's do.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "t2fit_affine.h"
#include "t2fit_error.h"
#include "t2fit_mattes.h"
#include "t2fit_reduce.h"
#include "t2fit_support.h"

namespace {

using t2fit::align_up, t2fit::ceil_div, t2fit::kBlock;
using t2fit::Affine, t2fit::Dims, t2fit::coord, t2fit::sample_metric;
using t2fit::bin_of, t2fit::parzen, t2fit::deposit, t2fit::zero_u64_kernel;
using t2fit::wave_butterfly, t2fit::TreePasses, t2fit::tree_plan, t2fit::tree_launch;

constexpr int kBX = 64, kBY = 4, kBZ = 8;  // the brick; kBX lanes of a wave, kBY waves
constexpr int kSums = T2FIT_REGISTER_SUMS;
constexpr size_t kAlign = 256;
static_assert(kBX == 64 && kBX * kBY == kBlock, "a wave per row of the brick");

constexpr int kMaxBins = 64;  // the bins of a wave fit one 64-bit presence word
constexpr int kMinMovingBins = 5;
constexpr int kMiSums = T2FIT_REGISTER_MI_SUMS;
constexpr int kHistGrid = 2048;  // workgroups of the joint histogram at most: each flushes its table once

enum SumsMode { kFromFixed = 0, kFromLut = 1, kFromMi = 2 };

struct SumsArgs {
  const float* fixed;        // <kFromFixed>
  const uint8_t* bins;       // <kFromLut>: f = lut[bins[at]]; <kFromMi> and the histogram: the row of the table
  const double* lut;         // <kFromMi>: the table T[n_bins][n_m]
  int n_bins;
  int n_m;                   // Mattes: the moving bins, t = (m - lo_m) * scale_m + 2
  double lo_m, scale_m;
  unsigned long long* hist;  // the joint histogram [n_bins][n_m]
  const uint8_t* fixed_mask;
  const float* moving;
  const uint8_t* moving_mask;
  Dims f, m;
  Affine A;
  int bricks_x, bricks_y;
  int64_t n_bricks;
  double* slabs;  // [kSums][n_bricks], the binned kernel: [2 n_bins][n_bricks]
};

// whether the fixed voxel (x, y, z), whose mask byte is set, counts; if so its interpolant m and, <true>, dm/dc:
// t2fit_affine.h's sample_metric at the voxel's image under A.  <.., true>: moving_mask may be NULL (all ones)
template <bool kGrad, bool kMaskOptional = false>
__device__ inline bool sample(const float* moving, const uint8_t* moving_mask, const Dims n, const Affine& A, int x, int y, int z,
                              double& m, double* g) {
  return sample_metric<kGrad, kMaskOptional>(moving, moving_mask, n, coord(A, 0, x, y, z), coord(A, 1, x, y, z), coord(A, 2, x, y, z), m, g);
}

template <int kMode>
__global__ __launch_bounds__(kBlock) void register_sums_kernel(const SumsArgs a) {
  constexpr int kN = kMode == kFromMi ? kMiSums : kSums;
  __shared__ double rows[kBY][kN];
  extern __shared__ double mi_table[];  // <kFromMi>: [n_bins][n_m], the launch sizes it
  if constexpr (kMode == kFromMi) {
    for (int i = threadIdx.x; i < a.n_bins * a.n_m; i += kBlock) mi_table[i] = a.lut[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int t = blockIdx.x;
  const int bx = t % a.bricks_x;
  t /= a.bricks_x;
  const int by = t % a.bricks_y, bz = t / a.bricks_y;
  const int x = bx * kBX + lane, y = by * kBY + wave;
  const bool column = x < a.f.nx && y < a.f.ny;
  const Dims n = a.m;
  double acc[kN];
#pragma unroll
  for (int q = 0; q < kN; ++q) acc[q] = 0.0;
#pragma unroll 1
  for (int k = 0; k < kBZ; ++k) {
    const int z = bz * kBZ + k;
    if (!column || z >= a.f.nz) continue;
    const int64_t at = ((int64_t)z * a.f.ny + y) * a.f.nx + x;
    if (a.fixed_mask[at] == 0) continue;
    double m, g[3];
    if (!sample<true>(a.moving, a.moving_mask, n, a.A, x, y, z, m, g)) continue;
    const double u[3] = {(double)x, (double)y, (double)z};
    if constexpr (kMode == kFromMi) {
      double dw[4];
      const int i0 = parzen<true>(m, a.lo_m, a.scale_m, a.n_m, dw);
      const double* row = mi_table + bin_of(a.bins[at], a.n_bins) * a.n_m + (i0 - 1);
      double c = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) c = c + row[j] * dw[j];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double cg = c * g[d];
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[4 * d + j] = acc[4 * d + j] + cg * u[j];
        acc[4 * d + 3] = acc[4 * d + 3] + cg;
      }
    } else {
      const double f = kMode == kFromLut ? a.lut[bin_of(a.bins[at], a.n_bins)] : (double)a.fixed[at];
      acc[0] = acc[0] + 1.0;
      acc[1] = acc[1] + f;
      acc[2] = acc[2] + m;
      acc[3] = acc[3] + f * f;
      acc[4] = acc[4] + m * m;
      acc[5] = acc[5] + f * m;
#pragma unroll
      for (int w = 0; w < 3; ++w) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double wg = w == 0 ? g[c] : (w == 1 ? f * g[c] : m * g[c]);
          const int q = 6 + 4 * (3 * w + c);
#pragma unroll
          for (int j = 0; j < 3; ++j) acc[q + j] = acc[q + j] + wg * u[j];
          acc[q + 3] = acc[q + 3] + wg;
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kN; ++q) {
    const double s = wave_butterfly(acc[q]);
    if (lane == 0) rows[wave][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < kN) {
    const int q = threadIdx.x;
    a.slabs[(int64_t)q * a.n_bricks + blockIdx.x] = (rows[0][q] + rows[2][q]) + (rows[1][q] + rows[3][q]);
  }
}

// ---- slice-to-volume registration: the 43 sums of every slice of every stack, each under its own affine ----------------
constexpr int kSvrBY = 32, kSvrRows = 8;  // a brick of a slice: 64 (x) x 32 (y); a wave owns 8 rows of it
constexpr int kSvrMaxStacks = T2FIT_SR_MAX_STACKS;
static_assert(kSvrRows * kBY == kSvrBY, "four waves of eight rows");

struct SvrRec {  // the layout include/t2fit.h documents: 128 bytes
  Affine A;
  int32_t stack, slice, active;
  int32_t pad[5];
};
static_assert(sizeof(SvrRec) == T2FIT_SVR_RECORD_BYTES && alignof(SvrRec) == 8, "the record is 128 bytes");

struct SvrStack {
  const float* fixed;
  const uint8_t* mask;  // NULL: all ones
  int lz, ly, lx;
  int bricks_x, n_bricks;
};

struct SvrArgs {
  SvrStack s[kSvrMaxStacks];
  int n_stacks;
  const float* moving;
  const uint8_t* moving_mask;  // NULL: all ones
  Dims m;
  const SvrRec* table;  // [n_slices]
  int max_bricks;       // the slabs of a record: row (43 record + q), max_bricks values
  double* slabs;
};

// Workgroup (brick b, record r): blockIdx.x = r * max_bricks + b.  The record's address is the same in every lane, so the
// affine and the indices are read once per wave.  The table is data: an inactive record, a stack or slice index out of
// range and a brick past the stack's count write a slab of +0.0; a non-finite affine fails the inside test everywhere.
__global__ __launch_bounds__(kBlock) void svr_sums_kernel(const SvrArgs a) {
  __shared__ double rows[kBY][kSums];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = (int)(blockIdx.x / (unsigned)a.max_bricks), b = (int)(blockIdx.x % (unsigned)a.max_bricks);
  const SvrRec& rec = a.table[r];
  double* slab = a.slabs + (int64_t)r * kSums * a.max_bricks + b;
  const int s = rec.stack, k = rec.slice;
  bool live = rec.active != 0 && s >= 0 && s < a.n_stacks;
  const SvrStack& st = a.s[live ? s : 0];
  live = live && k >= 0 && k < st.lz && b < st.n_bricks;
  if (!live) {
    if (threadIdx.x < kSums) slab[(int64_t)threadIdx.x * a.max_bricks] = 0.0;
    return;
  }
  const int bx = b % st.bricks_x, by = b / st.bricks_x;
  const int x = bx * kBX + lane, ly = st.ly, lx = st.lx;
  const float* fixed = st.fixed + (int64_t)k * ly * lx;
  const uint8_t* fmask = st.mask ? st.mask + (int64_t)k * ly * lx : nullptr;
  const Affine A = rec.A;
  const Dims n = a.m;
  double acc[kSums];
#pragma unroll
  for (int q = 0; q < kSums; ++q) acc[q] = 0.0;
#pragma unroll 1
  for (int i = 0; i < kSvrRows; ++i) {
    const int y = by * kSvrBY + wave * kSvrRows + i;
    if (x >= lx || y >= ly) continue;
    const int64_t at = (int64_t)y * lx + x;
    if (fmask && fmask[at] == 0) continue;
    double m, g[3];
    if (!sample<true, true>(a.moving, a.moving_mask, n, A, x, y, k, m, g)) continue;
    const double u[3] = {(double)x, (double)y, (double)k};
    const double f = (double)fixed[at];
    acc[0] = acc[0] + 1.0;
    acc[1] = acc[1] + f;
    acc[2] = acc[2] + m;
    acc[3] = acc[3] + f * f;
    acc[4] = acc[4] + m * m;
    acc[5] = acc[5] + f * m;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double wg = w == 0 ? g[c] : (w == 1 ? f * g[c] : m * g[c]);
        const int q = 6 + 4 * (3 * w + c);
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[q + j] = acc[q + j] + wg * u[j];
        acc[q + 3] = acc[q + 3] + wg;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kSums; ++q) {
    const double v = wave_butterfly(acc[q]);
    if (lane == 0) rows[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    const int q = threadIdx.x;
    slab[(int64_t)q * a.max_bricks] = (rows[0][q] + rows[2][q]) + (rows[1][q] + rows[3][q]);
  }
}

// hist[b][i0 - 1 + j] += floor(w_j 2^30 + 0.5) for every counted voxel; the caller has zeroed hist
__global__ __launch_bounds__(kBlock) void register_joint_hist_kernel(const SumsArgs a) {
  extern __shared__ unsigned long long mi_hist[];  // [n_bins][n_m], the launch sizes it
  const int n_entries = a.n_bins * a.n_m;
  for (int i = threadIdx.x; i < n_entries; i += kBlock) mi_hist[i] = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t brick = blockIdx.x; brick < a.n_bricks; brick += gridDim.x) {
    int t = (int)brick;
    const int bx = t % a.bricks_x;
    t /= a.bricks_x;
    const int by = t % a.bricks_y, bz = t / a.bricks_y;
    const int x = bx * kBX + lane, y = by * kBY + wave;
    if (x >= a.f.nx || y >= a.f.ny) continue;
#pragma unroll 1
    for (int k = 0; k < kBZ; ++k) {
      const int z = bz * kBZ + k;
      if (z >= a.f.nz) break;
      const int64_t at = ((int64_t)z * a.f.ny + y) * a.f.nx + x;
      if (a.fixed_mask[at] == 0) continue;
      double m, w[4];
      if (!sample<false>(a.moving, a.moving_mask, a.m, a.A, x, y, z, m, nullptr)) continue;
      const int i0 = parzen<false>(m, a.lo_m, a.scale_m, a.n_m, w);
      unsigned long long* row = mi_hist + bin_of(a.bins[at], a.n_bins) * a.n_m + (i0 - 1);
      deposit(row, w);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_entries; i += kBlock)
    if (mi_hist[i] != 0ull) atomicAdd(&a.hist[i], mi_hist[i]);
}

// slabs[b] = N_b and slabs[n_bins + b] = S_b of the brick, by the tree of the 43 sums
__global__ __launch_bounds__(kBlock) void register_binned_kernel(const SumsArgs a) {
  __shared__ double rows[kBY][2 * kMaxBins];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int t = blockIdx.x;
  const int bx = t % a.bricks_x;
  t /= a.bricks_x;
  const int by = t % a.bricks_y, bz = t / a.bricks_y;
  const int x = bx * kBX + lane, y = by * kBY + wave;
  const bool column = x < a.f.nx && y < a.f.ny;
  double mk[kBZ];
  int bk[kBZ];  // -1: the voxel does not count
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < kBZ; ++k) {
    const int z = bz * kBZ + k;
    mk[k] = 0.0;
    bk[k] = -1;
    if (column && z < a.f.nz) {
      const int64_t at = ((int64_t)z * a.f.ny + y) * a.f.nx + x;
      double m;
      if (a.fixed_mask[at] != 0 && sample<false>(a.moving, a.moving_mask, a.m, a.A, x, y, z, m, nullptr)) {
        const int b = bin_of(a.bins[at], a.n_bins);
        mk[k] = m;
        bk[k] = b;
        if (b < 32) lo |= 1u << b; else hi |= 1u << (b - 32);
      }
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    lo |= (uint32_t)__shfl_xor((int)lo, s, 64);
    hi |= (uint32_t)__shfl_xor((int)hi, s, 64);
  }
  uint64_t present = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)hi) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
  double my_n = 0.0, my_s = 0.0;  // lane b keeps bin b's row values
  while (present) {
    const int b = __ffsll((unsigned long long)present) - 1;
    present &= present - 1;
    double s = 0.0;
    int count = 0;
#pragma unroll
    for (int k = 0; k < kBZ; ++k) {
      const bool mine = bk[k] == b;
      if (mine) s = s + mk[k];
      count += __popcll(__ballot(mine));
    }
    s = wave_butterfly(s);
    if (lane == b) my_n = (double)count, my_s = s;
  }
  rows[wave][lane] = my_n;
  rows[wave][kMaxBins + lane] = my_s;
  __syncthreads();
  if (threadIdx.x < 2 * kMaxBins) {
    const int q = threadIdx.x, b = q & (kMaxBins - 1), which = q / kMaxBins;
    if (b < a.n_bins)
      a.slabs[(int64_t)(which * a.n_bins + b) * a.n_bricks + blockIdx.x] = (rows[0][q] + rows[2][q]) + (rows[1][q] + rows[3][q]);
  }
}

// bin = clamp(floor(((double)f - lo) * scale), 0, n_bins - 1); NaN: 0
__global__ __launch_bounds__(kBlock) void register_bin_kernel(const float* __restrict__ src, int64_t n, double lo, double scale, int n_bins,
                                                              uint8_t* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n) return;
  const double b = floor(((double)src[v] - lo) * scale), top = (double)(n_bins - 1);
  out[v] = (uint8_t)(b > 0.0 ? (b > top ? top : b) : 0.0);
}

__global__ void register_lut_kernel(const double* __restrict__ binned, int n_bins, double* __restrict__ lut) {
  const int b = threadIdx.x;
  if (b < n_bins) lut[b] = binned[b] > 0.0 ? binned[n_bins + b] / binned[b] : 0.0;
}

__global__ __launch_bounds__(kBlock) void shrink_kernel(const float* __restrict__ src, Dims n, int s, Dims o, float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= (int64_t)o.nz * o.ny * o.nx) return;
  const int x = (int)(v % o.nx);
  const int64_t r = v / o.nx;
  const int y = (int)(r % o.ny), z = (int)(r / o.ny);
  double acc = 0.0;
  for (int dz = 0; dz < s; ++dz)
    for (int dy = 0; dy < s; ++dy) {
      const float* row = src + ((int64_t)(z * s + dz) * n.ny + (y * s + dy)) * n.nx + (int64_t)x * s;
      for (int dx = 0; dx < s; ++dx) acc = acc + (double)row[dx];
    }
  out[v] = (float)(acc / (double)(s * s * s));
}

__global__ __launch_bounds__(kBlock) void shrink_mask_kernel(const uint8_t* __restrict__ src, Dims n, int s, Dims o,
                                                             uint8_t* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= (int64_t)o.nz * o.ny * o.nx) return;
  const int x = (int)(v % o.nx);
  const int64_t r = v / o.nx;
  const int y = (int)(r % o.ny), z = (int)(r / o.ny);
  uint8_t any = 0;
  for (int dz = 0; dz < s; ++dz)
    for (int dy = 0; dy < s; ++dy) {
      const uint8_t* row = src + ((int64_t)(z * s + dz) * n.ny + (y * s + dy)) * n.nx + (int64_t)x * s;
      for (int dx = 0; dx < s; ++dx) any |= row[dx] != 0;
    }
  out[v] = any;
}

// ---- host --------------------------------------------------------------------------------------------------------
constexpr int kMaxShrink = 32;

struct Plan {
  int bricks_x, bricks_y, bricks_z;
  TreePasses tree;  // pass_n[0] = the slabs
  size_t total;
};

int sums_plan(const std::string& w, int fz, int fy, int fx, Plan* plan, int n_sums = kSums) {
  if (t2fit::count_voxels(1, fz, fy, fx) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the fixed sizes must all be >= 1 and the volume at most 2^40 elements");
  plan->bricks_x = ceil_div(fx, kBX), plan->bricks_y = ceil_div(fy, kBY), plan->bricks_z = ceil_div(fz, kBZ);
  const int64_t bricks = (int64_t)plan->bricks_x * plan->bricks_y * plan->bricks_z;
  if (bricks > INT32_MAX) return t2fit::fail(T2FIT_E_INVALID, w + ": the fixed volume has more than 2^31-1 bricks (the launch index is 32-bit)");
  plan->total = 0;
  tree_plan(&plan->tree, bricks, [&](int64_t n) {
    const size_t here = plan->total;
    plan->total += align_up((size_t)n * n_sums * sizeof(double), kAlign);
    return here;
  });
  return T2FIT_OK;
}

// the checks the three entry points that sample the moving volume share, after the NULL checks and the plan
int sums_check(const std::string& w, const float* moving_dev, int mz, int my, int mx, const double* A, const void* workspace_dev,
               size_t workspace_bytes, const Plan& plan, const char* bytes_fn) {
  if (t2fit::count_voxels(1, mz, my, mx) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the moving sizes must all be >= 1 and the volume at most 2^40 elements");
  if (!t2fit::finite12(A)) return t2fit::fail(T2FIT_E_INVALID, w + ": A has a non-finite entry");
  if (reinterpret_cast<uintptr_t>(moving_dev) & 3) return t2fit::fail(T2FIT_E_INVALID, w + ": moving_dev is not aligned to 4 bytes");
  return t2fit::check_workspace(w, workspace_dev, workspace_bytes, plan.total, bytes_fn);
}

SumsArgs sums_args(const uint8_t* fixed_mask_dev, int fz, int fy, int fx, const float* moving_dev, const uint8_t* moving_mask_dev, int mz,
                   int my, int mx, const double* A, const Plan& plan, void* workspace_dev) {
  SumsArgs a;
  a.fixed = nullptr, a.bins = nullptr, a.lut = nullptr, a.n_bins = 1;
  a.n_m = kMinMovingBins, a.lo_m = 0.0, a.scale_m = 0.0, a.hist = nullptr;
  a.fixed_mask = fixed_mask_dev, a.moving = moving_dev, a.moving_mask = moving_mask_dev;
  a.f = Dims{fz, fy, fx}, a.m = Dims{mz, my, mx};
  for (int i = 0; i < 12; ++i) a.A.m[i] = A[i];
  a.bricks_x = plan.bricks_x, a.bricks_y = plan.bricks_y;
  a.n_bricks = plan.tree.pass_n[0];
  a.slabs = reinterpret_cast<double*>(static_cast<char*>(workspace_dev) + plan.tree.pass_at[0]);
  return a;
}

// the checks the two Mattes entry points share, after the NULL checks
int mi_check(const std::string& w, int n_f, int n_m, double lo_m, double scale_m) {
  if (n_f < 1 || n_f > kMaxBins) return t2fit::fail(T2FIT_E_INVALID, w + ": n_f is outside 1..64");
  if (n_m < kMinMovingBins || n_m > kMaxBins) return t2fit::fail(T2FIT_E_INVALID, w + ": n_m is outside 5..64");
  if (!std::isfinite(lo_m) || !std::isfinite(scale_m)) return t2fit::fail(T2FIT_E_INVALID, w + ": lo_m / scale_m is not finite");
  return T2FIT_OK;
}

int shrink_check(const std::string& w, const void* src, const void* out, int nz, int ny, int nx, int s, Dims* o) {
  if (!src || !out) return t2fit::fail(T2FIT_E_INVALID, w + ": src_dev / out_dev is NULL");
  if (src == out) return t2fit::fail(T2FIT_E_INVALID, w + ": out_dev must not be src_dev");
  if (t2fit::count_voxels(1, nz, ny, nx) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the sizes must all be >= 1 and the volume at most 2^40 elements");
  if (s < 1 || s > kMaxShrink) return t2fit::fail(T2FIT_E_INVALID, w + ": the shrink factor s is outside 1..32");
  if (nz / s < 1 || ny / s < 1 || nx / s < 1) return t2fit::fail(T2FIT_E_INVALID, w + ": s is larger than a size: the level would be empty");
  *o = Dims{nz / s, ny / s, nx / s};
  if (ceil_div((int64_t)o->nz * o->ny * o->nx, (int64_t)kBlock) > INT32_MAX)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the level has more than 2^39 elements");
  return T2FIT_OK;
}

// slice-to-volume registration: the bricks of every stack's slices, and the passes over 43 n_slices rows of max_bricks
struct SvrPlan {
  int bricks_x[kSvrMaxStacks], n_bricks[kSvrMaxStacks];
  int max_bricks;
  int64_t rows;  // 43 n_slices
  TreePasses tree;
  size_t total;
};

int svr_plan(const std::string& w, int n_stacks, const int32_t* lo_size, int n_slices, SvrPlan* plan) {
  if (n_stacks < 1 || n_stacks > kSvrMaxStacks) return t2fit::fail(T2FIT_E_INVALID, w + ": n_stacks must be 1 .. T2FIT_SR_MAX_STACKS");
  if (n_slices < 1) return t2fit::fail(T2FIT_E_INVALID, w + ": n_slices must be >= 1");
  plan->max_bricks = 0;
  for (int s = 0; s < n_stacks; ++s) {
    const int lz = lo_size[3 * s], ly = lo_size[3 * s + 1], lx = lo_size[3 * s + 2];
    if (t2fit::count_voxels(1, lz, ly, lx) < 0)
      return t2fit::fail(T2FIT_E_INVALID, w + ": the sizes of a stack must all be >= 1 and the stack at most 2^40 elements");
    plan->bricks_x[s] = ceil_div(lx, kBX);
    const int64_t bricks = (int64_t)plan->bricks_x[s] * ceil_div(ly, kSvrBY);
    if (bricks > INT32_MAX) return t2fit::fail(T2FIT_E_INVALID, w + ": a slice has more than 2^31-1 bricks");
    plan->n_bricks[s] = (int)bricks;
    if (plan->n_bricks[s] > plan->max_bricks) plan->max_bricks = plan->n_bricks[s];
  }
  if ((int64_t)n_slices * plan->max_bricks > INT32_MAX)
    return t2fit::fail(T2FIT_E_INVALID, w + ": more than 2^31-1 workgroups (n_slices times the largest brick count of a slice)");
  plan->rows = (int64_t)kSums * n_slices;
  plan->total = 0;
  tree_plan(&plan->tree, plan->max_bricks, [&](int64_t n) {
    const size_t here = plan->total;
    plan->total += align_up((size_t)n * (size_t)plan->rows * sizeof(double), kAlign);
    return here;
  });
  return T2FIT_OK;
}

}  // namespace

extern "C" {

int t2fit_svr_table_bytes(int n_slices, size_t* bytes) {
  const std::string w("t2fit_svr_table_bytes");
  if (!bytes) return t2fit::fail(T2FIT_E_INVALID, w + ": bytes is NULL");
  if (n_slices < 1) return t2fit::fail(T2FIT_E_INVALID, w + ": n_slices must be >= 1");
  *bytes = (size_t)n_slices * sizeof(SvrRec);
  return T2FIT_OK;
}

int t2fit_svr_table_host(int n_slices, const double* A, const int32_t* stack, const int32_t* slice, const uint8_t* active, int n_stacks,
                         const int32_t* lo_size, void* table_host, size_t bytes) {
  const std::string w("t2fit_svr_table_host");
  if (!A || !stack || !slice || !active || !lo_size || !table_host)
    return t2fit::fail(T2FIT_E_INVALID, w + ": A / stack / slice / active / lo_size / table_host is NULL");
  SvrPlan plan;
  const int rc = svr_plan(w, n_stacks, lo_size, n_slices, &plan);
  if (rc != T2FIT_OK) return rc;
  if (bytes < (size_t)n_slices * sizeof(SvrRec))
    return t2fit::fail(T2FIT_E_INVALID, w + ": the table is smaller than t2fit_svr_table_bytes says");
  for (int r = 0; r < n_slices; ++r) {  // every record is checked before a byte is written
    if (!t2fit::finite12(A + 12 * r)) return t2fit::fail(T2FIT_E_INVALID, w + ": record " + std::to_string(r) + ": A has a non-finite entry");
    if (stack[r] < 0 || stack[r] >= n_stacks)
      return t2fit::fail(T2FIT_E_INVALID, w + ": record " + std::to_string(r) + ": the stack index is outside 0 .. n_stacks - 1");
    if (slice[r] < 0 || slice[r] >= lo_size[3 * stack[r]])
      return t2fit::fail(T2FIT_E_INVALID, w + ": record " + std::to_string(r) + ": the slice index is outside its stack");
  }
  for (int r = 0; r < n_slices; ++r) {
    SvrRec rec = {};
    for (int i = 0; i < 12; ++i) rec.A.m[i] = A[12 * r + i];
    rec.stack = stack[r], rec.slice = slice[r], rec.active = active[r] != 0;
    std::memcpy(static_cast<char*>(table_host) + (size_t)r * sizeof(SvrRec), &rec, sizeof(SvrRec));
  }
  return T2FIT_OK;
}

int t2fit_svr_workspace_bytes(int n_stacks, const int32_t* lo_size, int n_slices, size_t* bytes) {
  const std::string w("t2fit_svr_workspace_bytes");
  if (!lo_size || !bytes) return t2fit::fail(T2FIT_E_INVALID, w + ": lo_size / bytes is NULL");
  SvrPlan plan;
  const int rc = svr_plan(w, n_stacks, lo_size, n_slices, &plan);
  if (rc != T2FIT_OK) return rc;
  *bytes = plan.total;
  return T2FIT_OK;
}

int t2fit_svr_sums_dev(int n_stacks, const float* const* fixed_dev, const uint8_t* const* fixed_mask_dev, const int32_t* lo_size,
                       const float* moving_dev, const uint8_t* moving_mask_dev, int mz, int my, int mx, const void* table_dev,
                       int n_slices, double* sums_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  const std::string w("t2fit_svr_sums_dev");
  if (!fixed_dev || !lo_size || !moving_dev || !table_dev || !sums_dev || !workspace_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": fixed_dev / lo_size / moving_dev / table_dev / sums_dev / workspace_dev is NULL");
  SvrPlan plan;
  const int rc = svr_plan(w, n_stacks, lo_size, n_slices, &plan);
  if (rc != T2FIT_OK) return rc;
  if (t2fit::count_voxels(1, mz, my, mx) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the moving sizes must all be >= 1 and the volume at most 2^40 elements");
  SvrArgs a = {};
  for (int s = 0; s < n_stacks; ++s) {
    if (!fixed_dev[s]) return t2fit::fail(T2FIT_E_INVALID, w + ": a stack pointer is NULL");
    if (reinterpret_cast<uintptr_t>(fixed_dev[s]) & 3) return t2fit::fail(T2FIT_E_INVALID, w + ": a stack is not aligned to 4 bytes");
    a.s[s].fixed = fixed_dev[s], a.s[s].mask = fixed_mask_dev ? fixed_mask_dev[s] : nullptr;
    a.s[s].lz = lo_size[3 * s], a.s[s].ly = lo_size[3 * s + 1], a.s[s].lx = lo_size[3 * s + 2];
    a.s[s].bricks_x = plan.bricks_x[s], a.s[s].n_bricks = plan.n_bricks[s];
  }
  if (reinterpret_cast<uintptr_t>(moving_dev) & 3) return t2fit::fail(T2FIT_E_INVALID, w + ": moving_dev is not aligned to 4 bytes");
  if ((reinterpret_cast<uintptr_t>(sums_dev) & 7) || (reinterpret_cast<uintptr_t>(table_dev) & 7))
    return t2fit::fail(T2FIT_E_INVALID, w + ": sums_dev / table_dev is not aligned to 8 bytes");
  const int ws_rc = t2fit::check_workspace(w, workspace_dev, workspace_bytes, plan.total, "t2fit_svr_workspace_bytes");
  if (ws_rc != T2FIT_OK) return ws_rc;
  hipStream_t st = (hipStream_t)stream;
  a.n_stacks = n_stacks, a.moving = moving_dev, a.moving_mask = moving_mask_dev, a.m = Dims{mz, my, mx};
  a.table = static_cast<const SvrRec*>(table_dev), a.max_bricks = plan.max_bricks;
  a.slabs = reinterpret_cast<double*>(static_cast<char*>(workspace_dev) + plan.tree.pass_at[0]);
  hipLaunchKernelGGL(svr_sums_kernel, dim3((unsigned)((int64_t)n_slices * plan.max_bricks)), dim3(kBlock), 0, st, a);
  tree_launch(plan.tree, plan.rows, workspace_dev, sums_dev, st);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_register_workspace_bytes(int fz, int fy, int fx, size_t* bytes) {
  if (!bytes) return t2fit::fail(T2FIT_E_INVALID, "t2fit_register_workspace_bytes: bytes is NULL");
  Plan plan;
  const int rc = sums_plan("t2fit_register_workspace_bytes", fz, fy, fx, &plan);
  if (rc != T2FIT_OK) return rc;
  *bytes = plan.total;
  return T2FIT_OK;
}

int t2fit_register_sums_dev(const float* fixed_dev, const uint8_t* fixed_mask_dev, int fz, int fy, int fx, const float* moving_dev,
                            const uint8_t* moving_mask_dev, int mz, int my, int mx, const double* A, double* sums_dev,
                            void* workspace_dev, size_t workspace_bytes, void* stream) {
  const std::string w("t2fit_register_sums_dev");
  if (!fixed_dev || !fixed_mask_dev || !moving_dev || !moving_mask_dev || !A || !sums_dev || !workspace_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": fixed_dev / fixed_mask_dev / moving_dev / moving_mask_dev / A / sums_dev / workspace_dev is NULL");
  Plan plan;
  const int rc = sums_plan(w, fz, fy, fx, &plan);
  if (rc != T2FIT_OK) return rc;
  if (t2fit::count_voxels(1, mz, my, mx) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the moving sizes must all be >= 1 and the volume at most 2^40 elements");
  if (!t2fit::finite12(A)) return t2fit::fail(T2FIT_E_INVALID, w + ": A has a non-finite entry");
  if ((reinterpret_cast<uintptr_t>(fixed_dev) & 3) || (reinterpret_cast<uintptr_t>(moving_dev) & 3))
    return t2fit::fail(T2FIT_E_INVALID, w + ": fixed_dev / moving_dev is not aligned to 4 bytes");
  if (reinterpret_cast<uintptr_t>(sums_dev) & 7) return t2fit::fail(T2FIT_E_INVALID, w + ": sums_dev is not aligned to 8 bytes");
  const int ws_rc = t2fit::check_workspace(w, workspace_dev, workspace_bytes, plan.total, "t2fit_register_workspace_bytes");
  if (ws_rc != T2FIT_OK) return ws_rc;
  SumsArgs a = sums_args(fixed_mask_dev, fz, fy, fx, moving_dev, moving_mask_dev, mz, my, mx, A, plan, workspace_dev);
  a.fixed = fixed_dev;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(register_sums_kernel<kFromFixed>), dim3((unsigned)a.n_bricks), dim3(kBlock), 0, (hipStream_t)stream, a);
  tree_launch(plan.tree, kSums, workspace_dev, sums_dev, (hipStream_t)stream);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_register_bin_dev(const float* src_dev, int64_t n_vox, double lo, double scale, int n_bins, uint8_t* out_dev, void* stream) {
  const std::string w("t2fit_register_bin_dev");
  if (!src_dev || !out_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": src_dev / out_dev is NULL");
  if (n_vox < 1 || n_vox >= ((int64_t)1 << 39)) return t2fit::fail(T2FIT_E_INVALID, w + ": n_vox is outside 1..2^39-1");
  if (n_bins < 1 || n_bins > kMaxBins) return t2fit::fail(T2FIT_E_INVALID, w + ": n_bins is outside 1..64");
  if (!std::isfinite(lo) || !std::isfinite(scale)) return t2fit::fail(T2FIT_E_INVALID, w + ": lo / scale is not finite");
  if (reinterpret_cast<uintptr_t>(src_dev) & 3) return t2fit::fail(T2FIT_E_INVALID, w + ": src_dev is not aligned to 4 bytes");
  hipLaunchKernelGGL(register_bin_kernel, dim3((unsigned)ceil_div(n_vox, (int64_t)kBlock)), dim3(kBlock), 0, (hipStream_t)stream, src_dev,
                     n_vox, lo, scale, n_bins, out_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_register_binned_workspace_bytes(int fz, int fy, int fx, int n_bins, size_t* bytes) {
  const std::string w("t2fit_register_binned_workspace_bytes");
  if (!bytes) return t2fit::fail(T2FIT_E_INVALID, w + ": bytes is NULL");
  if (n_bins < 1 || n_bins > kMaxBins) return t2fit::fail(T2FIT_E_INVALID, w + ": n_bins is outside 1..64");
  Plan plan;
  const int rc = sums_plan(w, fz, fy, fx, &plan, 2 * n_bins);
  if (rc != T2FIT_OK) return rc;
  *bytes = plan.total;
  return T2FIT_OK;
}

int t2fit_register_binned_sums_dev(const uint8_t* bins_dev, const uint8_t* fixed_mask_dev, int fz, int fy, int fx, const float* moving_dev,
                                   const uint8_t* moving_mask_dev, int mz, int my, int mx, const double* A, int n_bins,
                                   double* binned_dev, double* lut_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  const std::string w("t2fit_register_binned_sums_dev");
  if (!bins_dev || !fixed_mask_dev || !moving_dev || !moving_mask_dev || !A || !binned_dev || !workspace_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": bins_dev / fixed_mask_dev / moving_dev / moving_mask_dev / A / binned_dev / workspace_dev is NULL");
  if (n_bins < 1 || n_bins > kMaxBins) return t2fit::fail(T2FIT_E_INVALID, w + ": n_bins is outside 1..64");
  Plan plan;
  int rc = sums_plan(w, fz, fy, fx, &plan, 2 * n_bins);
  if (rc != T2FIT_OK) return rc;
  if ((rc = sums_check(w, moving_dev, mz, my, mx, A, workspace_dev, workspace_bytes, plan, "t2fit_register_binned_workspace_bytes")) != T2FIT_OK)
    return rc;
  if ((reinterpret_cast<uintptr_t>(binned_dev) & 7) || (reinterpret_cast<uintptr_t>(lut_dev) & 7))
    return t2fit::fail(T2FIT_E_INVALID, w + ": binned_dev / lut_dev is not aligned to 8 bytes");
  hipStream_t st = (hipStream_t)stream;
  SumsArgs a = sums_args(fixed_mask_dev, fz, fy, fx, moving_dev, moving_mask_dev, mz, my, mx, A, plan, workspace_dev);
  a.bins = bins_dev, a.n_bins = n_bins;
  hipLaunchKernelGGL(register_binned_kernel, dim3((unsigned)a.n_bricks), dim3(kBlock), 0, st, a);
  tree_launch(plan.tree, 2 * n_bins, workspace_dev, binned_dev, st);
  if (lut_dev) hipLaunchKernelGGL(register_lut_kernel, dim3(1), dim3(kMaxBins), 0, st, (const double*)binned_dev, n_bins, lut_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_register_sums_lut_dev(const uint8_t* bins_dev, const double* lut_dev, int n_bins, const uint8_t* fixed_mask_dev, int fz, int fy,
                                int fx, const float* moving_dev, const uint8_t* moving_mask_dev, int mz, int my, int mx, const double* A,
                                double* sums_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  const std::string w("t2fit_register_sums_lut_dev");
  if (!bins_dev || !lut_dev || !fixed_mask_dev || !moving_dev || !moving_mask_dev || !A || !sums_dev || !workspace_dev)
    return t2fit::fail(T2FIT_E_INVALID,
                       w + ": bins_dev / lut_dev / fixed_mask_dev / moving_dev / moving_mask_dev / A / sums_dev / workspace_dev is NULL");
  if (n_bins < 1 || n_bins > kMaxBins) return t2fit::fail(T2FIT_E_INVALID, w + ": n_bins is outside 1..64");
  Plan plan;
  int rc = sums_plan(w, fz, fy, fx, &plan);
  if (rc != T2FIT_OK) return rc;
  if ((rc = sums_check(w, moving_dev, mz, my, mx, A, workspace_dev, workspace_bytes, plan, "t2fit_register_workspace_bytes")) != T2FIT_OK)
    return rc;
  if ((reinterpret_cast<uintptr_t>(sums_dev) & 7) || (reinterpret_cast<uintptr_t>(lut_dev) & 7))
    return t2fit::fail(T2FIT_E_INVALID, w + ": sums_dev / lut_dev is not aligned to 8 bytes");
  SumsArgs a = sums_args(fixed_mask_dev, fz, fy, fx, moving_dev, moving_mask_dev, mz, my, mx, A, plan, workspace_dev);
  a.bins = bins_dev, a.lut = lut_dev, a.n_bins = n_bins;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(register_sums_kernel<kFromLut>), dim3((unsigned)a.n_bricks), dim3(kBlock), 0, (hipStream_t)stream, a);
  tree_launch(plan.tree, kSums, workspace_dev, sums_dev, (hipStream_t)stream);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_register_joint_hist_dev(const uint8_t* bins_dev, const uint8_t* fixed_mask_dev, int fz, int fy, int fx, const float* moving_dev,
                                  const uint8_t* moving_mask_dev, int mz, int my, int mx, const double* A, int n_f, int n_m, double lo_m,
                                  double scale_m, uint64_t* hist_dev, void* stream) {
  const std::string w("t2fit_register_joint_hist_dev");
  if (!bins_dev || !fixed_mask_dev || !moving_dev || !moving_mask_dev || !A || !hist_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": bins_dev / fixed_mask_dev / moving_dev / moving_mask_dev / A / hist_dev is NULL");
  int rc = mi_check(w, n_f, n_m, lo_m, scale_m);
  if (rc != T2FIT_OK) return rc;
  Plan plan;
  if ((rc = sums_plan(w, fz, fy, fx, &plan, kMiSums)) != T2FIT_OK) return rc;
  if ((int64_t)fz * fy * fx > ((int64_t)1 << 32))
    return t2fit::fail(T2FIT_E_INVALID, w + ": the fixed volume has more than 2^32 voxels (a histogram entry could pass 2^63)");
  if (t2fit::count_voxels(1, mz, my, mx) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the moving sizes must all be >= 1 and the volume at most 2^40 elements");
  if (!t2fit::finite12(A)) return t2fit::fail(T2FIT_E_INVALID, w + ": A has a non-finite entry");
  if (reinterpret_cast<uintptr_t>(moving_dev) & 3) return t2fit::fail(T2FIT_E_INVALID, w + ": moving_dev is not aligned to 4 bytes");
  if (reinterpret_cast<uintptr_t>(hist_dev) & 7) return t2fit::fail(T2FIT_E_INVALID, w + ": hist_dev is not aligned to 8 bytes");
  hipStream_t st = (hipStream_t)stream;
  SumsArgs a = sums_args(fixed_mask_dev, fz, fy, fx, moving_dev, moving_mask_dev, mz, my, mx, A, plan, nullptr);
  a.slabs = nullptr;
  a.bins = bins_dev, a.n_bins = n_f, a.n_m = n_m, a.lo_m = lo_m, a.scale_m = scale_m;
  a.hist = reinterpret_cast<unsigned long long*>(hist_dev);
  const int n_entries = n_f * n_m;
  const unsigned grid = (unsigned)(a.n_bricks < kHistGrid ? a.n_bricks : kHistGrid);
  hipLaunchKernelGGL(zero_u64_kernel, dim3((unsigned)ceil_div(n_entries, kBlock)), dim3(kBlock), 0, st, a.hist, n_entries);
  hipLaunchKernelGGL(register_joint_hist_kernel, dim3(grid), dim3(kBlock), (size_t)n_entries * sizeof(unsigned long long), st, a);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_register_mi_workspace_bytes(int fz, int fy, int fx, size_t* bytes) {
  if (!bytes) return t2fit::fail(T2FIT_E_INVALID, "t2fit_register_mi_workspace_bytes: bytes is NULL");
  Plan plan;
  const int rc = sums_plan("t2fit_register_mi_workspace_bytes", fz, fy, fx, &plan, kMiSums);
  if (rc != T2FIT_OK) return rc;
  *bytes = plan.total;
  return T2FIT_OK;
}

int t2fit_register_mi_gradient_dev(const uint8_t* bins_dev, const double* table_dev, int n_f, int n_m, double lo_m, double scale_m,
                                   const uint8_t* fixed_mask_dev, int fz, int fy, int fx, const float* moving_dev,
                                   const uint8_t* moving_mask_dev, int mz, int my, int mx, const double* A, double* sums_dev,
                                   void* workspace_dev, size_t workspace_bytes, void* stream) {
  const std::string w("t2fit_register_mi_gradient_dev");
  if (!bins_dev || !table_dev || !fixed_mask_dev || !moving_dev || !moving_mask_dev || !A || !sums_dev || !workspace_dev)
    return t2fit::fail(T2FIT_E_INVALID,
                       w + ": bins_dev / table_dev / fixed_mask_dev / moving_dev / moving_mask_dev / A / sums_dev / workspace_dev is NULL");
  int rc = mi_check(w, n_f, n_m, lo_m, scale_m);
  if (rc != T2FIT_OK) return rc;
  Plan plan;
  if ((rc = sums_plan(w, fz, fy, fx, &plan, kMiSums)) != T2FIT_OK) return rc;
  if ((rc = sums_check(w, moving_dev, mz, my, mx, A, workspace_dev, workspace_bytes, plan, "t2fit_register_mi_workspace_bytes")) != T2FIT_OK)
    return rc;
  if ((reinterpret_cast<uintptr_t>(sums_dev) & 7) || (reinterpret_cast<uintptr_t>(table_dev) & 7))
    return t2fit::fail(T2FIT_E_INVALID, w + ": sums_dev / table_dev is not aligned to 8 bytes");
  SumsArgs a = sums_args(fixed_mask_dev, fz, fy, fx, moving_dev, moving_mask_dev, mz, my, mx, A, plan, workspace_dev);
  a.bins = bins_dev, a.lut = table_dev, a.n_bins = n_f, a.n_m = n_m, a.lo_m = lo_m, a.scale_m = scale_m;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(register_sums_kernel<kFromMi>), dim3((unsigned)a.n_bricks), dim3(kBlock),
                     (size_t)n_f * n_m * sizeof(double), (hipStream_t)stream, a);
  tree_launch(plan.tree, kMiSums, workspace_dev, sums_dev, (hipStream_t)stream);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_shrink_dev(const float* src_dev, int nz, int ny, int nx, int s, float* out_dev, void* stream) {
  const std::string w("t2fit_shrink_dev");
  Dims o;
  const int rc = shrink_check(w, src_dev, out_dev, nz, ny, nx, s, &o);
  if (rc != T2FIT_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(src_dev) & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 3))
    return t2fit::fail(T2FIT_E_INVALID, w + ": src_dev / out_dev is not aligned to 4 bytes");
  const int64_t n_out = (int64_t)o.nz * o.ny * o.nx;
  hipLaunchKernelGGL(shrink_kernel, dim3((unsigned)ceil_div(n_out, (int64_t)kBlock)), dim3(kBlock), 0, (hipStream_t)stream, src_dev,
                     Dims{nz, ny, nx}, s, o, out_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_shrink_mask_dev(const uint8_t* src_dev, int nz, int ny, int nx, int s, uint8_t* out_dev, void* stream) {
  const std::string w("t2fit_shrink_mask_dev");
  Dims o;
  const int rc = shrink_check(w, src_dev, out_dev, nz, ny, nx, s, &o);
  if (rc != T2FIT_OK) return rc;
  const int64_t n_out = (int64_t)o.nz * o.ny * o.nx;
  hipLaunchKernelGGL(shrink_mask_kernel, dim3((unsigned)ceil_div(n_out, (int64_t)kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     src_dev, Dims{nz, ny, nx}, s, o, out_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

}  // extern "C"

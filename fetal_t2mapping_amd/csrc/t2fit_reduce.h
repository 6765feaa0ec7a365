// t2fit_reduce.h -- the 256-fan float64 tree over rows of partials that t2fit_register.hip (the volume's sums and the
// slices' of t2fit_svr_sums_dev), t2fit_n4.hip and t2fit_seg.hip run in the same words: its kernel, its plan and its
// launches.  One text, so one summation order, which each unit's bit-identity tests pin.  (t2fit_support.h lists the
// reductions that are NOT shared.)  Only a unit that launches the tree includes this: the kernel is emitted wherever it is.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "t2fit_support.h"

namespace t2fit {

constexpr int kTreeFan = 256;  // values a workgroup of the tree adds
constexpr int kMaxPasses = 8;  // 256^8 = 2^64 values
static_assert(kTreeFan == kBlock, "a value per thread");

namespace {  // (a kernel per unit that includes this: the units are linked without relocatable device code)

// out[q][b] = the halving sum of in[q][256 b .. 256 b + 255] (zeros beyond n); grid (n_out, the number of sums)
__global__ __launch_bounds__(kBlock) void tree_reduce_kernel(const double* __restrict__ in, int64_t n, double* __restrict__ out, int64_t n_out) {
  __shared__ double s[kTreeFan];
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.y, i = (int64_t)blockIdx.x * kTreeFan + tid;
  s[tid] = i < n ? in[q * n + i] : 0.0;
  __syncthreads();
#pragma unroll
  for (int h = kTreeFan / 2; h >= 1; h >>= 1) {
    if (tid < h) s[tid] = s[tid] + s[tid + h];
    __syncthreads();
  }
  if (tid == 0) out[q * n_out + blockIdx.x] = s[0];
}

}  // namespace

// ---- host: the passes of the tree.  Pass p reads pass_n[p] values per sum at pass_at[p] of the workspace and leaves
// ceil(pass_n[p] / 256) of them for pass p + 1; the last pass (pass_n <= 256) leaves one.
struct TreePasses {
  int n_pass;
  int64_t pass_n[kMaxPasses];
  size_t pass_at[kMaxPasses];
};

// take(n) reserves the room of n values per sum and returns where it lies; first = the partials per sum, >= 1
template <class Take> void tree_plan(TreePasses* t, int64_t first, Take take) {
  t->n_pass = 0;
  for (int64_t n = first;; n = ceil_div(n, (int64_t)kTreeFan)) {
    t->pass_n[t->n_pass] = n;
    t->pass_at[t->n_pass] = take(n);
    ++t->n_pass;
    if (n <= kTreeFan) break;
  }
}

// queue the passes over `rows` sums, the last one into out_dev[rows]; rows beyond a grid's y extent take further launches
inline void tree_launch(const TreePasses& t, int64_t rows, void* workspace_dev, double* out_dev, hipStream_t st) {
  constexpr int64_t kRowsPerLaunch = 65535;
  char* ws = static_cast<char*>(workspace_dev);
  for (int p = 0; p < t.n_pass; ++p) {
    const bool last = p + 1 == t.n_pass;
    const int64_t n = t.pass_n[p], n_out = last ? 1 : t.pass_n[p + 1];
    const double* in = reinterpret_cast<const double*>(ws + t.pass_at[p]);
    double* out = last ? out_dev : reinterpret_cast<double*>(ws + t.pass_at[p + 1]);
    for (int64_t q0 = 0; q0 < rows; q0 += kRowsPerLaunch) {
      const int64_t q_n = rows - q0 < kRowsPerLaunch ? rows - q0 : kRowsPerLaunch;
      hipLaunchKernelGGL(tree_reduce_kernel, dim3((unsigned)n_out, (unsigned)q_n), dim3(kBlock), 0, st, in + q0 * n, n, out + q0 * n_out, n_out);
    }
  }
}

}  // namespace t2fit

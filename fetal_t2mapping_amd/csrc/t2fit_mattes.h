// t2fit_mattes.h -- the device rules of Mattes mutual information that the affine metric (t2fit_register.hip) and the
// free-form one (t2fit_ffd.hip) share, so that a zero lattice gives the affine's bytes: the bin of a fixed voxel, the cubic
// B-spline Parzen window of a moving sample, the fixed-point deposit into a uint64 histogram row, and the kernel that
// zeroes such a histogram (t2fit_n4.hip's histogram uses that one too).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "t2fit_support.h"

namespace t2fit {

// a bin byte above n_bins - 1 counts as n_bins - 1 (t2fit_register_bin_dev writes none)
__device__ inline int bin_of(uint8_t b, int n_bins) { return (int)b < n_bins ? (int)b : n_bins - 1; }

// The cubic B-spline Parzen window of a moving sample (include/t2fit.h has the order of operations): returns i0, and the
// four weights (<false>) or their derivatives with respect to t (<true>) on the bins i0 - 1 .. i0 + 2.  2 <= i0 <= n_m - 3
// whatever m is (a NaN lands at t = 2), so the bins stay inside a row of n_m.
template <bool kDeriv>
__device__ inline int parzen(double m, double lo, double scale, int n_m, double* w) {
  double t = (m - lo) * scale + 2.0;
  const double top = (double)(n_m - 2), last = (double)(n_m - 3);
  t = t >= 2.0 ? t : 2.0;
  t = t <= top ? t : top;
  double base = floor(t);
  base = base < last ? base : last;
  const double u = t - base, v = 1.0 - u, u2 = u * u, v2 = v * v;
  if (kDeriv) {
    w[0] = -(v2 * 0.5);
    w[1] = 1.5 * u2 - 2.0 * u;
    w[2] = (-1.5 * u2 + u) + 0.5;
    w[3] = u2 * 0.5;
  } else {
    const double u3 = u2 * u, v3 = v2 * v;
    w[0] = v3 / 6.0;
    w[1] = ((3.0 * u3 - 6.0 * u2) + 4.0) / 6.0;
    w[2] = (((-3.0 * u3 + 3.0 * u2) + 3.0 * u) + 1.0) / 6.0;
    w[3] = u3 / 6.0;
  }
  return (int)base;
}

// row[j] += floor(w_j 2^30 + 0.5), j = 0 .. 3: integer adds, exact in any order
__device__ inline void deposit(unsigned long long* row, const double* w) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned long long q = (unsigned long long)floor(w[j] * 1073741824.0 + 0.5);
    if (q != 0ull) atomicAdd(&row[j], q);
  }
}

namespace {  // (a kernel per unit that includes this: the units are linked without relocatable device code)

__global__ __launch_bounds__(kBlock) void zero_u64_kernel(unsigned long long* __restrict__ v, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) v[i] = 0ull;
}

}  // namespace

}  // namespace t2fit

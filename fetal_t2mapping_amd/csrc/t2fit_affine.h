// t2fit_affine.h -- the index affine of a resampling stage and the three small rules every kernel that samples through
// one shares (include/t2fit.h: the coordinate, the inside test, the clamp): t2fit_resample.hip and t2fit_register.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace t2fit {

struct Affine {  // c_a = ((m[4a] ix + m[4a+1] iy) + m[4a+2] iz) + m[4a+3], a = 0 is x
  double m[12];
};

struct Dims {
  int nz, ny, nx;
};

__device__ inline double coord(const Affine& A, int a, int ix, int iy, int iz) {
  return ((A.m[4 * a] * (double)ix + A.m[4 * a + 1] * (double)iy) + A.m[4 * a + 2] * (double)iz) + A.m[4 * a + 3];
}

__device__ inline bool inside_axis(double c, int n) { return c >= -0.5 && c < (double)n - 0.5; }

__device__ inline int clamp_index(double f, int n) {
  const double hi = (double)(n - 1);
  f = f < 0.0 ? 0.0 : f;
  f = f > hi ? hi : f;
  return (int)f;
}

// ---- host: the checks of an entry point that takes an affine and sizes
inline bool finite12(const double* A) {
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(A[i])) return false;
  return true;
}

// voxels of n_vol volumes of (nz, ny, nx), or -1 when a size is < 1 or the count exceeds 2^40
inline int64_t count_voxels(int n_vol, int nz, int ny, int nx) {
  if (n_vol < 1 || nz < 1 || ny < 1 || nx < 1) return -1;
  const int64_t plane = (int64_t)ny * nx, slabs = (int64_t)n_vol * nz;
  if (slabs > ((int64_t)1 << 40) / plane) return -1;
  return slabs * plane;
}

}  // namespace t2fit

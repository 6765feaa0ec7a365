// t2fit_affine.h -- the index affine of a resampling stage, the three small rules every kernel that samples through one
// shares (include/t2fit.h: the coordinate, the inside test, the clamp), and the two samples built on them, each written
// at a continuous index so that the affine stages (t2fit_register.hip, t2fit_resample.hip) and the free-form one
// (t2fit_ffd.hip) run the same text: the metric's sample and the resampling sample.
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

// ---- the metric's sample at a continuous index (cx, cy, cz) of the moving volume: registration under an affine, the
// free-form deformation at c(x) (a zero lattice gives the affine's bytes).
__device__ inline double lerp(double p, double q, double w) { return w == 0.0 ? p : p + w * (q - p); }

// whether a fixed voxel that lands at (cx, cy, cz) counts -- inside the volume and the nearest node's mask byte set; if so
// its trilinear interpolant m and, <true>, dm/dc (zero along an axis where the taps coincide or the index is below the
// first node).  <.., true>: moving_mask may be NULL (all ones)
template <bool kGrad, bool kMaskOptional = false>
__device__ inline bool sample_metric(const float* moving, const uint8_t* moving_mask, const Dims n, double cx, double cy, double cz, double& m,
                                     double* g) {
  if (!(inside_axis(cx, n.nx) && inside_axis(cy, n.ny) && inside_axis(cz, n.nz))) return false;
  const int qx = clamp_index(floor(cx + 0.5), n.nx), qy = clamp_index(floor(cy + 0.5), n.ny), qz = clamp_index(floor(cz + 0.5), n.nz);
  if ((!kMaskOptional || moving_mask) && moving_mask[((int64_t)qz * n.ny + qy) * n.nx + qx] == 0) return false;
  const int x0 = clamp_index(floor(cx), n.nx), y0 = clamp_index(floor(cy), n.ny), z0 = clamp_index(floor(cz), n.nz);
  double dx = cx - (double)x0, dy = cy - (double)y0, dz = cz - (double)z0;
  dx = dx < 0.0 ? 0.0 : dx;
  dy = dy < 0.0 ? 0.0 : dy;
  dz = dz < 0.0 ? 0.0 : dz;
  const int x1 = x0 + 1 < n.nx ? x0 + 1 : n.nx - 1, y1 = y0 + 1 < n.ny ? y0 + 1 : n.ny - 1, z1 = z0 + 1 < n.nz ? z0 + 1 : n.nz - 1;
  const float* r00 = moving + ((int64_t)z0 * n.ny + y0) * n.nx;
  const float* r01 = moving + ((int64_t)z0 * n.ny + y1) * n.nx;
  const float* r10 = moving + ((int64_t)z1 * n.ny + y0) * n.nx;
  const float* r11 = moving + ((int64_t)z1 * n.ny + y1) * n.nx;
  const double v000 = r00[x0], v001 = r00[x1], v010 = r01[x0], v011 = r01[x1];
  const double v100 = r10[x0], v101 = r10[x1], v110 = r11[x0], v111 = r11[x1];
  const double l00 = lerp(v000, v001, dx), l01 = lerp(v010, v011, dx), l10 = lerp(v100, v101, dx), l11 = lerp(v110, v111, dx);
  const double p0 = lerp(l00, l01, dy), p1 = lerp(l10, l11, dy);
  m = lerp(p0, p1, dz);
  if (!kGrad) return true;
  g[0] = lerp(lerp(v001 - v000, v011 - v010, dy), lerp(v101 - v100, v111 - v110, dy), dz);
  g[1] = lerp(l01 - l00, l11 - l10, dz);
  g[2] = p1 - p0;
  if (x1 == x0 || cx < 0.0) g[0] = 0.0;
  if (y1 == y0 || cy < 0.0) g[1] = 0.0;
  if (z1 == z0 || cz < 0.0) g[2] = 0.0;
  return true;
}

// ---- the resampling sample at (cx, cy, cz): the stack reconstruction under an affine, the free-form warp at c(x).
// One level of the interpolation, weight w in (0, 1): lo + w (hi - lo).  An infinite lo makes that the NaN of Inf - Inf,
// where the weighted mean it stands for is that Inf (NaN only against the opposite Inf): lo + hi is just that, and is NaN
// wherever lo or hi is.  Finite values never take the branch.
__device__ inline double lerp_inf(double lo, double hi, double w) {
  const double r = lo + w * (hi - lo);
  return __builtin_expect(r != r, 0) ? lo + hi : r;
}

// Linear sample of a volume of `n`; fetch(x, y, z) returns the node as a double.  False outside the volume, where nothing
// is fetched and the caller's default stands; else r is the sample before any cast.  A weight that is exactly 0 skips
// the upper tap: a row, a plane and the volume are each evaluated only where their weight asks for them.
template <typename Fetch>
__device__ inline bool sample_linear(const Fetch& fetch, const Dims n, double cx, double cy, double cz, double& r) {
  if (!(inside_axis(cx, n.nx) && inside_axis(cy, n.ny) && inside_axis(cz, n.nz))) return false;
  const int x0 = clamp_index(floor(cx), n.nx), y0 = clamp_index(floor(cy), n.ny), z0 = clamp_index(floor(cz), n.nz);
  double dx = cx - (double)x0, dy = cy - (double)y0, dz = cz - (double)z0;
  dx = dx < 0.0 ? 0.0 : dx;
  dy = dy < 0.0 ? 0.0 : dy;
  dz = dz < 0.0 ? 0.0 : dz;
  const int x1 = x0 + 1 < n.nx ? x0 + 1 : n.nx - 1, y1 = y0 + 1 < n.ny ? y0 + 1 : n.ny - 1, z1 = z0 + 1 < n.nz ? z0 + 1 : n.nz - 1;
  auto row = [&](int z, int y) {
    double v = fetch(x0, y, z);
    if (dx != 0.0) {
      const double hi = fetch(x1, y, z);
      v = lerp_inf(v, hi, dx);
    }
    return v;
  };
  auto plane = [&](int z) {
    double v = row(z, y0);
    if (dy != 0.0) {
      const double hi = row(z, y1);
      v = lerp_inf(v, hi, dy);
    }
    return v;
  };
  r = plane(z0);
  if (dz != 0.0) {
    const double hi = plane(z1);
    r = lerp_inf(r, hi, dz);
  }
  return true;
}

struct MemFetch {  // a float32 volume in memory
  const float* v;
  int ny, nx;
  __device__ inline double operator()(int x, int y, int z) const { return (double)v[((int64_t)z * ny + y) * nx + x]; }
};

// nearest: the 32-bit pattern of the node floor(c + 0.5), clamped into the volume
__device__ inline uint32_t sample_nearest(const uint32_t* v, const Dims n, double cx, double cy, double cz, uint32_t default_bits) {
  if (!(inside_axis(cx, n.nx) && inside_axis(cy, n.ny) && inside_axis(cz, n.nz))) return default_bits;
  const int x = clamp_index(floor(cx + 0.5), n.nx), y = clamp_index(floor(cy + 0.5), n.ny), z = clamp_index(floor(cz + 0.5), n.nz);
  return v[((int64_t)z * n.ny + y) * n.nx + x];
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

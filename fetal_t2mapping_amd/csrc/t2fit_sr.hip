// t2fit_sr.hip -- gfx950 kernels and C ABI of the super-resolution reconstruction's acquisition operator (include/t2fit.h:
// t2fit_sr_plan_host, t2fit_sr_forward_dev, t2fit_sr_adjoint_dev, t2fit_sr_workspace_bytes).  A thick slice is the
// slice-profile average of the 1 mm volume; fetal_t2mapping_amd/_sr.py restates the operator, its adjoint and the
// proximal-gradient loop built on them in numpy.
//
// One definition of the weight of a pair (stack sample j, voxel v) serves both kernels (pair_weight below): it is formed
// from u = coord(B, v) in both, so the matrix and its transpose hold the same bits.
//   sr_forward_kernel  one thread per stack sample, lanes along stack x.  The box of voxels around B^-1 j (radii from
//                      t2fit_sr_plan_host) is walked once per chunk of kSrChunk echoes: the weights and the normaliser are
//                      formed once and feed kSrChunk float64 accumulators held in registers.
//   sr_adjoint_kernel  one thread per voxel, lanes along x, all stacks in one pass: per stack 2 x 2 in-plane candidates and
//                      the few slices the profile reaches, again kSrChunk accumulators per walk.
//   sr_slice_forward_kernel, sr_slice_adjoint_kernel  the same pair with a rigid pose per slice (t2fit_sr_slice_*): the
//                      affines come from a table in device memory; the adjoint culls the slices per tile of voxels first.
// No atomics; every sum runs in the order the header fixes.  Compiled with -ffp-contract=off: one rounding per operation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "t2fit_affine.h"
#include "t2fit_error.h"
#include "t2fit_support.h"

namespace {

using t2fit::align_up, t2fit::kBlock;
using t2fit::Affine, t2fit::Dims, t2fit::coord, t2fit::finite12, t2fit::count_voxels;

constexpr int kSrChunk = 4;  // echoes per walk of the candidates (registers and occupancy at 2, 4, 8)
constexpr size_t kAlign = 256;
constexpr double kBspline3Fwhm = 1.4447034489287527;  // 2 x with x^3 / 2 - x^2 + 1 / 3 = 0
constexpr double kMaxReach = 1048576.0;               // radii beyond 2^20 voxels mean a singular affine

__host__ __device__ inline double tri(double d) {
  const double a = 1.0 - fabs(d);
  return a > 0.0 ? a : 0.0;
}

// box: par = h, 1 on -h <= d < h.  bspline3: par = a, beta3(|d| / a).
__host__ __device__ inline double prof(double d, int profile, double par) {
  if (profile == T2FIT_SR_PROFILE_BOX) return (d >= -par && d < par) ? 1.0 : 0.0;
  const double t = fabs(d) / par;
  if (t < 1.0) return (2.0 / 3.0 - t * t) + 0.5 * ((t * t) * t);
  if (t < 2.0) {
    const double q = 2.0 - t;
    return ((q * q) * q) / 6.0;
  }
  return 0.0;
}

__host__ __device__ inline double pair_weight(double ux, double uy, double uz, double jx, double jy, double jz, int profile,
                                              double par) {
  return (tri(ux - jx) * tri(uy - jy)) * prof(uz - jz, profile, par);
}

// the profile's parameter and the half-width of its support, in slice-index units, from thickness / slice spacing
inline void profile_params(int profile, double rel, double* par, double* hw) {
  if (profile == T2FIT_SR_PROFILE_BOX) {
    *par = *hw = rel / 2.0;
  } else {
    *par = rel / kBspline3Fwhm;
    *hw = 2.0 * *par;
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------
struct SrForwardArgs {
  const float* x;       // [n_vol][h] or NULL (weights only)
  const float* y;       // [n_vol][l] or NULL
  const uint8_t* mask;  // [l] or NULL
  float* out;           // [n_vol][l] or NULL
  double* N;            // [l] or NULL
  Dims h, l;
  Affine B, Binv;
  int rx, ry, rz;
  int profile, n_vol;
  double par;
};

// first and last index of [k - r, k + r] inside [0, n - 1], formed in double: a centre far outside gives an empty range
__device__ inline void box_range(double k, int r, int n, int* lo, int* hi) {
  double a = k - (double)r, b = k + (double)r;
  a = a < 0.0 ? 0.0 : a;
  a = a > (double)n ? (double)n : a;
  b = b > (double)(n - 1) ? (double)(n - 1) : b;
  b = b < -1.0 ? -1.0 : b;
  *lo = (int)a, *hi = (int)b;
}

__global__ __launch_bounds__(kBlock) void sr_forward_kernel(const SrForwardArgs a) {
  const int64_t n_l = (int64_t)a.l.nz * a.l.ny * a.l.nx, n_h = (int64_t)a.h.nz * a.h.ny * a.h.nx;
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= n_l) return;
  const int jx = (int)(j % a.l.nx), jy = (int)((j / a.l.nx) % a.l.ny), jz = (int)(j / ((int64_t)a.l.nx * a.l.ny));
  const int c0 = blockIdx.y * kSrChunk;
  const int nv = a.x ? (a.n_vol - c0 < kSrChunk ? a.n_vol - c0 : kSrChunk) : 0;
  int x0, x1, y0, y1, z0, z1;
  box_range(floor(coord(a.Binv, 0, jx, jy, jz) + 0.5), a.rx, a.h.nx, &x0, &x1);
  box_range(floor(coord(a.Binv, 1, jx, jy, jz) + 0.5), a.ry, a.h.ny, &y0, &y1);
  box_range(floor(coord(a.Binv, 2, jx, jy, jz) + 0.5), a.rz, a.h.nz, &z0, &z1);
  const double djx = (double)jx, djy = (double)jy, djz = (double)jz;
  double acc[kSrChunk], n_sum = 0.0;
#pragma unroll
  for (int e = 0; e < kSrChunk; ++e) acc[e] = 0.0;
  const float* x = a.x + (int64_t)c0 * n_h;
  for (int vz = z0; vz <= z1; ++vz)
    for (int vy = y0; vy <= y1; ++vy)
      for (int vx = x0; vx <= x1; ++vx) {
        const double w = pair_weight(coord(a.B, 0, vx, vy, vz), coord(a.B, 1, vx, vy, vz), coord(a.B, 2, vx, vy, vz), djx, djy,
                                     djz, a.profile, a.par);
        if (!(w > 0.0)) continue;
        n_sum = n_sum + w;
        const int64_t v = ((int64_t)vz * a.h.ny + vy) * a.h.nx + vx;
#pragma unroll
        for (int e = 0; e < kSrChunk; ++e)
          if (e < nv) acc[e] = acc[e] + w * (double)x[e * n_h + v];
      }
  if (a.N && blockIdx.y == 0) a.N[j] = n_sum;
  if (!a.out) return;
  const bool counts = n_sum > 0.0 && (!a.mask || a.mask[j] != 0);
#pragma unroll
  for (int e = 0; e < kSrChunk; ++e)
    if (e < nv) {
      const int64_t o = (int64_t)(c0 + e) * n_l + j;
      float res = 0.0f;
      if (counts) {
        double r = acc[e] / n_sum;
        if (a.y) r = r - (double)a.y[o];
        res = (float)r;
      }
      a.out[o] = res;
    }
}

// ---- adjoint ---------------------------------------------------------------------------------------------------------
struct SrStack {
  const float* r;       // [n_vol][l]
  const double* N;      // [l]
  const uint8_t* mask;  // [l] or NULL
  Dims l;
  int profile;
  Affine B;
  double par, hw;
  int nzc, pad;
};

struct SrAdjointArgs {
  SrStack s[T2FIT_SR_MAX_STACKS];
  const float* x;  // [n_vol][h] or NULL (the bare adjoint)
  float* out;      // [n_vol][h]
  Dims h;
  int n_stacks;
  double tau;
  int n_vol;
};

__global__ __launch_bounds__(kBlock) void sr_adjoint_kernel(const SrAdjointArgs a) {
  const int64_t n_h = (int64_t)a.h.nz * a.h.ny * a.h.nx;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_h) return;
  const int vx = (int)(i % a.h.nx), vy = (int)((i / a.h.nx) % a.h.ny), vz = (int)(i / ((int64_t)a.h.nx * a.h.ny));
  const int c0 = blockIdx.y * kSrChunk;
  const int nv = a.n_vol - c0 < kSrChunk ? a.n_vol - c0 : kSrChunk;
  double acc[kSrChunk];
#pragma unroll
  for (int e = 0; e < kSrChunk; ++e) acc[e] = 0.0;
  for (int s = 0; s < a.n_stacks; ++s) {
    const SrStack& k = a.s[s];
    const int64_t n_l = (int64_t)k.l.nz * k.l.ny * k.l.nx;
    const float* r = k.r + (int64_t)c0 * n_l;
    const double ux = coord(k.B, 0, vx, vy, vz), uy = coord(k.B, 1, vx, vy, vz), uz = coord(k.B, 2, vx, vy, vz);
    const double fx = floor(ux), fy = floor(uy), fz = floor(uz - k.hw);
    for (int cz = 0; cz < k.nzc; ++cz) {
      const double jz = fz + (double)cz;
      if (!(jz >= 0.0 && jz <= (double)(k.l.nz - 1))) continue;
#pragma unroll
      for (int cy = 0; cy < 2; ++cy) {
        const double jy = fy + (double)cy;
        if (!(jy >= 0.0 && jy <= (double)(k.l.ny - 1))) continue;
#pragma unroll
        for (int cx = 0; cx < 2; ++cx) {
          const double jx = fx + (double)cx;
          if (!(jx >= 0.0 && jx <= (double)(k.l.nx - 1))) continue;
          const double w = pair_weight(ux, uy, uz, jx, jy, jz, k.profile, k.par);
          if (!(w > 0.0)) continue;
          const int64_t j = ((int64_t)jz * k.l.ny + (int64_t)jy) * k.l.nx + (int64_t)jx;
          const double nj = k.N[j];
          if (!(nj > 0.0) || (k.mask && k.mask[j] == 0)) continue;
#pragma unroll
          for (int e = 0; e < kSrChunk; ++e)
            if (e < nv) acc[e] = acc[e] + (w * (double)r[e * n_l + j]) / nj;
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < kSrChunk; ++e)
    if (e < nv) {
      const int64_t o = (int64_t)(c0 + e) * n_h + i;
      a.out[o] = a.x ? (float)((double)a.x[o] - a.tau * acc[e]) : (float)acc[e];
    }
}

// ---- host --------------------------------------------------------------------------------------------------------
int profile_check(const std::string& w, int profile, double thickness) {
  if (profile != T2FIT_SR_PROFILE_BOX && profile != T2FIT_SR_PROFILE_BSPLINE3)
    return t2fit::fail(T2FIT_E_INVALID, w + ": unknown profile (T2FIT_SR_PROFILE_BOX or T2FIT_SR_PROFILE_BSPLINE3)");
  if (!(thickness > 0.0) || !std::isfinite(thickness))
    return t2fit::fail(T2FIT_E_INVALID, w + ": thickness must be finite and > 0 (in units of the slice spacing)");
  return T2FIT_OK;
}

int launch_grid(const std::string& w, int64_t n, int n_vol, dim3* grid) {
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  if (blocks > INT32_MAX) return t2fit::fail(T2FIT_E_INVALID, w + ": a volume has more than 2^39 elements");
  *grid = dim3((unsigned)blocks, (unsigned)((n_vol + kSrChunk - 1) / kSrChunk));
  return T2FIT_OK;
}

// the arithmetic of t2fit_sr_plan_host on checked pointers: one affine, its inverse by cofactors and the radii
int plan_one(const std::string& w, const double* B, const double* half, double* Binv, int32_t* radius) {
  if (!finite12(B)) return t2fit::fail(T2FIT_E_INVALID, w + ": B has a non-finite entry");
  for (int a = 0; a < 3; ++a)
    if (!(half[a] > 0.0) || !std::isfinite(half[a]))
      return t2fit::fail(T2FIT_E_INVALID, w + ": the half-widths must be finite and > 0");
  auto m = [&](int r, int c) { return B[4 * r + c]; };
  double c[3][3];  // cofactors
  c[0][0] = m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1);
  c[0][1] = m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2);
  c[0][2] = m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0);
  c[1][0] = m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2);
  c[1][1] = m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0);
  c[1][2] = m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1);
  c[2][0] = m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1);
  c[2][1] = m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2);
  c[2][2] = m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0);
  const double det = (m(0, 0) * c[0][0] + m(0, 1) * c[0][1]) + m(0, 2) * c[0][2];
  if (!std::isfinite(det) || det == 0.0) return t2fit::fail(T2FIT_E_INVALID, w + ": B is singular");
  double inv[12];
  int32_t rad[3];
  for (int a = 0; a < 3; ++a) {
    for (int k = 0; k < 3; ++k) inv[4 * a + k] = c[k][a] / det;
    inv[4 * a + 3] = -((inv[4 * a] * B[3] + inv[4 * a + 1] * B[7]) + inv[4 * a + 2] * B[11]);
    const double reach = (std::fabs(inv[4 * a]) * half[0] + std::fabs(inv[4 * a + 1]) * half[1]) + std::fabs(inv[4 * a + 2]) * half[2];
    if (!std::isfinite(reach) || !(reach < kMaxReach)) return t2fit::fail(T2FIT_E_INVALID, w + ": B is singular");
    rad[a] = (int32_t)std::ceil(reach) + 1;
  }
  if (!finite12(inv)) return t2fit::fail(T2FIT_E_INVALID, w + ": B is singular");
  for (int i = 0; i < 12; ++i) Binv[i] = inv[i];
  for (int a = 0; a < 3; ++a) radius[a] = rad[a];
  return T2FIT_OK;
}

// ---- a rigid pose per slice ------------------------------------------------------------------------------------------
// Slice k of a stack has its own affine; the records live in device memory (t2fit_sr_slice_table_host packs them) because
// an affine per slice does not fit the kernel argument segment.  The table is data: whatever it holds, both kernels end and
// stay inside their buffers -- every range is clamped to the grid by comparisons that are false for NaN, and every index
// that addresses memory is checked against its size.
struct SrSliceRec {  // the layout include/t2fit.h documents: 208 bytes
  Affine B, Binv;
  int32_t radius[3];
  int32_t pad;
};
static_assert(sizeof(SrSliceRec) == T2FIT_SR_SLICE_RECORD_BYTES && alignof(SrSliceRec) == 8, "the slice record is 208 bytes");

struct SrSliceForwardArgs {
  const float* x;
  const float* y;
  const uint8_t* mask;
  float* out;
  double* N;
  const SrSliceRec* table;  // [l.nz]
  Dims h, l;
  int profile, n_vol;
  double par;
  int plane_blocks;  // workgroups per slice
};

// box_range for a centre and a radius read from memory: a non-finite centre gives the empty range (lo = n, hi = -1)
__device__ inline void box_range_checked(double k, int r, int n, int* lo, int* hi) {
  const double a = k - (double)r, b = k + (double)r;
  int l = n, h = -1;
  if (a <= (double)n) l = a > 0.0 ? (int)a : 0;
  if (b >= -1.0) h = b < (double)(n - 1) ? (int)b : n - 1;
  *lo = l, *hi = h;
}

// sr_forward_kernel with the slice's record in place of the kernel-argument affine.  A workgroup lies inside one slice, so
// the record's address is the same in every lane and the affines are read once per wave, by scalar loads.
__global__ __launch_bounds__(kBlock) void sr_slice_forward_kernel(const SrSliceForwardArgs a) {
  const int64_t plane = (int64_t)a.l.ny * a.l.nx, n_l = plane * a.l.nz, n_h = (int64_t)a.h.nz * a.h.ny * a.h.nx;
  const int jz = (int)(blockIdx.x / (unsigned)a.plane_blocks);
  const int64_t p = (int64_t)(blockIdx.x % (unsigned)a.plane_blocks) * kBlock + threadIdx.x;
  if (p >= plane) return;
  const SrSliceRec& rec = a.table[jz];
  const int jx = (int)(p % a.l.nx), jy = (int)(p / a.l.nx);
  const int64_t j = (int64_t)jz * plane + p;
  const int c0 = blockIdx.y * kSrChunk;
  const int nv = a.x ? (a.n_vol - c0 < kSrChunk ? a.n_vol - c0 : kSrChunk) : 0;
  int x0, x1, y0, y1, z0, z1;
  box_range_checked(floor(coord(rec.Binv, 0, jx, jy, jz) + 0.5), rec.radius[0], a.h.nx, &x0, &x1);
  box_range_checked(floor(coord(rec.Binv, 1, jx, jy, jz) + 0.5), rec.radius[1], a.h.ny, &y0, &y1);
  box_range_checked(floor(coord(rec.Binv, 2, jx, jy, jz) + 0.5), rec.radius[2], a.h.nz, &z0, &z1);
  const double djx = (double)jx, djy = (double)jy, djz = (double)jz;
  double acc[kSrChunk], n_sum = 0.0;
#pragma unroll
  for (int e = 0; e < kSrChunk; ++e) acc[e] = 0.0;
  const float* x = a.x + (int64_t)c0 * n_h;
  for (int vz = z0; vz <= z1; ++vz)
    for (int vy = y0; vy <= y1; ++vy)
      for (int vx = x0; vx <= x1; ++vx) {
        const double w = pair_weight(coord(rec.B, 0, vx, vy, vz), coord(rec.B, 1, vx, vy, vz), coord(rec.B, 2, vx, vy, vz), djx,
                                     djy, djz, a.profile, a.par);
        if (!(w > 0.0)) continue;
        n_sum = n_sum + w;
        const int64_t v = ((int64_t)vz * a.h.ny + vy) * a.h.nx + vx;
#pragma unroll
        for (int e = 0; e < kSrChunk; ++e)
          if (e < nv) acc[e] = acc[e] + w * (double)x[e * n_h + v];
      }
  if (a.N && blockIdx.y == 0) a.N[j] = n_sum;
  if (!a.out) return;
  const bool counts = n_sum > 0.0 && (!a.mask || a.mask[j] != 0);
#pragma unroll
  for (int e = 0; e < kSrChunk; ++e)
    if (e < nv) {
      const int64_t o = (int64_t)(c0 + e) * n_l + j;
      float res = 0.0f;
      if (counts) {
        double r = acc[e] / n_sum;
        if (a.y) r = r - (double)a.y[o];
        res = (float)r;
      }
      a.out[o] = res;
    }
}

// The adjoint: a workgroup owns a tile of kTileX x kTileY x kTileZ voxels, lanes along x, one wave per z layer.
constexpr int kTileX = 16, kTileY = 4, kTileZ = 4;
constexpr int kWaves = kBlock / 64;
static_assert(kTileX * kTileY * kTileZ == kBlock && kTileX * kTileY == 64, "a wave is one z layer of the tile");
constexpr double kCullMargin = 0x1p-40;  // times the magnitude of the terms; see coord_range

struct SrSliceStack {
  const float* r;           // [n_vol][l]
  const double* N;          // [l]
  const uint8_t* mask;      // [l] or NULL
  const SrSliceRec* table;  // [l.nz]
  Dims l;
  int profile;
  double par, hw;
};

struct SrSliceAdjointArgs {
  SrSliceStack s[T2FIT_SR_MAX_STACKS];
  const float* x;  // [n_vol][h] or NULL
  float* out;      // [n_vol][h]
  Dims h;
  int n_stacks;
  double tau;
  int n_vol;
  int tiles_x, tiles_y;
};

// Bounds of coordinate a of B over the integer box [x0, x1] x [y0, y1] x [z0, z1], by intervals: each product takes its
// smaller / larger end.  A coordinate the kernel computes at a voxel of the box, and each bound here, is off its exact
// value by at most six roundings of quantities no larger than mag = sum of the largest |term|, that is by < 2^-50 mag; the
// bounds are widened by kCullMargin * mag = 2^-40 mag.  Overflowing products give infinite bounds, which keep the slice.
__device__ inline void coord_range(const Affine& B, int a, double x0, double x1, double y0, double y1, double z0, double z1,
                                   double* lo, double* hi) {
  const double px0 = B.m[4 * a] * x0, px1 = B.m[4 * a] * x1, py0 = B.m[4 * a + 1] * y0, py1 = B.m[4 * a + 1] * y1;
  const double pz0 = B.m[4 * a + 2] * z0, pz1 = B.m[4 * a + 2] * z1, c = B.m[4 * a + 3];
  const double l = (((px0 < px1 ? px0 : px1) + (py0 < py1 ? py0 : py1)) + (pz0 < pz1 ? pz0 : pz1)) + c;
  const double h = (((px0 < px1 ? px1 : px0) + (py0 < py1 ? py1 : py0)) + (pz0 < pz1 ? pz1 : pz0)) + c;
  const double ax = fabs(px0) > fabs(px1) ? fabs(px0) : fabs(px1), ay = fabs(py0) > fabs(py1) ? fabs(py0) : fabs(py1);
  const double az = fabs(pz0) > fabs(pz1) ? fabs(pz0) : fabs(pz1);
  const double mg = (((ax + ay) + az) + fabs(c)) * kCullMargin;
  *lo = l - mg, *hi = h + mg;
}

// The terms of slice k of stack st for the voxel (vx, vy, vz), pz = prof(u_z - k) > 0 already formed: the 2 x 2 in-plane
// candidates in ascending (cy, cx).  k may differ from lane to lane (it is below st.l.nz in every lane).
__device__ inline void slice_terms(const SrSliceStack& st, const float* r, int64_t n_l, int nv, int k, double pz, int vx, int vy,
                                   int vz, double* acc) {
  const SrSliceRec& rec = st.table[k];
  const double ux = coord(rec.B, 0, vx, vy, vz), uy = coord(rec.B, 1, vx, vy, vz);
  const double fx = floor(ux), fy = floor(uy);
#pragma unroll
  for (int cy = 0; cy < 2; ++cy) {
    const double jy = fy + (double)cy;
    if (!(jy >= 0.0 && jy <= (double)(st.l.ny - 1))) continue;
#pragma unroll
    for (int cx = 0; cx < 2; ++cx) {
      const double jx = fx + (double)cx;
      if (!(jx >= 0.0 && jx <= (double)(st.l.nx - 1))) continue;
      const double w = (tri(ux - jx) * tri(uy - jy)) * pz;  // pair_weight, its profile factor formed once
      if (!(w > 0.0)) continue;
      const int64_t j = ((int64_t)k * st.l.ny + (int64_t)jy) * st.l.nx + (int64_t)jx;
      const double nj = st.N[j];
      if (!(nj > 0.0) || (st.mask && st.mask[j] == 0)) continue;
#pragma unroll
      for (int e = 0; e < kSrChunk; ++e)
        if (e < nv) acc[e] = acc[e] + (w * (double)r[e * n_l + j]) / nj;
    }
  }
}

// Stage 1 (cull): per stack, in passes of kBlock slices, lane t takes slice base + t, bounds the tile's stack coordinates
// under that slice's affine and keeps the slice iff they can meet the slice's support; the survivors are compacted in
// ascending k into an LDS list (ballot and prefix count inside a wave, wave offsets in wave order).  Stage 2 (walk): every
// lane walks the list; the slice index is the same in every lane, so the record is read by scalar loads, and the profile
// factor comes from the lane's own u_z; the in-plane terms follow in slice_terms.  A pair of weight 0 is skipped, so what the cull lets through does not matter as
// long as it drops no slice that contributes.
__global__ __launch_bounds__(kBlock) void sr_slice_adjoint_kernel(const SrSliceAdjointArgs a) {
  __shared__ int list[kBlock];
  __shared__ int wave_count[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x;
  const int x0 = (tile % a.tiles_x) * kTileX, y0 = ((tile / a.tiles_x) % a.tiles_y) * kTileY;
  const int z0 = (tile / (a.tiles_x * a.tiles_y)) * kTileZ;
  const int vx = x0 + tid % kTileX, vy = y0 + (tid / kTileX) % kTileY, vz = z0 + wave;
  const bool live = vx < a.h.nx && vy < a.h.ny && vz < a.h.nz;
  const double bx0 = (double)x0, bx1 = (double)((x0 + kTileX < a.h.nx ? x0 + kTileX : a.h.nx) - 1);
  const double by0 = (double)y0, by1 = (double)((y0 + kTileY < a.h.ny ? y0 + kTileY : a.h.ny) - 1);
  const double bz0 = (double)z0, bz1 = (double)((z0 + kTileZ < a.h.nz ? z0 + kTileZ : a.h.nz) - 1);
  const int64_t n_h = (int64_t)a.h.nz * a.h.ny * a.h.nx;
  const int c0 = blockIdx.y * kSrChunk;
  const int nv = a.n_vol - c0 < kSrChunk ? a.n_vol - c0 : kSrChunk;
  double acc[kSrChunk];
#pragma unroll
  for (int e = 0; e < kSrChunk; ++e) acc[e] = 0.0;
  int held = -1;  // the slice this lane has met and not yet added, or -1
  double held_pz = 0.0;
  for (int s = 0; s < a.n_stacks; ++s) {
    const SrSliceStack& st = a.s[s];
    const int64_t n_l = (int64_t)st.l.nz * st.l.ny * st.l.nx;
    const float* r = st.r + (int64_t)c0 * n_l;
    for (int base = 0; base < st.l.nz; base += kBlock) {
      const int mine = base + tid;
      bool keep = false;
      if (mine < st.l.nz) {
        const SrSliceRec& rec = st.table[mine];
        double lo, hi;
        coord_range(rec.B, 2, bx0, bx1, by0, by1, bz0, bz1, &lo, &hi);
        keep = hi >= (double)mine - st.hw && lo <= (double)mine + st.hw;
        coord_range(rec.B, 0, bx0, bx1, by0, by1, bz0, bz1, &lo, &hi);
        keep = keep && hi >= -1.0 && lo <= (double)st.l.nx;
        coord_range(rec.B, 1, bx0, bx1, by0, by1, bz0, bz1, &lo, &hi);
        keep = keep && hi >= -1.0 && lo <= (double)st.l.ny;
      }
      const unsigned long long votes = __ballot(keep);
      __syncthreads();  // the walk of the pass before has read the list and the counts
      if (lane == 0) wave_count[wave] = __popcll(votes);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const int n = wave_count[w];
        before += w < wave ? n : 0;
        total += n;
      }
      if (keep) list[before + __popcll(votes & ((1ull << lane) - 1ull))] = mine;
      __syncthreads();
      // Lanes of a wave meet their slices at different steps of the walk, and the terms of a slice are the costly part
      // (a float64 division per echo and candidate).  So a lane only notes the slice it has met (held, held_pz) and the
      // wave adds the noted slices' terms together, every lane for its own slice, when a lane that still holds one meets
      // the next, and at the end of the pass: each lane still adds its slices in ascending k.
      for (int i = 0; i < total; ++i) {
        const int k = __builtin_amdgcn_readfirstlane(list[i]);
        const SrSliceRec& rec = st.table[k];
        const double pz = prof(coord(rec.B, 2, vx, vy, vz) - (double)k, st.profile, st.par);
        const bool met = live && pz > 0.0;
        if (__any(met && held >= 0)) {
          if (held >= 0) slice_terms(st, r, n_l, nv, held, held_pz, vx, vy, vz, acc);
          held = -1;
        }
        if (met) held = k, held_pz = pz;
      }
      if (held >= 0) slice_terms(st, r, n_l, nv, held, held_pz, vx, vy, vz, acc);
      held = -1;
    }
  }
  if (!live) return;
  const int64_t i = ((int64_t)vz * a.h.ny + vy) * a.h.nx + vx;
#pragma unroll
  for (int e = 0; e < kSrChunk; ++e)
    if (e < nv) {
      const int64_t o = (int64_t)(c0 + e) * n_h + i;
      a.out[o] = a.x ? (float)((double)a.x[o] - a.tau * acc[e]) : (float)acc[e];
    }
}

}  // namespace

extern "C" {

int t2fit_sr_plan_host(const double* B, const double* half, double* Binv, int32_t* radius) {
  const std::string w("t2fit_sr_plan_host");
  if (!B || !half || !Binv || !radius) return t2fit::fail(T2FIT_E_INVALID, w + ": B / half / Binv / radius is NULL");
  return plan_one(w, B, half, Binv, radius);
}

int t2fit_sr_workspace_bytes(int n_stacks, const int32_t* lo_size, int hz, int hy, int hx, int n_vol, size_t* bytes) {
  const std::string w("t2fit_sr_workspace_bytes");
  if (!lo_size || !bytes) return t2fit::fail(T2FIT_E_INVALID, w + ": lo_size / bytes is NULL");
  if (n_stacks < 1 || n_stacks > T2FIT_SR_MAX_STACKS)
    return t2fit::fail(T2FIT_E_INVALID, w + ": n_stacks must be 1 .. T2FIT_SR_MAX_STACKS");
  const int64_t n_h = count_voxels(n_vol, hz, hy, hx);
  if (n_h < 0) return t2fit::fail(T2FIT_E_INVALID, w + ": n_vol and the sizes must all be >= 1 and a volume at most 2^40 elements");
  size_t total = align_up((size_t)n_h * 4, kAlign);
  for (int s = 0; s < n_stacks; ++s) {
    const int64_t n_l = count_voxels(n_vol, lo_size[3 * s], lo_size[3 * s + 1], lo_size[3 * s + 2]);
    if (n_l < 0) return t2fit::fail(T2FIT_E_INVALID, w + ": n_vol and the sizes must all be >= 1 and a stack at most 2^40 elements");
    total += align_up((size_t)(n_l / n_vol) * 8, kAlign) + align_up((size_t)n_l * 4, kAlign);
  }
  *bytes = total;
  return T2FIT_OK;
}

int t2fit_sr_forward_dev(const float* x_dev, int hz, int hy, int hx, int n_vol, const double* B, const double* Binv,
                         const int32_t* radius, int profile, double thickness, const float* y_dev, const uint8_t* mask_dev, int lz,
                         int ly, int lx, float* out_dev, double* N_dev, void* stream) {
  const std::string w("t2fit_sr_forward_dev");
  if (!B || !Binv || !radius) return t2fit::fail(T2FIT_E_INVALID, w + ": B / Binv / radius is NULL");
  if (!out_dev && !N_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": out_dev and N_dev are both NULL");
  if ((x_dev == nullptr) != (out_dev == nullptr))
    return t2fit::fail(T2FIT_E_INVALID, w + ": x_dev and out_dev go together (both NULL: the weights only)");
  if (y_dev && !out_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": y_dev needs x_dev and out_dev");
  if (count_voxels(n_vol, hz, hy, hx) < 0 || count_voxels(n_vol, lz, ly, lx) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": n_vol and the sizes must all be >= 1 and a volume at most 2^40 elements");
  if (!finite12(B) || !finite12(Binv)) return t2fit::fail(T2FIT_E_INVALID, w + ": B / Binv has a non-finite entry");
  for (int a = 0; a < 3; ++a)
    if (radius[a] < 1 || radius[a] > (int32_t)kMaxReach + 1)
      return t2fit::fail(T2FIT_E_INVALID, w + ": a radius is < 1 or beyond 2^20 + 1 (t2fit_sr_plan_host)");
  const int rc = profile_check(w, profile, thickness);
  if (rc != T2FIT_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(x_dev) & 3) || (reinterpret_cast<uintptr_t>(y_dev) & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 3) ||
      (reinterpret_cast<uintptr_t>(N_dev) & 7))
    return t2fit::fail(T2FIT_E_INVALID, w + ": x_dev / y_dev / out_dev is not aligned to 4 bytes or N_dev not to 8");
  if (out_dev && out_dev == x_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": out_dev must not be x_dev");
  SrForwardArgs a;
  a.x = x_dev, a.y = y_dev, a.mask = mask_dev, a.out = out_dev, a.N = N_dev;
  a.h = Dims{hz, hy, hx}, a.l = Dims{lz, ly, lx};
  for (int i = 0; i < 12; ++i) a.B.m[i] = B[i], a.Binv.m[i] = Binv[i];
  a.rx = radius[0], a.ry = radius[1], a.rz = radius[2];
  a.profile = profile, a.n_vol = n_vol;
  double hw;
  profile_params(profile, thickness, &a.par, &hw);
  dim3 grid;
  const int e = launch_grid(w, (int64_t)lz * ly * lx, x_dev ? n_vol : 1, &grid);
  if (e != T2FIT_OK) return e;
  hipLaunchKernelGGL(sr_forward_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_sr_adjoint_dev(int n_stacks, const float* const* r_dev, const double* const* N_dev, const uint8_t* const* mask_dev,
                         const int32_t* lo_size, const double* B, const int32_t* profile, const double* thickness,
                         const float* x_dev, double tau, float* out_dev, int hz, int hy, int hx, int n_vol, void* stream) {
  const std::string w("t2fit_sr_adjoint_dev");
  if (!r_dev || !N_dev || !lo_size || !B || !profile || !thickness || !out_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": r_dev / N_dev / lo_size / B / profile / thickness / out_dev is NULL");
  if (n_stacks < 1 || n_stacks > T2FIT_SR_MAX_STACKS)
    return t2fit::fail(T2FIT_E_INVALID, w + ": n_stacks must be 1 .. T2FIT_SR_MAX_STACKS");
  if (count_voxels(n_vol, hz, hy, hx) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": n_vol and the sizes must all be >= 1 and a volume at most 2^40 elements");
  if (!std::isfinite(tau)) return t2fit::fail(T2FIT_E_INVALID, w + ": tau is not finite");
  if ((reinterpret_cast<uintptr_t>(x_dev) & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 3))
    return t2fit::fail(T2FIT_E_INVALID, w + ": x_dev / out_dev is not aligned to 4 bytes");
  SrAdjointArgs a = {};
  for (int s = 0; s < n_stacks; ++s) {
    SrStack& k = a.s[s];
    if (!r_dev[s] || !N_dev[s]) return t2fit::fail(T2FIT_E_INVALID, w + ": a residual or normaliser pointer is NULL");
    if ((reinterpret_cast<uintptr_t>(r_dev[s]) & 3) || (reinterpret_cast<uintptr_t>(N_dev[s]) & 7) || r_dev[s] == out_dev)
      return t2fit::fail(T2FIT_E_INVALID, w + ": a residual is not aligned to 4 bytes or is out_dev, or a normaliser not to 8");
    if (count_voxels(n_vol, lo_size[3 * s], lo_size[3 * s + 1], lo_size[3 * s + 2]) < 0)
      return t2fit::fail(T2FIT_E_INVALID, w + ": n_vol and the sizes must all be >= 1 and a stack at most 2^40 elements");
    if (!finite12(B + 12 * s)) return t2fit::fail(T2FIT_E_INVALID, w + ": B has a non-finite entry");
    const int rc = profile_check(w, profile[s], thickness[s]);
    if (rc != T2FIT_OK) return rc;
    k.r = r_dev[s], k.N = N_dev[s], k.mask = mask_dev ? mask_dev[s] : nullptr;
    k.l = Dims{lo_size[3 * s], lo_size[3 * s + 1], lo_size[3 * s + 2]};
    k.profile = profile[s];
    for (int i = 0; i < 12; ++i) k.B.m[i] = B[12 * s + i];
    profile_params(profile[s], thickness[s], &k.par, &k.hw);
    if (!(k.hw < kMaxReach)) return t2fit::fail(T2FIT_E_INVALID, w + ": thickness is beyond 2^20 slice spacings");
    k.nzc = (int)std::floor(2.0 * k.hw) + 3, k.pad = 0;
  }
  a.x = x_dev, a.out = out_dev, a.h = Dims{hz, hy, hx}, a.n_stacks = n_stacks, a.tau = tau, a.n_vol = n_vol;
  dim3 grid;
  const int e = launch_grid(w, (int64_t)hz * hy * hx, n_vol, &grid);
  if (e != T2FIT_OK) return e;
  hipLaunchKernelGGL(sr_adjoint_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_sr_slice_table_bytes(int lz, size_t* bytes) {
  const std::string w("t2fit_sr_slice_table_bytes");
  if (!bytes) return t2fit::fail(T2FIT_E_INVALID, w + ": bytes is NULL");
  if (lz < 1) return t2fit::fail(T2FIT_E_INVALID, w + ": lz must be >= 1");
  *bytes = (size_t)lz * sizeof(SrSliceRec);
  return T2FIT_OK;
}

int t2fit_sr_slice_table_host(int lz, const double* B, int profile, double thickness, void* table_host, size_t bytes) {
  const std::string w("t2fit_sr_slice_table_host");
  if (!B || !table_host) return t2fit::fail(T2FIT_E_INVALID, w + ": B / table_host is NULL");
  if (lz < 1) return t2fit::fail(T2FIT_E_INVALID, w + ": lz must be >= 1");
  if (bytes < (size_t)lz * sizeof(SrSliceRec))
    return t2fit::fail(T2FIT_E_INVALID, w + ": the table is smaller than t2fit_sr_slice_table_bytes says");
  const int rc = profile_check(w, profile, thickness);
  if (rc != T2FIT_OK) return rc;
  double par, hw;
  profile_params(profile, thickness, &par, &hw);
  const double half[3] = {1.0, 1.0, hw};
  for (int k = 0; k < lz; ++k) {  // every slice is checked before a byte is written
    SrSliceRec rec;
    const int e = plan_one(w + ": slice " + std::to_string(k), B + 12 * k, half, rec.Binv.m, rec.radius);
    if (e != T2FIT_OK) return e;
  }
  for (int k = 0; k < lz; ++k) {
    SrSliceRec rec;
    for (int i = 0; i < 12; ++i) rec.B.m[i] = B[12 * k + i];
    (void)plan_one(w, B + 12 * k, half, rec.Binv.m, rec.radius);
    rec.pad = 0;
    std::memcpy(static_cast<char*>(table_host) + (size_t)k * sizeof(SrSliceRec), &rec, sizeof(SrSliceRec));
  }
  return T2FIT_OK;
}

int t2fit_sr_slice_forward_dev(const float* x_dev, int hz, int hy, int hx, int n_vol, const void* table_dev, int profile,
                               double thickness, const float* y_dev, const uint8_t* mask_dev, int lz, int ly, int lx, float* out_dev,
                               double* N_dev, void* stream) {
  const std::string w("t2fit_sr_slice_forward_dev");
  if (!table_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": table_dev is NULL");
  if (reinterpret_cast<uintptr_t>(table_dev) & 7) return t2fit::fail(T2FIT_E_INVALID, w + ": table_dev is not aligned to 8 bytes");
  if (!out_dev && !N_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": out_dev and N_dev are both NULL");
  if ((x_dev == nullptr) != (out_dev == nullptr))
    return t2fit::fail(T2FIT_E_INVALID, w + ": x_dev and out_dev go together (both NULL: the weights only)");
  if (y_dev && !out_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": y_dev needs x_dev and out_dev");
  if (count_voxels(n_vol, hz, hy, hx) < 0 || count_voxels(n_vol, lz, ly, lx) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": n_vol and the sizes must all be >= 1 and a volume at most 2^40 elements");
  const int rc = profile_check(w, profile, thickness);
  if (rc != T2FIT_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(x_dev) & 3) || (reinterpret_cast<uintptr_t>(y_dev) & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 3) ||
      (reinterpret_cast<uintptr_t>(N_dev) & 7))
    return t2fit::fail(T2FIT_E_INVALID, w + ": x_dev / y_dev / out_dev is not aligned to 4 bytes or N_dev not to 8");
  if (out_dev && out_dev == x_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": out_dev must not be x_dev");
  SrSliceForwardArgs a;
  a.x = x_dev, a.y = y_dev, a.mask = mask_dev, a.out = out_dev, a.N = N_dev;
  a.table = static_cast<const SrSliceRec*>(table_dev);
  a.h = Dims{hz, hy, hx}, a.l = Dims{lz, ly, lx};
  a.profile = profile, a.n_vol = n_vol;
  double hw;
  profile_params(profile, thickness, &a.par, &hw);
  const int64_t plane_blocks = ((int64_t)ly * lx + kBlock - 1) / kBlock;
  if (plane_blocks * lz > INT32_MAX) return t2fit::fail(T2FIT_E_INVALID, w + ": a stack has more than 2^39 elements");
  a.plane_blocks = (int)plane_blocks;
  const dim3 grid((unsigned)(plane_blocks * lz), (unsigned)(((x_dev ? n_vol : 1) + kSrChunk - 1) / kSrChunk));
  hipLaunchKernelGGL(sr_slice_forward_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_sr_slice_adjoint_dev(int n_stacks, const float* const* r_dev, const double* const* N_dev, const uint8_t* const* mask_dev,
                               const void* const* table_dev, const int32_t* lo_size, const int32_t* profile, const double* thickness,
                               const float* x_dev, double tau, float* out_dev, int hz, int hy, int hx, int n_vol, void* stream) {
  const std::string w("t2fit_sr_slice_adjoint_dev");
  if (!r_dev || !N_dev || !table_dev || !lo_size || !profile || !thickness || !out_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": r_dev / N_dev / table_dev / lo_size / profile / thickness / out_dev is NULL");
  if (n_stacks < 1 || n_stacks > T2FIT_SR_MAX_STACKS)
    return t2fit::fail(T2FIT_E_INVALID, w + ": n_stacks must be 1 .. T2FIT_SR_MAX_STACKS");
  if (count_voxels(n_vol, hz, hy, hx) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": n_vol and the sizes must all be >= 1 and a volume at most 2^40 elements");
  if (!std::isfinite(tau)) return t2fit::fail(T2FIT_E_INVALID, w + ": tau is not finite");
  if ((reinterpret_cast<uintptr_t>(x_dev) & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 3))
    return t2fit::fail(T2FIT_E_INVALID, w + ": x_dev / out_dev is not aligned to 4 bytes");
  SrSliceAdjointArgs a = {};
  for (int s = 0; s < n_stacks; ++s) {
    SrSliceStack& k = a.s[s];
    if (!r_dev[s] || !N_dev[s]) return t2fit::fail(T2FIT_E_INVALID, w + ": a residual or normaliser pointer is NULL");
    if (!table_dev[s]) return t2fit::fail(T2FIT_E_INVALID, w + ": a slice table pointer is NULL");
    if (reinterpret_cast<uintptr_t>(table_dev[s]) & 7) return t2fit::fail(T2FIT_E_INVALID, w + ": a slice table is not aligned to 8 bytes");
    if ((reinterpret_cast<uintptr_t>(r_dev[s]) & 3) || (reinterpret_cast<uintptr_t>(N_dev[s]) & 7) || r_dev[s] == out_dev)
      return t2fit::fail(T2FIT_E_INVALID, w + ": a residual is not aligned to 4 bytes or is out_dev, or a normaliser not to 8");
    if (count_voxels(n_vol, lo_size[3 * s], lo_size[3 * s + 1], lo_size[3 * s + 2]) < 0)
      return t2fit::fail(T2FIT_E_INVALID, w + ": n_vol and the sizes must all be >= 1 and a stack at most 2^40 elements");
    const int rc = profile_check(w, profile[s], thickness[s]);
    if (rc != T2FIT_OK) return rc;
    k.r = r_dev[s], k.N = N_dev[s], k.mask = mask_dev ? mask_dev[s] : nullptr;
    k.table = static_cast<const SrSliceRec*>(table_dev[s]);
    k.l = Dims{lo_size[3 * s], lo_size[3 * s + 1], lo_size[3 * s + 2]};
    k.profile = profile[s];
    profile_params(profile[s], thickness[s], &k.par, &k.hw);
    if (!(k.hw < kMaxReach)) return t2fit::fail(T2FIT_E_INVALID, w + ": thickness is beyond 2^20 slice spacings");
  }
  a.x = x_dev, a.out = out_dev, a.h = Dims{hz, hy, hx}, a.n_stacks = n_stacks, a.tau = tau, a.n_vol = n_vol;
  a.tiles_x = (hx + kTileX - 1) / kTileX, a.tiles_y = (hy + kTileY - 1) / kTileY;
  const int64_t tiles = (int64_t)a.tiles_x * a.tiles_y * ((hz + kTileZ - 1) / kTileZ);
  if (tiles > INT32_MAX) return t2fit::fail(T2FIT_E_INVALID, w + ": a volume has more than 2^39 elements");
  const dim3 grid((unsigned)tiles, (unsigned)((n_vol + kSrChunk - 1) / kSrChunk));
  hipLaunchKernelGGL(sr_slice_adjoint_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

}  // extern "C"

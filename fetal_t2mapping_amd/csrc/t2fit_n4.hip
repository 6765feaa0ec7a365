// t2fit_n4.hip -- gfx950 kernels and C ABI of the N4 bias-field correction's device half (include/t2fit.h:
// t2fit_n4_workspace_bytes, t2fit_n4_log_dev, t2fit_n4_minmax_dev, t2fit_n4_histogram_dev, t2fit_n4_weights_dev,
// t2fit_n4_fit_dev, t2fit_n4_field_dev, t2fit_n4_apply_dev).  Stands for sitk.N4BiasFieldCorrectionImageFilter inside the
// reference's run_biasfield_correction / run_biasfield_correction2 (utils/qmri_utils.py:254-357).  The sharpening table,
// the lattice refinement, the convergence figure and the loop stay on the host (fetal_t2mapping_amd/_bias.py, which also
// states every kernel here in numpy).
//
//   n4_log_kernel       M = mask and in > 0; u0 = (float)log((double)in) in M, +0.0 elsewhere.
//   n4_minmax_kernel    min and max of u over M per workgroup (grid-stride), n4_minmax_final_kernel over the partials.
//   n4_hist_kernel      a uint64 histogram per workgroup in LDS (integer LDS atomics), then one integer atomic per
//                       non-empty bin to global memory.  Integer adds are exact in any order.
//   n4_axis_kernel      per axis and voxel index: the first lattice node k and the weights b (t2fit_bspline.h, shared with
//                       t2fit_ffd.hip), a = b^3 / S, q = b^2.
//   n4_rows_kernel      THE HOT ONE.  A wave per row (z, y): reads u and M once, forms the residual from the table E in
//                       LDS and contracts x: lane l adds terms l, l + 64, .. from +0.0 into C accumulators (C = the
//                       lattice side, a template argument: the four weights of a voxel are selected into place, there
//                       is no indexed register array and no scratch), then C xor butterflies (32 .. 1).  <kOmega>: the
//                       term is q alone (the mask's weight).
//   n4_y_kernel, n4_z_kernel   the y and z contractions in index order from +0.0, a thread per output; the z kernel ends
//                       with omega = the sum, or with delta = the sum and lattice += delta / omega.
//   n4_field_kernel     a workgroup per slice z and four rows: T1[z] (C x C) and the rows' T2 (C) in LDS, a wave per row;
//                       writes the new field and u, the row's sum d and sum d^2 (d = expm1(new - old) over M, same lane
//                       order and butterfly) and the row's min and max of the new u.
//   tree_reduce_kernel  (t2fit_reduce.h) a pass of the tree over the rows: 256 consecutive values by halving in LDS.
//   n4_apply_kernel     out = (float)((double)in / exp((double)field) * scale).
// No floating-point atomics; the order of every floating-point addition is a function of the sizes alone.  Compiled with
// -ffp-contract=off: every multiply and add rounds once, as numpy's do.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "t2fit_bspline.h"
#include "t2fit_error.h"
#include "t2fit_mattes.h"
#include "t2fit_reduce.h"
#include "t2fit_support.h"

namespace {

using t2fit::align_up, t2fit::ceil_div, t2fit::kBlock, t2fit::misaligned, t2fit::check_workspace;
using t2fit::bspline_node, t2fit::bspline_weights, t2fit::select_tap, t2fit::zero_u64_kernel;
using t2fit::wave_butterfly, t2fit::TreePasses, t2fit::tree_plan, t2fit::tree_launch;

constexpr int kWaves = kBlock / 64;  // rows a workgroup takes
constexpr size_t kAlign = 256;
constexpr const char* kBytesFn = "t2fit_n4_workspace_bytes";  // what reports the workspace every entry point here takes
constexpr int kMaxBins = 1024;
constexpr int kMaxSide = 19;
constexpr int kMaxGrid = 1024;       // workgroups of the grid-stride kernels (min/max, histogram)
constexpr int kTab = 12;             // doubles per voxel index of an axis table: b0..3, a0..3, q0..3
constexpr unsigned long long kFix = 1ull << 24;

__global__ __launch_bounds__(kBlock) void n4_log_kernel(const float* __restrict__ in, const uint8_t* __restrict__ mask, int64_t n,
                                                        float* __restrict__ u0, uint8_t* __restrict__ m) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n) return;
  const float x = in[v];
  const bool on = (mask == nullptr || mask[v] != 0) && x > 0.0f;
  m[v] = on ? 1 : 0;
  u0[v] = on ? (float)log((double)x) : 0.0f;
}

__global__ __launch_bounds__(kBlock) void n4_minmax_kernel(const float* __restrict__ u, const uint8_t* __restrict__ m, int64_t n,
                                                           float* __restrict__ mins, float* __restrict__ maxs) {
  __shared__ float lo_s[kBlock], hi_s[kBlock];
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock)
    if (m[v] != 0) {
      const float x = u[v];
      lo = x < lo ? x : lo;
      hi = x > hi ? x : hi;
    }
  lo_s[threadIdx.x] = lo, hi_s[threadIdx.x] = hi;
  __syncthreads();
  for (int h = kBlock / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) {
      lo_s[threadIdx.x] = lo_s[threadIdx.x + h] < lo_s[threadIdx.x] ? lo_s[threadIdx.x + h] : lo_s[threadIdx.x];
      hi_s[threadIdx.x] = hi_s[threadIdx.x + h] > hi_s[threadIdx.x] ? hi_s[threadIdx.x + h] : hi_s[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) mins[blockIdx.x] = lo_s[0], maxs[blockIdx.x] = hi_s[0];
}

// one workgroup: out[0] = min of mins[0..n), out[1] = max of maxs[0..n)
__global__ __launch_bounds__(kBlock) void n4_minmax_final_kernel(const float* __restrict__ mins, const float* __restrict__ maxs, int64_t n,
                                                                 float* __restrict__ out) {
  __shared__ float lo_s[kBlock], hi_s[kBlock];
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t v = threadIdx.x; v < n; v += kBlock) {
    lo = mins[v] < lo ? mins[v] : lo;
    hi = maxs[v] > hi ? maxs[v] : hi;
  }
  lo_s[threadIdx.x] = lo, hi_s[threadIdx.x] = hi;
  __syncthreads();
  for (int h = kBlock / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) {
      lo_s[threadIdx.x] = lo_s[threadIdx.x + h] < lo_s[threadIdx.x] ? lo_s[threadIdx.x + h] : lo_s[threadIdx.x];
      hi_s[threadIdx.x] = hi_s[threadIdx.x + h] > hi_s[threadIdx.x] ? hi_s[threadIdx.x + h] : hi_s[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = lo_s[0], out[1] = hi_s[0];
}

// the bin coordinate of a sample: i in 0 .. bins - 2 and t in [0, 1]
__device__ inline void bin_coord(float u, double lo, double slope, int bins, int& i, double& t) {
  double c = ((double)u - lo) / slope;
  const double top = (double)(bins - 1);
  c = c > 0.0 ? c : 0.0;
  c = c < top ? c : top;
  double f = floor(c);
  f = f < top - 1.0 ? f : top - 1.0;
  i = (int)f;
  t = c - f;
}

__global__ __launch_bounds__(kBlock) void n4_hist_kernel(const float* __restrict__ u, const uint8_t* __restrict__ m, int64_t n, double lo,
                                                         double slope, int bins, unsigned long long* __restrict__ hist) {
  __shared__ unsigned long long h[kMaxBins];
  for (int b = threadIdx.x; b < bins; b += kBlock) h[b] = 0ull;
  __syncthreads();
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock)
    if (m[v] != 0) {
      int i;
      double t;
      bin_coord(u[v], lo, slope, bins, i, t);
      const unsigned long long w = (unsigned long long)floor(t * (double)kFix + 0.5);
      atomicAdd(&h[i], kFix - w);
      atomicAdd(&h[i + 1], w);
    }
  __syncthreads();
  for (int b = threadIdx.x; b < bins; b += kBlock)
    if (h[b] != 0ull) atomicAdd(&hist[b], h[b]);
}

// ---- the lattice ---------------------------------------------------------------------------------------------------------
struct Axes {        // the three axis tables, z then y then x, in one run of the workspace
  const int* k;      // [nz + ny + nx]
  const double* w;   // [nz + ny + nx][kTab]
  int nz, ny, nx;
};

__global__ __launch_bounds__(kBlock) void n4_axis_kernel(int nz, int ny, int nx, int side, int* __restrict__ k_out, double* __restrict__ w_out) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= nz + ny + nx) return;
  const int n = v < nz ? nz : (v < nz + ny ? ny : nx);
  const int i = v < nz ? v : (v < nz + ny ? v - nz : v - nz - ny);
  double kf, tau, b[4];
  bspline_node(i, n, side, kf, tau);
  bspline_weights(tau, b);
  double q[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = b[j] * b[j];
  const double ssq = ((q[0] + q[1]) + q[2]) + q[3];
  k_out[v] = (int)kf;
  double* w = w_out + (int64_t)v * kTab;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    w[j] = b[j];
    w[4 + j] = (q[j] * b[j]) / ssq;
    w[8 + j] = q[j];
  }
}

struct RowsArgs {
  const float* u;
  const uint8_t* m;
  const double* table;  // NULL: the residual is u itself
  double lo, slope;
  int bins;
  Axes ax;
  int64_t rows;         // nz * ny
  double* xs;           // [rows][C]
};

template <int C, bool kOmega>
__global__ __launch_bounds__(kBlock) void n4_rows_kernel(const RowsArgs a) {
  __shared__ double e_s[kOmega ? 1 : kMaxBins];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool sharpen = !kOmega && a.table != nullptr;
  if (sharpen) {
    for (int b = threadIdx.x; b < a.bins; b += kBlock) e_s[b] = a.table[b];
    __syncthreads();
  }
  const int64_t row = (int64_t)blockIdx.x * kWaves + wave;
  if (row >= a.rows) return;  // (the whole wave)
  const int nx = a.ax.nx;
  const int* kx = a.ax.k + a.ax.nz + a.ax.ny;
  const double* wx = a.ax.w + (int64_t)(a.ax.nz + a.ax.ny) * kTab + (kOmega ? 8 : 4);
  const float* u = a.u + row * nx;
  const uint8_t* m = a.m + row * nx;
  double acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0;
#pragma unroll 1
  for (int x = lane; x < nx; x += 64) {
    if (m[x] == 0) continue;  // the term is +0.0
    double r = 1.0;
    if (!kOmega) {
      r = (double)u[x];
      if (sharpen) {
        int i;
        double t;
        bin_coord(u[x], a.lo, a.slope, a.bins, i, t);
        r = r - (e_s[i] * (1.0 - t) + e_s[i + 1] * t);
      }
    }
    const int k = kx[x];
    const double* w = wx + (int64_t)x * kTab;
    const double w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      acc[c] = acc[c] + select_tap(c - k, w0, w1, w2, w3) * r;
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double s = wave_butterfly(acc[c]);
    if (lane == 0) a.xs[row * C + c] = s;
  }
}

// ys[z][cy][cx] = sum over y, in order from +0.0, of w_y[cy] xs[z][y][cx]; off = 4 (a) or 8 (q)
__global__ __launch_bounds__(kBlock) void n4_y_kernel(const double* __restrict__ xs, Axes ax, int side, int off, double* __restrict__ ys) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= (int64_t)ax.nz * side * side) return;
  const int cx = (int)(v % side), cy = (int)((v / side) % side);
  const int64_t z = v / ((int64_t)side * side);
  const int* ky = ax.k + ax.nz;
  const double* wy = ax.w + (int64_t)ax.nz * kTab + off;
  double acc = 0.0;
  for (int y = 0; y < ax.ny; ++y) {
    const int d = cy - ky[y];
    if (d >= 0 && d < 4) acc = acc + wy[(int64_t)y * kTab + d] * xs[(z * ax.ny + y) * side + cx];
  }
  ys[v] = acc;
}

// the z contraction; omega_out: omega = the sum.  Else delta = the sum and lattice += delta / omega (0 where omega is 0)
__global__ __launch_bounds__(kBlock) void n4_z_kernel(const double* __restrict__ ys, Axes ax, int side, int off, double* __restrict__ omega_out,
                                                      const double* __restrict__ omega, double* __restrict__ delta,
                                                      double* __restrict__ lattice) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= side * side * side) return;
  const int rest = v % (side * side), cz = v / (side * side);
  const double* wz = ax.w + off;
  double acc = 0.0;
  for (int z = 0; z < ax.nz; ++z) {
    const int d = cz - ax.k[z];
    if (d >= 0 && d < 4) acc = acc + wz[(int64_t)z * kTab + d] * ys[(int64_t)z * side * side + rest];
  }
  if (omega_out) {
    omega_out[v] = acc;
    return;
  }
  delta[v] = acc;
  const double om = omega[v];
  lattice[v] = lattice[v] + (om != 0.0 ? acc / om : 0.0);
}

struct FieldArgs {
  const double* lattice;
  int side;
  const float* u0;
  const uint8_t* m;
  Axes ax;
  int tiles_y;          // ceil(ny / kWaves)
  float* field;         // in: the old field, out: the new one (a voxel is read and written by one lane)
  float* u;
  double* row_sums;     // [2][rows]
  float* row_min;       // [rows]
  float* row_max;
  int64_t rows;
};

__global__ __launch_bounds__(kBlock) void n4_field_kernel(const FieldArgs a) {
  __shared__ double t1[kMaxSide * kMaxSide];
  __shared__ double t2[kWaves][kMaxSide + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = a.side, cc = c * c;
  const int z = blockIdx.x / a.tiles_y, y = (blockIdx.x % a.tiles_y) * kWaves + wave;
  {
    const int kz = a.ax.k[z];
    const double* bz = a.ax.w + (int64_t)z * kTab;
    const double* l = a.lattice + (int64_t)kz * cc;
    for (int i = threadIdx.x; i < cc; i += kBlock)
      t1[i] = ((bz[0] * l[i] + bz[1] * l[cc + i]) + bz[2] * l[2 * cc + i]) + bz[3] * l[3 * cc + i];
  }
  __syncthreads();
  const bool valid = y < a.ax.ny;
  if (valid && lane < c) {
    const int ky = a.ax.k[a.ax.nz + y];
    const double* by = a.ax.w + (int64_t)(a.ax.nz + y) * kTab;
    const double* p = t1 + ky * c + lane;
    t2[wave][lane] = ((by[0] * p[0] + by[1] * p[c]) + by[2] * p[2 * c]) + by[3] * p[3 * c];
  }
  __syncthreads();
  if (!valid) return;  // (the whole wave)
  const int nx = a.ax.nx;
  const int64_t row = (int64_t)z * a.ax.ny + y;
  const int* kx = a.ax.k + a.ax.nz + a.ax.ny;
  const double* bx = a.ax.w + (int64_t)(a.ax.nz + a.ax.ny) * kTab;
  double sd = 0.0, sdd = 0.0;
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll 1
  for (int x = lane; x < nx; x += 64) {
    const double* b = bx + (int64_t)x * kTab;
    const double* p = t2[wave] + kx[x];
    const float f = (float)(((b[0] * p[0] + b[1] * p[1]) + b[2] * p[2]) + b[3] * p[3]);
    const int64_t at = row * nx + x;
    const float old = a.field[at];
    a.field[at] = f;
    float un = 0.0f;
    if (a.m[at] != 0) {
      un = (float)((double)a.u0[at] - (double)f);
      const double d = expm1((double)f - (double)old);
      sd = sd + d;
      sdd = sdd + d * d;
      lo = un < lo ? un : lo;
      hi = un > hi ? un : hi;
    }
    a.u[at] = un;
  }
  sd = wave_butterfly(sd);
  sdd = wave_butterfly(sdd);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const float ol = __shfl_xor(lo, s, 64), oh = __shfl_xor(hi, s, 64);
    lo = ol < lo ? ol : lo;
    hi = oh > hi ? oh : hi;
  }
  if (lane == 0) {
    a.row_sums[row] = sd;
    a.row_sums[a.rows + row] = sdd;
    a.row_min[row] = lo;
    a.row_max[row] = hi;
  }
}

__global__ __launch_bounds__(kBlock) void n4_apply_kernel(const float* __restrict__ in, const float* __restrict__ field, int64_t n, double scale,
                                                          float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n) return;
  out[v] = (float)(((double)in[v] / exp((double)field[v])) * scale);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// The workspace of a volume and a lattice side: the parts every entry point finds at the same place.
struct Plan {
  int nz, ny, nx, side;
  int64_t rows, n_vox;
  size_t k_at, w_at, xs_at, ys_at, min_at, max_at;
  TreePasses tree;  // over the two row sums of the field kernel; pass_n[0] = rows
  size_t total;
};

bool side_ok(int side) { return side == 4 || side == 5 || side == 7 || side == 11 || side == 19; }

int make_plan(const std::string& w, int nz, int ny, int nx, int side, Plan* p) {
  if (nz < 1 || ny < 1 || nx < 1) return t2fit::fail(T2FIT_E_INVALID, w + ": the sizes must all be >= 1");
  if ((int64_t)nz + ny + nx > (1 << 30)) return t2fit::fail(T2FIT_E_INVALID, w + ": the sizes add up to more than 2^30");
  const int64_t rows = (int64_t)nz * ny;
  if (rows > INT32_MAX || rows * nx > ((int64_t)1 << 40))
    return t2fit::fail(T2FIT_E_INVALID, w + ": more than 2^31-1 rows or 2^40 elements");
  if (!side_ok(side)) return t2fit::fail(T2FIT_E_INVALID, w + ": the lattice side is not one of 4, 5, 7, 11, 19");
  p->nz = nz, p->ny = ny, p->nx = nx, p->side = side, p->rows = rows, p->n_vox = rows * nx;
  const size_t n_axis = (size_t)nz + ny + nx;
  size_t at = 0;
  auto take = [&at](size_t bytes) {
    const size_t here = at;
    at += align_up(bytes, kAlign);
    return here;
  };
  p->k_at = take(n_axis * sizeof(int));
  p->w_at = take(n_axis * kTab * sizeof(double));
  p->xs_at = take((size_t)rows * side * sizeof(double));
  p->ys_at = take((size_t)nz * side * side * sizeof(double));
  p->min_at = take((size_t)(rows > kMaxGrid ? rows : kMaxGrid) * sizeof(float));
  p->max_at = take((size_t)(rows > kMaxGrid ? rows : kMaxGrid) * sizeof(float));
  tree_plan(&p->tree, rows, [&](int64_t n) { return take((size_t)n * 2 * sizeof(double)); });
  p->total = at;
  return T2FIT_OK;
}

int check_count(const std::string& w, int64_t n_vox) {
  if (n_vox < 1 || n_vox >= ((int64_t)1 << 39)) return t2fit::fail(T2FIT_E_INVALID, w + ": n_vox is outside 1..2^39-1");
  return T2FIT_OK;
}

int check_bins(const std::string& w, double lo, double slope, int bins) {
  if (bins < 2 || bins > kMaxBins) return t2fit::fail(T2FIT_E_INVALID, w + ": bins is outside 2..1024");
  if (!std::isfinite(lo) || !std::isfinite(slope) || !(slope > 0.0)) return t2fit::fail(T2FIT_E_INVALID, w + ": lo / slope is not finite, or slope is not > 0");
  return T2FIT_OK;
}

unsigned stride_grid(int64_t n) {
  const int64_t g = ceil_div(n, (int64_t)kBlock * 8);
  return (unsigned)(g < 1 ? 1 : (g > kMaxGrid ? kMaxGrid : g));
}

Axes launch_axes(const Plan& p, char* ws, hipStream_t st) {
  int* k = reinterpret_cast<int*>(ws + p.k_at);
  double* wt = reinterpret_cast<double*>(ws + p.w_at);
  hipLaunchKernelGGL(n4_axis_kernel, dim3((unsigned)ceil_div(p.nz + p.ny + p.nx, kBlock)), dim3(kBlock), 0, st, p.nz, p.ny, p.nx, p.side, k, wt);
  return Axes{k, wt, p.nz, p.ny, p.nx};
}

template <bool kOmega>
void launch_rows(const RowsArgs& a, int side, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(a.rows, (int64_t)kWaves)), block(kBlock);
  switch (side) {
    case 4: hipLaunchKernelGGL(HIP_KERNEL_NAME(n4_rows_kernel<4, kOmega>), grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL(HIP_KERNEL_NAME(n4_rows_kernel<5, kOmega>), grid, block, 0, st, a); break;
    case 7: hipLaunchKernelGGL(HIP_KERNEL_NAME(n4_rows_kernel<7, kOmega>), grid, block, 0, st, a); break;
    case 11: hipLaunchKernelGGL(HIP_KERNEL_NAME(n4_rows_kernel<11, kOmega>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(n4_rows_kernel<19, kOmega>), grid, block, 0, st, a); break;
  }
}

// the x, y and z contractions; omega_out or (omega, delta, lattice) as n4_z_kernel takes them
void launch_contractions(const Plan& p, char* ws, RowsArgs a, bool is_omega, double* omega_out, const double* omega, double* delta,
                         double* lattice, hipStream_t st) {
  a.ax = launch_axes(p, ws, st);
  a.rows = p.rows;
  a.xs = reinterpret_cast<double*>(ws + p.xs_at);
  double* ys = reinterpret_cast<double*>(ws + p.ys_at);
  if (is_omega) launch_rows<true>(a, p.side, st); else launch_rows<false>(a, p.side, st);
  const int off = is_omega ? 8 : 4, c = p.side;
  hipLaunchKernelGGL(n4_y_kernel, dim3((unsigned)ceil_div((int64_t)p.nz * c * c, (int64_t)kBlock)), dim3(kBlock), 0, st, (const double*)a.xs, a.ax, c,
                     off, ys);
  hipLaunchKernelGGL(n4_z_kernel, dim3((unsigned)ceil_div(c * c * c, kBlock)), dim3(kBlock), 0, st, (const double*)ys, a.ax, c, off, omega_out, omega,
                     delta, lattice);
}

}  // namespace

extern "C" {

int t2fit_n4_workspace_bytes(int nz, int ny, int nx, int side, size_t* bytes) {
  if (!bytes) return t2fit::fail(T2FIT_E_INVALID, "t2fit_n4_workspace_bytes: bytes is NULL");
  Plan p;
  const int rc = make_plan("t2fit_n4_workspace_bytes", nz, ny, nx, side, &p);
  if (rc != T2FIT_OK) return rc;
  *bytes = p.total;
  return T2FIT_OK;
}

int t2fit_n4_log_dev(const float* in_dev, const uint8_t* mask_dev, int64_t n_vox, float* u0_dev, uint8_t* m_dev, void* stream) {
  const std::string w("t2fit_n4_log_dev");
  if (!in_dev || !u0_dev || !m_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": in_dev / u0_dev / m_dev is NULL");
  const int rc = check_count(w, n_vox);
  if (rc != T2FIT_OK) return rc;
  if (misaligned(in_dev, 4) || misaligned(u0_dev, 4)) return t2fit::fail(T2FIT_E_INVALID, w + ": in_dev / u0_dev is not aligned to 4 bytes");
  if (in_dev == u0_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": u0_dev must not be in_dev");
  hipLaunchKernelGGL(n4_log_kernel, dim3((unsigned)ceil_div(n_vox, (int64_t)kBlock)), dim3(kBlock), 0, (hipStream_t)stream, in_dev, mask_dev, n_vox,
                     u0_dev, m_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_n4_minmax_dev(const float* u_dev, const uint8_t* m_dev, int64_t n_vox, float* range_dev, void* workspace_dev, size_t workspace_bytes,
                        void* stream) {
  const std::string w("t2fit_n4_minmax_dev");
  if (!u_dev || !m_dev || !range_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": u_dev / m_dev / range_dev is NULL");
  int rc = check_count(w, n_vox);
  if (rc != T2FIT_OK) return rc;
  if (misaligned(u_dev, 4) || misaligned(range_dev, 4)) return t2fit::fail(T2FIT_E_INVALID, w + ": u_dev / range_dev is not aligned to 4 bytes");
  // the partials: kMaxGrid minima at the place of the row minima, kMaxGrid maxima 256-aligned after them
  const size_t part = align_up((size_t)kMaxGrid * sizeof(float), kAlign);
  if ((rc = check_workspace(w, workspace_dev, workspace_bytes, 2 * part, kBytesFn)) != T2FIT_OK) return rc;
  float* mins = static_cast<float*>(workspace_dev);
  float* maxs = reinterpret_cast<float*>(static_cast<char*>(workspace_dev) + part);
  const unsigned grid = stride_grid(n_vox);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(n4_minmax_kernel, dim3(grid), dim3(kBlock), 0, st, u_dev, m_dev, n_vox, mins, maxs);
  hipLaunchKernelGGL(n4_minmax_final_kernel, dim3(1), dim3(kBlock), 0, st, (const float*)mins, (const float*)maxs, (int64_t)grid, range_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_n4_histogram_dev(const float* u_dev, const uint8_t* m_dev, int64_t n_vox, double lo, double slope, int bins, uint64_t* hist_dev,
                           void* stream) {
  const std::string w("t2fit_n4_histogram_dev");
  if (!u_dev || !m_dev || !hist_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": u_dev / m_dev / hist_dev is NULL");
  int rc = check_count(w, n_vox);
  if (rc != T2FIT_OK) return rc;
  if ((rc = check_bins(w, lo, slope, bins)) != T2FIT_OK) return rc;
  if (misaligned(u_dev, 4)) return t2fit::fail(T2FIT_E_INVALID, w + ": u_dev is not aligned to 4 bytes");
  if (misaligned(hist_dev, 8)) return t2fit::fail(T2FIT_E_INVALID, w + ": hist_dev is not aligned to 8 bytes");
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(hist_dev);
  hipLaunchKernelGGL(zero_u64_kernel, dim3((unsigned)ceil_div(bins, kBlock)), dim3(kBlock), 0, st, hist, bins);
  hipLaunchKernelGGL(n4_hist_kernel, dim3(stride_grid(n_vox)), dim3(kBlock), 0, st, u_dev, m_dev, n_vox, lo, slope, bins, hist);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_n4_weights_dev(const uint8_t* m_dev, int nz, int ny, int nx, int side, double* omega_dev, void* workspace_dev, size_t workspace_bytes,
                         void* stream) {
  const std::string w("t2fit_n4_weights_dev");
  if (!m_dev || !omega_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": m_dev / omega_dev is NULL");
  Plan p;
  int rc = make_plan(w, nz, ny, nx, side, &p);
  if (rc != T2FIT_OK) return rc;
  if (misaligned(omega_dev, 8)) return t2fit::fail(T2FIT_E_INVALID, w + ": omega_dev is not aligned to 8 bytes");
  if ((rc = check_workspace(w, workspace_dev, workspace_bytes, p.total, kBytesFn)) != T2FIT_OK) return rc;
  RowsArgs a{};
  a.m = m_dev;
  launch_contractions(p, static_cast<char*>(workspace_dev), a, true, omega_dev, nullptr, nullptr, nullptr, (hipStream_t)stream);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_n4_fit_dev(const float* u_dev, const uint8_t* m_dev, int nz, int ny, int nx, const double* table_dev, double lo, double slope, int bins,
                     int side, const double* omega_dev, double* lattice_dev, double* delta_dev, void* workspace_dev, size_t workspace_bytes,
                     void* stream) {
  const std::string w("t2fit_n4_fit_dev");
  if (!u_dev || !m_dev || !omega_dev || !lattice_dev || !delta_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": u_dev / m_dev / omega_dev / lattice_dev / delta_dev is NULL");
  Plan p;
  int rc = make_plan(w, nz, ny, nx, side, &p);
  if (rc != T2FIT_OK) return rc;
  if (table_dev && (rc = check_bins(w, lo, slope, bins)) != T2FIT_OK) return rc;
  if (misaligned(u_dev, 4)) return t2fit::fail(T2FIT_E_INVALID, w + ": u_dev is not aligned to 4 bytes");
  if (misaligned(table_dev, 8) || misaligned(omega_dev, 8) || misaligned(lattice_dev, 8) || misaligned(delta_dev, 8))
    return t2fit::fail(T2FIT_E_INVALID, w + ": table_dev / omega_dev / lattice_dev / delta_dev is not aligned to 8 bytes");
  if (delta_dev == lattice_dev || delta_dev == omega_dev || lattice_dev == omega_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": omega_dev, lattice_dev and delta_dev must be three arrays");
  if ((rc = check_workspace(w, workspace_dev, workspace_bytes, p.total, kBytesFn)) != T2FIT_OK) return rc;
  RowsArgs a{};
  a.u = u_dev, a.m = m_dev, a.table = table_dev, a.lo = lo, a.slope = slope, a.bins = table_dev ? bins : 2;
  launch_contractions(p, static_cast<char*>(workspace_dev), a, false, nullptr, omega_dev, delta_dev, lattice_dev, (hipStream_t)stream);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_n4_field_dev(const double* lattice_dev, int side, const float* u0_dev, const uint8_t* m_dev, int nz, int ny, int nx, float* field_dev,
                       float* u_dev, double* sums_dev, float* range_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  const std::string w("t2fit_n4_field_dev");
  if (!lattice_dev || !u0_dev || !m_dev || !field_dev || !u_dev || !sums_dev || !range_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": lattice_dev / u0_dev / m_dev / field_dev / u_dev / sums_dev / range_dev is NULL");
  Plan p;
  int rc = make_plan(w, nz, ny, nx, side, &p);
  if (rc != T2FIT_OK) return rc;
  if (misaligned(u0_dev, 4) || misaligned(field_dev, 4) || misaligned(u_dev, 4) || misaligned(range_dev, 4))
    return t2fit::fail(T2FIT_E_INVALID, w + ": u0_dev / field_dev / u_dev / range_dev is not aligned to 4 bytes");
  if (misaligned(lattice_dev, 8) || misaligned(sums_dev, 8)) return t2fit::fail(T2FIT_E_INVALID, w + ": lattice_dev / sums_dev is not aligned to 8 bytes");
  if (field_dev == u_dev || field_dev == u0_dev || u_dev == u0_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": u0_dev, field_dev and u_dev must be three arrays");
  const int tiles_y = ceil_div(ny, kWaves);
  if ((int64_t)nz * tiles_y > INT32_MAX) return t2fit::fail(T2FIT_E_INVALID, w + ": more than 2^31-1 workgroups");
  if ((rc = check_workspace(w, workspace_dev, workspace_bytes, p.total, kBytesFn)) != T2FIT_OK) return rc;
  char* ws = static_cast<char*>(workspace_dev);
  hipStream_t st = (hipStream_t)stream;
  FieldArgs a;
  a.lattice = lattice_dev, a.side = side, a.u0 = u0_dev, a.m = m_dev;
  a.ax = launch_axes(p, ws, st);
  a.tiles_y = tiles_y, a.field = field_dev, a.u = u_dev;
  a.row_sums = reinterpret_cast<double*>(ws + p.tree.pass_at[0]);
  a.row_min = reinterpret_cast<float*>(ws + p.min_at), a.row_max = reinterpret_cast<float*>(ws + p.max_at);
  a.rows = p.rows;
  hipLaunchKernelGGL(n4_field_kernel, dim3((unsigned)(nz * tiles_y)), dim3(kBlock), 0, st, a);
  tree_launch(p.tree, 2, ws, sums_dev, st);
  hipLaunchKernelGGL(n4_minmax_final_kernel, dim3(1), dim3(kBlock), 0, st, (const float*)a.row_min, (const float*)a.row_max, p.rows, range_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_n4_apply_dev(const float* in_dev, const float* field_dev, int64_t n_vox, double scale, float* out_dev, void* stream) {
  const std::string w("t2fit_n4_apply_dev");
  if (!in_dev || !field_dev || !out_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": in_dev / field_dev / out_dev is NULL");
  const int rc = check_count(w, n_vox);
  if (rc != T2FIT_OK) return rc;
  if (!std::isfinite(scale)) return t2fit::fail(T2FIT_E_INVALID, w + ": scale is not finite");
  if (misaligned(in_dev, 4) || misaligned(field_dev, 4) || misaligned(out_dev, 4))
    return t2fit::fail(T2FIT_E_INVALID, w + ": in_dev / field_dev / out_dev is not aligned to 4 bytes");
  if (out_dev == field_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": out_dev must not be field_dev");
  hipLaunchKernelGGL(n4_apply_kernel, dim3((unsigned)ceil_div(n_vox, (int64_t)kBlock)), dim3(kBlock), 0, (hipStream_t)stream, in_dev, field_dev, n_vox,
                     scale, out_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

}  // extern "C"

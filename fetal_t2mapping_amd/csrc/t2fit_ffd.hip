// t2fit_ffd.hip -- gfx950 kernels and C ABI of the non-rigid alignment's device half (include/t2fit.h:
// t2fit_ffd_workspace_bytes, t2fit_ffd_joint_hist_dev, t2fit_ffd_gradient_dev, t2fit_ffd_warp_dev, t2fit_ffd_jacobian_dev):
// a cubic B-spline free-form deformation d(x) on top of an index affine A, c(x) = A (x + d(x), 1), under Mattes mutual
// information.  The reference has no non-rigid step; the metric arithmetic, the regulariser and the descent stay on the
// host (fetal_t2mapping_amd/_ffd.py, which also states every kernel here in numpy).
//
// Every kernel walks the fixed grid the same way: a workgroup owns one plane z and four rows y, a wave per row, lane l
// the voxels l, l + 64, ..  The lattice (3 c^3 doubles: 165 KB at side 19, more than the 160 KiB of LDS) stays in global
// memory and is read through L2; what a workgroup stages in LDS is the plane's z contraction T1 (3 c^2 doubles, 8.7 KB at
// side 19) and each row's y contraction T2 (3 c doubles), so a voxel pays four taps per component, not 64.
//   ffd_axis_kernel     per axis and voxel index: the first node k, the weights b and their index derivatives db.
//   ffd_hist_kernel     the joint histogram of t2fit_register_joint_hist_dev with c(x): a uint64 table per workgroup in
//                       LDS (integer LDS atomics), the workgroup strides over the tiles and adds its nonzero entries to
//                       global memory once (integer atomics: exact in any order).
//   ffd_rows_kernel     THE HOT ONE.  Per counted voxel the force f_j = ((s g_0) A[0][j] + (s g_1) A[1][j]) + (s g_2) A[2][j]
//                       (s from the table in LDS), contracted along x as t2fit_n4.hip's fit kernel does: lane l adds
//                       its terms in order from +0.0 into 3 C accumulators (C = the side, a template argument: selected
//                       weights, no indexed register array, no scratch), then 3 C xor butterflies.  A node outside the
//                       voxel's four gets +0.0, selected after the product, so nothing non-finite crosses a support.
//   ffd_y_kernel, ffd_z_kernel   the y and z contractions in index order from +0.0, a thread per output.
//   ffd_warp_kernel     the resampling sample of t2fit_affine.h (linear with the zero-weight skip, or nearest) at c(x).
//   ffd_jac_kernel      det(I + dd/dx) from the derivative weights, per row the minimum over the mask and the count of
//                       det <= 0; ffd_jac_final_kernel reduces the rows (minimum and count: exact in any order).
// What the affine stages compute at A (x, 1) is computed here at c(x) by the same functions, so a zero lattice gives their
// bytes: the metric's sample and the resampling sample (t2fit_affine.h), the Parzen window, the bin and the histogram
// deposit (t2fit_mattes.h).  The node and weights of a voxel index and the selected tap are t2fit_n4.hip's (t2fit_bspline.h).
// No floating-point atomics; the order of every floating-point addition is a function of the sizes alone.  Compiled with
// -ffp-contract=off: every multiply and add rounds once, as numpy's do.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "t2fit_affine.h"
#include "t2fit_bspline.h"
#include "t2fit_error.h"
#include "t2fit_mattes.h"
#include "t2fit_support.h"

namespace {

using t2fit::align_up, t2fit::ceil_div, t2fit::kBlock, t2fit::misaligned;
using t2fit::Affine, t2fit::Dims, t2fit::MemFetch, t2fit::sample_metric, t2fit::sample_linear, t2fit::sample_nearest;
using t2fit::bspline_node, t2fit::bspline_weights, t2fit::select_tap;
using t2fit::bin_of, t2fit::parzen, t2fit::deposit, t2fit::zero_u64_kernel, t2fit::wave_butterfly;

constexpr int kWaves = kBlock / 64;  // rows a workgroup takes
constexpr size_t kAlign = 256;
constexpr int kMaxSide = 19;
constexpr int kTab = 8;              // doubles per voxel index of an axis table: b0..3, db0..3
constexpr int kMaxBins = 64, kMinMovingBins = 5;
constexpr int kHistGrid = 2048;      // workgroups of the joint histogram at most: each flushes its table once
static_assert(3 * kMaxSide <= 64, "a lane per (component, node) of a row's T2");

struct Axes {        // the three axis tables, z then y then x, in one run of the workspace
  const int* k;      // [nz + ny + nx]
  const double* w;   // [nz + ny + nx][kTab]
  int nz, ny, nx;
};

struct Lat {
  const double* phi;  // [3][c][c][c]
  int side;
  Axes ax;
  int tiles_y;        // ceil(ny / kWaves)
  int n_tiles;        // nz * tiles_y
};

__global__ __launch_bounds__(kBlock) void ffd_axis_kernel(int nz, int ny, int nx, int side, int* __restrict__ k_out, double* __restrict__ w_out) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= nz + ny + nx) return;
  const int n = v < nz ? nz : (v < nz + ny ? ny : nx);
  const int i = v < nz ? v : (v < nz + ny ? v - nz : v - nz - ny);
  double kf, tau, scale = 0.0;  // scale: cells per voxel, d tau / d index
  if (n > 1) scale = (double)(side - 3) / (double)(n - 1);
  bspline_node(i, n, side, kf, tau);
  const double t2 = tau * tau, om = 1.0 - tau;
  k_out[v] = (int)kf;
  double* w = w_out + (int64_t)v * kTab;
  bspline_weights(tau, w);
  w[4] = (-((om * om) * 0.5)) * scale;
  w[5] = (1.5 * t2 - 2.0 * tau) * scale;
  w[6] = ((-1.5 * t2 + tau) + 0.5) * scale;
  w[7] = (t2 * 0.5) * scale;
}

// T1 of plane z: t1[comp][cy][cx] = sum_j bz_j phi[comp][kz + j][cy][cx], added in tap order; <true>: also t1d with dbz
template <bool kDeriv>
__device__ inline void stage_plane(const Lat& L, int z, double* t1, double* t1d) {
  const int c = L.side, cc = c * c;
  const int kz = L.ax.k[z];
  const double* wz = L.ax.w + (int64_t)z * kTab;
  for (int i = threadIdx.x; i < 3 * cc; i += kBlock) {
    const int comp = i / cc, r = i - comp * cc;
    const double* l = L.phi + ((int64_t)comp * c + kz) * cc + r;
    const double l0 = l[0], l1 = l[cc], l2 = l[2 * cc], l3 = l[3 * cc];
    t1[i] = ((wz[0] * l0 + wz[1] * l1) + wz[2] * l2) + wz[3] * l3;
    if (kDeriv) t1d[i] = ((wz[4] * l0 + wz[5] * l1) + wz[6] * l2) + wz[7] * l3;
  }
}

// T2 of row y (this wave's): t2[comp][cx] = sum_j w_j src[comp][ky + j][cx]; off 0: by, 4: dby
__device__ inline void stage_row(const Lat& L, int y, const double* src, int off, double (*t2)[kMaxSide + 1]) {
  const int lane = threadIdx.x & 63, c = L.side;
  if (lane >= 3 * c) return;
  const int comp = lane / c, cx = lane - comp * c;
  const int ky = L.ax.k[L.ax.nz + y];
  const double* wy = L.ax.w + (int64_t)(L.ax.nz + y) * kTab + off;
  const double* p = src + (comp * c + ky) * c + cx;
  t2[comp][cx] = ((wy[0] * p[0] + wy[1] * p[c]) + wy[2] * p[2 * c]) + wy[3] * p[3 * c];
}

__device__ inline double taps(const double* w, const double* p) { return ((w[0] * p[0] + w[1] * p[1]) + w[2] * p[2]) + w[3] * p[3]; }

// c(x) of the voxel (x, y, z) of a staged row
__device__ inline void deformed(const Lat& L, const Affine& A, const double (*t2)[kMaxSide + 1], int x, int y, int z, double* c) {
  const int kx = L.ax.k[L.ax.nz + L.ax.ny + x];
  const double* bx = L.ax.w + (int64_t)(L.ax.nz + L.ax.ny + x) * kTab;
  const double px = (double)x + taps(bx, t2[0] + kx), py = (double)y + taps(bx, t2[1] + kx), pz = (double)z + taps(bx, t2[2] + kx);
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = ((A.m[4 * a] * px + A.m[4 * a + 1] * py) + A.m[4 * a + 2] * pz) + A.m[4 * a + 3];
}

struct MetricArgs {
  Lat L;
  const uint8_t* bins;
  const double* table;       // the gradient: T[n_f][n_m]
  int n_f, n_m;
  double lo_m, scale_m;
  unsigned long long* hist;  // the histogram [n_f][n_m]
  const uint8_t* fixed_mask;
  const float* moving;
  const uint8_t* moving_mask;
  Dims m;
  Affine A;
  double* xs;                // the gradient: [rows][3][C]
};

__global__ __launch_bounds__(kBlock) void ffd_hist_kernel(const MetricArgs a) {
  __shared__ double t1[3 * kMaxSide * kMaxSide];
  __shared__ double t2[kWaves][3][kMaxSide + 1];
  extern __shared__ unsigned long long ffd_hist[];  // [n_f][n_m], the launch sizes it
  const int n_entries = a.n_f * a.n_m;
  for (int i = threadIdx.x; i < n_entries; i += kBlock) ffd_hist[i] = 0ull;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nx = a.L.ax.nx, ny = a.L.ax.ny;
  for (int tile = blockIdx.x; tile < a.L.n_tiles; tile += gridDim.x) {
    const int z = tile / a.L.tiles_y, y = (tile % a.L.tiles_y) * kWaves + wave;
    __syncthreads();  // (the rows of the tile before have left T1; the first time: the table is zero)
    stage_plane<false>(a.L, z, t1, nullptr);
    __syncthreads();
    const bool valid = y < ny;
    if (valid) stage_row(a.L, y, t1, 0, t2[wave]);
    __syncthreads();
    if (!valid) continue;
    const int64_t row = (int64_t)z * ny + y;
#pragma unroll 1
    for (int x = lane; x < nx; x += 64) {
      const int64_t at = row * nx + x;
      if (a.fixed_mask[at] == 0) continue;
      double c[3], m, w[4];
      deformed(a.L, a.A, t2[wave], x, y, z, c);
      if (!sample_metric<false>(a.moving, a.moving_mask, a.m, c[0], c[1], c[2], m, nullptr)) continue;
      const int i0 = parzen<false>(m, a.lo_m, a.scale_m, a.n_m, w);
      unsigned long long* hrow = ffd_hist + bin_of(a.bins[at], a.n_f) * a.n_m + (i0 - 1);
      deposit(hrow, w);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_entries; i += kBlock)
    if (ffd_hist[i] != 0ull) atomicAdd(&a.hist[i], ffd_hist[i]);
}

template <int C>
__global__ __launch_bounds__(kBlock) void ffd_rows_kernel(const MetricArgs a) {
  __shared__ double t1[3 * kMaxSide * kMaxSide];
  __shared__ double t2[kWaves][3][kMaxSide + 1];
  extern __shared__ double ffd_table[];  // [n_f][n_m], the launch sizes it
  for (int i = threadIdx.x; i < a.n_f * a.n_m; i += kBlock) ffd_table[i] = a.table[i];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nx = a.L.ax.nx, ny = a.L.ax.ny;
  const int z = blockIdx.x / a.L.tiles_y, y = (blockIdx.x % a.L.tiles_y) * kWaves + wave;
  stage_plane<false>(a.L, z, t1, nullptr);
  __syncthreads();
  const bool valid = y < ny;
  if (valid) stage_row(a.L, y, t1, 0, t2[wave]);
  __syncthreads();
  if (!valid) return;  // (the whole wave)
  const int64_t row = (int64_t)z * ny + y;
  const int* kx = a.L.ax.k + a.L.ax.nz + ny;
  const double* wx = a.L.ax.w + (int64_t)(a.L.ax.nz + ny) * kTab;
  double acc[3][C];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int c = 0; c < C; ++c) acc[j][c] = 0.0;
#pragma unroll 1
  for (int x = lane; x < nx; x += 64) {
    const int64_t at = row * nx + x;
    if (a.fixed_mask[at] == 0) continue;  // the term is +0.0
    double cc[3], m, g[3], dw[4];
    deformed(a.L, a.A, t2[wave], x, y, z, cc);
    if (!sample_metric<true>(a.moving, a.moving_mask, a.m, cc[0], cc[1], cc[2], m, g)) continue;
    const int i0 = parzen<true>(m, a.lo_m, a.scale_m, a.n_m, dw);
    const double* trow = ffd_table + bin_of(a.bins[at], a.n_f) * a.n_m + (i0 - 1);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) s = s + trow[j] * dw[j];
    const double sg0 = s * g[0], sg1 = s * g[1], sg2 = s * g[2];
    double f[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) f[j] = (sg0 * a.A.m[j] + sg1 * a.A.m[4 + j]) + sg2 * a.A.m[8 + j];
    const int k = kx[x];
    const double* w = wx + (int64_t)x * kTab;
    const double w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int d = c - k;
      const double wc = select_tap(d, w0, w1, w2, w3);
      const bool in = (unsigned)d < 4u;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double t = wc * f[j];
        acc[j][c] = acc[j][c] + (in ? t : 0.0);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double s = wave_butterfly(acc[j][c]);
      if (lane == 0) a.xs[(row * 3 + j) * C + c] = s;
    }
}

// ys[z][comp][cy][cx] = sum over y, in order from +0.0, of by[cy] xs[z][y][comp][cx]
__global__ __launch_bounds__(kBlock) void ffd_y_kernel(const double* __restrict__ xs, Axes ax, int side, double* __restrict__ ys) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= (int64_t)ax.nz * 3 * side * side) return;
  const int cx = (int)(v % side), cy = (int)((v / side) % side), comp = (int)((v / ((int64_t)side * side)) % 3);
  const int64_t z = v / ((int64_t)3 * side * side);
  const int* ky = ax.k + ax.nz;
  const double* wy = ax.w + (int64_t)ax.nz * kTab;
  double acc = 0.0;
  for (int y = 0; y < ax.ny; ++y) {
    const int d = cy - ky[y];
    if (d >= 0 && d < 4) acc = acc + wy[(int64_t)y * kTab + d] * xs[((z * ax.ny + y) * 3 + comp) * side + cx];
  }
  ys[v] = acc;
}

// out[comp][cz][cy][cx] = sum over z, in order from +0.0, of bz[cz] ys[z][comp][cy][cx]
__global__ __launch_bounds__(kBlock) void ffd_z_kernel(const double* __restrict__ ys, Axes ax, int side, double* __restrict__ out) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  const int cc = side * side;
  if (v >= 3 * cc * side) return;
  const int rest = v % cc, cz = (v / cc) % side, comp = v / (cc * side);
  double acc = 0.0;
  for (int z = 0; z < ax.nz; ++z) {
    const int d = cz - ax.k[z];
    if (d >= 0 && d < 4) acc = acc + ax.w[(int64_t)z * kTab + d] * ys[((int64_t)z * 3 + comp) * cc + rest];
  }
  out[v] = acc;
}

// ---- the warp: t2fit_affine.h's resampling sample at c(x) -------------------------------------------------------------
// the linear sample as a float32 (the warp has no integer pixel type); outside the volume, default_value
__device__ inline float warp_linear(const MemFetch& fetch, const Dims n, const double* c, float default_value) {
  double r;
  if (!sample_linear(fetch, n, c[0], c[1], c[2], r)) return default_value;
  return (float)r;
}

struct WarpArgs {
  Lat L;
  const uint32_t* src;
  uint32_t* out;
  Dims n;
  Affine A;
  int nearest;
  uint32_t default_bits;
};

__global__ __launch_bounds__(kBlock) void ffd_warp_kernel(const WarpArgs a) {
  __shared__ double t1[3 * kMaxSide * kMaxSide];
  __shared__ double t2[kWaves][3][kMaxSide + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nx = a.L.ax.nx, ny = a.L.ax.ny;
  const int z = blockIdx.x / a.L.tiles_y, y = (blockIdx.x % a.L.tiles_y) * kWaves + wave;
  stage_plane<false>(a.L, z, t1, nullptr);
  __syncthreads();
  const bool valid = y < ny;
  if (valid) stage_row(a.L, y, t1, 0, t2[wave]);
  __syncthreads();
  if (!valid) return;  // (the whole wave)
  const int64_t row = (int64_t)z * ny + y;
  const MemFetch fetch{reinterpret_cast<const float*>(a.src), a.n.ny, a.n.nx};
#pragma unroll 1
  for (int x = lane; x < nx; x += 64) {
    double c[3];
    deformed(a.L, a.A, t2[wave], x, y, z, c);
    a.out[row * nx + x] = a.nearest ? sample_nearest(a.src, a.n, c[0], c[1], c[2], a.default_bits)
                                    : __float_as_uint(warp_linear(fetch, a.n, c, __uint_as_float(a.default_bits)));
  }
}

// ---- the Jacobian ----------------------------------------------------------------------------------------------------------
struct JacArgs {
  Lat L;
  const uint8_t* mask;
  double* row_min;               // [rows]
  unsigned long long* row_cnt;   // [rows]
};

__global__ __launch_bounds__(kBlock) void ffd_jac_kernel(const JacArgs a) {
  __shared__ double t1[3 * kMaxSide * kMaxSide], t1d[3 * kMaxSide * kMaxSide];
  __shared__ double t2[kWaves][3][3][kMaxSide + 1];  // [wave][0: bz by, 1: bz dby, 2: dbz by][comp][cx]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nx = a.L.ax.nx, ny = a.L.ax.ny;
  const int z = blockIdx.x / a.L.tiles_y, y = (blockIdx.x % a.L.tiles_y) * kWaves + wave;
  stage_plane<true>(a.L, z, t1, t1d);
  __syncthreads();
  const bool valid = y < ny;
  if (valid) {
    stage_row(a.L, y, t1, 0, t2[wave][0]);
    stage_row(a.L, y, t1, 4, t2[wave][1]);
    stage_row(a.L, y, t1d, 0, t2[wave][2]);
  }
  __syncthreads();
  if (!valid) return;  // (the whole wave)
  const int64_t row = (int64_t)z * ny + y;
  const int* kx = a.L.ax.k + a.L.ax.nz + ny;
  const double* wx = a.L.ax.w + (int64_t)(a.L.ax.nz + ny) * kTab;
  double lo = INFINITY;
  unsigned long long folded = 0ull;
#pragma unroll 1
  for (int x = lane; x < nx; x += 64) {
    if (a.mask[row * nx + x] == 0) continue;
    const int k = kx[x];
    const double* w = wx + (int64_t)x * kTab;
    double j[3][3];  // j[comp][axis], axis 0 is x
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
      j[comp][0] = taps(w + 4, t2[wave][0][comp] + k);
      j[comp][1] = taps(w, t2[wave][1][comp] + k);
      j[comp][2] = taps(w, t2[wave][2][comp] + k);
      j[comp][comp] = 1.0 + j[comp][comp];
    }
    const double det = (j[0][0] * (j[1][1] * j[2][2] - j[1][2] * j[2][1]) - j[0][1] * (j[1][0] * j[2][2] - j[1][2] * j[2][0])) +
                       j[0][2] * (j[1][0] * j[2][1] - j[1][1] * j[2][0]);
    lo = det < lo ? det : lo;
    folded += det <= 0.0 ? 1ull : 0ull;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const double other = __shfl_xor(lo, s, 64);
    lo = other < lo ? other : lo;
    folded += (unsigned long long)__shfl_xor((long long)folded, s, 64);
  }
  if (lane == 0) a.row_min[row] = lo, a.row_cnt[row] = folded;
}

// one workgroup: the minimum and the total over the rows
__global__ __launch_bounds__(kBlock) void ffd_jac_final_kernel(const double* __restrict__ row_min, const unsigned long long* __restrict__ row_cnt,
                                                               int64_t rows, double* __restrict__ min_out, long long* __restrict__ count_out) {
  __shared__ double lo_s[kBlock];
  __shared__ unsigned long long n_s[kBlock];
  double lo = INFINITY;
  unsigned long long n = 0ull;
  for (int64_t r = threadIdx.x; r < rows; r += kBlock) {
    lo = row_min[r] < lo ? row_min[r] : lo;
    n += row_cnt[r];
  }
  lo_s[threadIdx.x] = lo, n_s[threadIdx.x] = n;
  __syncthreads();
  for (int h = kBlock / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) {
      lo_s[threadIdx.x] = lo_s[threadIdx.x + h] < lo_s[threadIdx.x] ? lo_s[threadIdx.x + h] : lo_s[threadIdx.x];
      n_s[threadIdx.x] += n_s[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *min_out = lo_s[0], *count_out = (long long)n_s[0];
}

// ---- host ----------------------------------------------------------------------------------------------------------------
struct Plan {
  int nz, ny, nx, side, tiles_y;
  int64_t rows;
  size_t k_at, w_at, xs_at, ys_at, min_at, cnt_at, total;
};

bool side_ok(int side) { return side == 4 || side == 5 || side == 7 || side == 11 || side == 19; }

int make_plan(const std::string& w, int nz, int ny, int nx, int side, Plan* p) {
  if (t2fit::count_voxels(1, nz, ny, nx) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the fixed sizes must all be >= 1 and the volume at most 2^40 elements");
  if (!side_ok(side)) return t2fit::fail(T2FIT_E_INVALID, w + ": the lattice side is not one of 4, 5, 7, 11, 19");
  if ((int64_t)nz + ny + nx > (1 << 30)) return t2fit::fail(T2FIT_E_INVALID, w + ": the fixed sizes add up to more than 2^30");
  p->nz = nz, p->ny = ny, p->nx = nx, p->side = side, p->tiles_y = ceil_div(ny, kWaves);
  p->rows = (int64_t)nz * ny;
  if ((int64_t)nz * p->tiles_y > INT32_MAX || (int64_t)nz * 3 * side * side > ((int64_t)1 << 38))
    return t2fit::fail(T2FIT_E_INVALID, w + ": the fixed volume has more than 2^31-1 tiles of four rows (the launch index is 32-bit)");
  const size_t n_axis = (size_t)nz + ny + nx;
  size_t at = 0;
  auto take = [&at](size_t bytes) {
    const size_t here = at;
    at += align_up(bytes, kAlign);
    return here;
  };
  p->k_at = take(n_axis * sizeof(int));
  p->w_at = take(n_axis * kTab * sizeof(double));
  p->xs_at = take((size_t)p->rows * 3 * side * sizeof(double));
  p->ys_at = take((size_t)nz * 3 * side * side * sizeof(double));
  p->min_at = take((size_t)p->rows * sizeof(double));
  p->cnt_at = take((size_t)p->rows * sizeof(unsigned long long));
  p->total = at;
  return T2FIT_OK;
}

// the lattice and the workspace: what every entry point checks after its own NULL checks and the plan
int check_common(const std::string& w, const double* lattice_dev, const void* ws, size_t bytes, const Plan& p) {
  if (misaligned(lattice_dev, 8)) return t2fit::fail(T2FIT_E_INVALID, w + ": lattice_dev is not aligned to 8 bytes");
  return t2fit::check_workspace(w, ws, bytes, p.total, "t2fit_ffd_workspace_bytes");
}

int check_metric(const std::string& w, int n_f, int n_m, double lo_m, double scale_m, const float* moving_dev, int mz, int my, int mx,
                 const double* A) {
  if (n_f < 1 || n_f > kMaxBins) return t2fit::fail(T2FIT_E_INVALID, w + ": n_f is outside 1..64");
  if (n_m < kMinMovingBins || n_m > kMaxBins) return t2fit::fail(T2FIT_E_INVALID, w + ": n_m is outside 5..64");
  if (!std::isfinite(lo_m) || !std::isfinite(scale_m)) return t2fit::fail(T2FIT_E_INVALID, w + ": lo_m / scale_m is not finite");
  if (t2fit::count_voxels(1, mz, my, mx) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the moving sizes must all be >= 1 and the volume at most 2^40 elements");
  if (!t2fit::finite12(A)) return t2fit::fail(T2FIT_E_INVALID, w + ": A has a non-finite entry");
  if (misaligned(moving_dev, 4)) return t2fit::fail(T2FIT_E_INVALID, w + ": moving_dev is not aligned to 4 bytes");
  return T2FIT_OK;
}

Lat launch_axes(const Plan& p, const double* lattice_dev, char* ws, hipStream_t st) {
  int* k = reinterpret_cast<int*>(ws + p.k_at);
  double* wt = reinterpret_cast<double*>(ws + p.w_at);
  hipLaunchKernelGGL(ffd_axis_kernel, dim3((unsigned)ceil_div(p.nz + p.ny + p.nx, kBlock)), dim3(kBlock), 0, st, p.nz, p.ny, p.nx, p.side, k, wt);
  return Lat{lattice_dev, p.side, Axes{k, wt, p.nz, p.ny, p.nx}, p.tiles_y, p.nz * p.tiles_y};
}

void launch_rows(const MetricArgs& a, size_t lds, hipStream_t st) {
  const dim3 grid((unsigned)a.L.n_tiles), block(kBlock);
  switch (a.L.side) {
    case 4: hipLaunchKernelGGL(HIP_KERNEL_NAME(ffd_rows_kernel<4>), grid, block, lds, st, a); break;
    case 5: hipLaunchKernelGGL(HIP_KERNEL_NAME(ffd_rows_kernel<5>), grid, block, lds, st, a); break;
    case 7: hipLaunchKernelGGL(HIP_KERNEL_NAME(ffd_rows_kernel<7>), grid, block, lds, st, a); break;
    case 11: hipLaunchKernelGGL(HIP_KERNEL_NAME(ffd_rows_kernel<11>), grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(ffd_rows_kernel<19>), grid, block, lds, st, a); break;
  }
}

MetricArgs metric_args(const Lat& L, const uint8_t* bins_dev, int n_f, int n_m, double lo_m, double scale_m, const uint8_t* fixed_mask_dev,
                       const float* moving_dev, const uint8_t* moving_mask_dev, int mz, int my, int mx, const double* A) {
  MetricArgs a;
  a.L = L, a.bins = bins_dev, a.table = nullptr, a.n_f = n_f, a.n_m = n_m, a.lo_m = lo_m, a.scale_m = scale_m, a.hist = nullptr;
  a.fixed_mask = fixed_mask_dev, a.moving = moving_dev, a.moving_mask = moving_mask_dev, a.m = Dims{mz, my, mx}, a.xs = nullptr;
  for (int i = 0; i < 12; ++i) a.A.m[i] = A[i];
  return a;
}

}  // namespace

extern "C" {

int t2fit_ffd_workspace_bytes(int fz, int fy, int fx, int side, size_t* bytes) {
  if (!bytes) return t2fit::fail(T2FIT_E_INVALID, "t2fit_ffd_workspace_bytes: bytes is NULL");
  Plan p;
  const int rc = make_plan("t2fit_ffd_workspace_bytes", fz, fy, fx, side, &p);
  if (rc != T2FIT_OK) return rc;
  *bytes = p.total;
  return T2FIT_OK;
}

int t2fit_ffd_joint_hist_dev(const uint8_t* bins_dev, const uint8_t* fixed_mask_dev, int fz, int fy, int fx, const float* moving_dev,
                             const uint8_t* moving_mask_dev, int mz, int my, int mx, const double* A, const double* lattice_dev, int side,
                             int n_f, int n_m, double lo_m, double scale_m, uint64_t* hist_dev, void* workspace_dev, size_t workspace_bytes,
                             void* stream) {
  const std::string w("t2fit_ffd_joint_hist_dev");
  if (!bins_dev || !fixed_mask_dev || !moving_dev || !moving_mask_dev || !A || !lattice_dev || !hist_dev || !workspace_dev)
    return t2fit::fail(T2FIT_E_INVALID,
                       w + ": bins_dev / fixed_mask_dev / moving_dev / moving_mask_dev / A / lattice_dev / hist_dev / workspace_dev is NULL");
  Plan p;
  int rc = make_plan(w, fz, fy, fx, side, &p);
  if (rc != T2FIT_OK) return rc;
  if ((rc = check_metric(w, n_f, n_m, lo_m, scale_m, moving_dev, mz, my, mx, A)) != T2FIT_OK) return rc;
  if ((int64_t)fz * fy * fx > ((int64_t)1 << 32))
    return t2fit::fail(T2FIT_E_INVALID, w + ": the fixed volume has more than 2^32 voxels (a histogram entry could pass 2^63)");
  if (misaligned(hist_dev, 8)) return t2fit::fail(T2FIT_E_INVALID, w + ": hist_dev is not aligned to 8 bytes");
  if ((rc = check_common(w, lattice_dev, workspace_dev, workspace_bytes, p)) != T2FIT_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  MetricArgs a = metric_args(launch_axes(p, lattice_dev, static_cast<char*>(workspace_dev), st), bins_dev, n_f, n_m, lo_m, scale_m,
                             fixed_mask_dev, moving_dev, moving_mask_dev, mz, my, mx, A);
  a.hist = reinterpret_cast<unsigned long long*>(hist_dev);
  const int n_entries = n_f * n_m;
  const unsigned grid = (unsigned)(a.L.n_tiles < kHistGrid ? a.L.n_tiles : kHistGrid);
  hipLaunchKernelGGL(zero_u64_kernel, dim3((unsigned)ceil_div(n_entries, kBlock)), dim3(kBlock), 0, st, a.hist, n_entries);
  hipLaunchKernelGGL(ffd_hist_kernel, dim3(grid), dim3(kBlock), (size_t)n_entries * sizeof(unsigned long long), st, a);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_ffd_gradient_dev(const uint8_t* bins_dev, const double* table_dev, int n_f, int n_m, double lo_m, double scale_m,
                           const uint8_t* fixed_mask_dev, int fz, int fy, int fx, const float* moving_dev, const uint8_t* moving_mask_dev,
                           int mz, int my, int mx, const double* A, const double* lattice_dev, int side, double* grad_dev, void* workspace_dev,
                           size_t workspace_bytes, void* stream) {
  const std::string w("t2fit_ffd_gradient_dev");
  if (!bins_dev || !table_dev || !fixed_mask_dev || !moving_dev || !moving_mask_dev || !A || !lattice_dev || !grad_dev || !workspace_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": bins_dev / table_dev / fixed_mask_dev / moving_dev / moving_mask_dev / A / lattice_dev / grad_dev / "
                                            "workspace_dev is NULL");
  Plan p;
  int rc = make_plan(w, fz, fy, fx, side, &p);
  if (rc != T2FIT_OK) return rc;
  if ((rc = check_metric(w, n_f, n_m, lo_m, scale_m, moving_dev, mz, my, mx, A)) != T2FIT_OK) return rc;
  if (misaligned(grad_dev, 8) || misaligned(table_dev, 8))
    return t2fit::fail(T2FIT_E_INVALID, w + ": grad_dev / table_dev is not aligned to 8 bytes");
  if (grad_dev == lattice_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": grad_dev must not be lattice_dev");
  if ((rc = check_common(w, lattice_dev, workspace_dev, workspace_bytes, p)) != T2FIT_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace_dev);
  MetricArgs a = metric_args(launch_axes(p, lattice_dev, ws, st), bins_dev, n_f, n_m, lo_m, scale_m, fixed_mask_dev, moving_dev,
                             moving_mask_dev, mz, my, mx, A);
  a.table = table_dev;
  a.xs = reinterpret_cast<double*>(ws + p.xs_at);
  double* ys = reinterpret_cast<double*>(ws + p.ys_at);
  launch_rows(a, (size_t)n_f * n_m * sizeof(double), st);
  hipLaunchKernelGGL(ffd_y_kernel, dim3((unsigned)ceil_div((int64_t)fz * 3 * side * side, (int64_t)kBlock)), dim3(kBlock), 0, st,
                     (const double*)a.xs, a.L.ax, side, ys);
  hipLaunchKernelGGL(ffd_z_kernel, dim3((unsigned)ceil_div(3 * side * side * side, kBlock)), dim3(kBlock), 0, st, (const double*)ys, a.L.ax, side,
                     grad_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_ffd_warp_dev(const void* src_dev, int src_type, int nz, int ny, int nx, const double* A, const double* lattice_dev, int side,
                       void* out_dev, int oz, int oy, int ox, int interp, double default_value, void* workspace_dev, size_t workspace_bytes,
                       void* stream) {
  const std::string w("t2fit_ffd_warp_dev");
  if (!src_dev || !out_dev || !A || !lattice_dev || !workspace_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": src_dev / out_dev / A / lattice_dev / workspace_dev is NULL");
  if (src_type != T2FIT_RESAMPLE_F32 && src_type != T2FIT_RESAMPLE_I32)
    return t2fit::fail(T2FIT_E_INVALID, w + ": unknown src_type (T2FIT_RESAMPLE_F32 or T2FIT_RESAMPLE_I32)");
  if (interp != T2FIT_INTERP_LINEAR && interp != T2FIT_INTERP_NEAREST)
    return t2fit::fail(T2FIT_E_INVALID, w + ": unknown interp (T2FIT_INTERP_LINEAR or T2FIT_INTERP_NEAREST)");
  if (src_type == T2FIT_RESAMPLE_I32 && interp != T2FIT_INTERP_NEAREST)
    return t2fit::fail(T2FIT_E_INVALID, w + ": an int32 source is warped with T2FIT_INTERP_NEAREST only");
  Plan p;
  int rc = make_plan(w, oz, oy, ox, side, &p);
  if (rc != T2FIT_OK) return rc;
  if (t2fit::count_voxels(1, nz, ny, nx) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the moving sizes (the source's) must all be >= 1 and the volume at most 2^40 elements");
  if (!t2fit::finite12(A)) return t2fit::fail(T2FIT_E_INVALID, w + ": A has a non-finite entry");
  if (src_type == T2FIT_RESAMPLE_I32 && !(default_value >= -2147483648.0 && default_value <= 2147483647.0))
    return t2fit::fail(T2FIT_E_INVALID, w + ": default_value does not fit the int32 source");
  if (misaligned(src_dev, 4) || misaligned(out_dev, 4)) return t2fit::fail(T2FIT_E_INVALID, w + ": src_dev / out_dev is not aligned to 4 bytes");
  if (src_dev == out_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": out_dev must not be src_dev");
  if ((rc = check_common(w, lattice_dev, workspace_dev, workspace_bytes, p)) != T2FIT_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  WarpArgs a;
  a.L = launch_axes(p, lattice_dev, static_cast<char*>(workspace_dev), st);
  a.src = static_cast<const uint32_t*>(src_dev), a.out = static_cast<uint32_t*>(out_dev), a.n = Dims{nz, ny, nx};
  for (int i = 0; i < 12; ++i) a.A.m[i] = A[i];
  a.nearest = interp == T2FIT_INTERP_NEAREST;
  if (src_type == T2FIT_RESAMPLE_I32) {
    a.default_bits = (uint32_t)(int32_t)default_value;
  } else {
    const float f = (float)default_value;
    static_assert(sizeof(f) == sizeof(a.default_bits), "bit copy");
    __builtin_memcpy(&a.default_bits, &f, 4);
  }
  hipLaunchKernelGGL(ffd_warp_kernel, dim3((unsigned)a.L.n_tiles), dim3(kBlock), 0, st, a);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_ffd_jacobian_dev(const double* lattice_dev, int side, const uint8_t* mask_dev, int fz, int fy, int fx, double* min_dev,
                           int64_t* n_folded_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  const std::string w("t2fit_ffd_jacobian_dev");
  if (!lattice_dev || !mask_dev || !min_dev || !n_folded_dev || !workspace_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": lattice_dev / mask_dev / min_dev / n_folded_dev / workspace_dev is NULL");
  Plan p;
  int rc = make_plan(w, fz, fy, fx, side, &p);
  if (rc != T2FIT_OK) return rc;
  if (misaligned(min_dev, 8) || misaligned(n_folded_dev, 8))
    return t2fit::fail(T2FIT_E_INVALID, w + ": min_dev / n_folded_dev is not aligned to 8 bytes");
  if ((rc = check_common(w, lattice_dev, workspace_dev, workspace_bytes, p)) != T2FIT_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace_dev);
  JacArgs a;
  a.L = launch_axes(p, lattice_dev, ws, st);
  a.mask = mask_dev;
  a.row_min = reinterpret_cast<double*>(ws + p.min_at);
  a.row_cnt = reinterpret_cast<unsigned long long*>(ws + p.cnt_at);
  hipLaunchKernelGGL(ffd_jac_kernel, dim3((unsigned)a.L.n_tiles), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(ffd_jac_final_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)a.row_min, (const unsigned long long*)a.row_cnt, p.rows,
                     min_dev, reinterpret_cast<long long*>(n_folded_dev));
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

}  // extern "C"

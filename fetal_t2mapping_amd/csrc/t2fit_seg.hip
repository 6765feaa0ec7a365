// t2fit_seg.hip -- gfx950 kernels and C ABI of the atlas-prior EM tissue segmentation (include/t2fit.h: t2fit_seg_*).
// A Gaussian mixture over 1 .. 4 channels (echoes) with spatial priors and a mean-field Potts term; the loop, the class
// model and the stop rule are host code (fetal_t2mapping_amd/_seg.py, which also states every kernel in numpy).
//   seg_mask_kernel       M = mask != 0 and every channel finite; streaming.
//   seg_blur_kernel       one pass of the separable Gaussian along one axis for one class plane per blockIdx.y: an ordered
//                         float64 sum of at most 65 taps, one rounding to float32.  The x pass forms the one-hot image from
//                         the labels while it reads them; the taps travel in the kernel arguments.
//   seg_normalise_kernel  pi from the priors and the floor; streaming, one lane per voxel.
//   seg_sums_kernel       the moments of one class per blockIdx.y: a lane keeps its 4 voxels' channel values of the current
//                         class walk in registers, 1 + C + C (C + 1) / 2 float64 accumulators, the wave butterfly and the
//                         four-wave LDS step; per-workgroup partials, then the fixed tree of t2fit_reduce.h.
//   seg_estep_kernel<C>   one E-step: lanes along x, a 4 x 4 x 64 tile per workgroup (a lane walks 4 slices), the model in the
//                         kernel arguments (scalar loads), a_k and q_k of the 8 possible classes in registers behind a
//                         compile-time loop bound; the six neighbours of p_old come through the vector cache.
//   seg_labels_kernel     first argmax.
// No floating-point atomics; every sum runs in the order the header fixes.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "t2fit_affine.h"
#include "t2fit_error.h"
#include "t2fit_reduce.h"
#include "t2fit_support.h"

namespace {

using t2fit::align_up, t2fit::kBlock, t2fit::count_voxels, t2fit::misaligned;
using t2fit::finite_bits, t2fit::wave_butterfly, t2fit::TreePasses, t2fit::tree_plan, t2fit::tree_launch;

constexpr int kMaxClass = T2FIT_SEG_MAX_CLASSES, kMaxChan = T2FIT_SEG_MAX_CHANNELS, kMaxRadius = T2FIT_SEG_MAX_RADIUS;
constexpr int kMaxMoments = 1 + kMaxChan + kMaxChan * (kMaxChan + 1) / 2;  // 15
constexpr int kVoxPerLane = 4, kVoxPerBlock = kVoxPerLane * kBlock;        // the sums kernel: 1024 voxels per workgroup
constexpr int kFan = t2fit::kTreeFan;                                      // values one workgroup of a reduce pass folds
constexpr int kWaves = kBlock / 64;
constexpr int kTileZ = 4, kTileY = 4, kTileX = 64;  // the E-step: lanes (64, 4), each walking kTileZ slices
constexpr size_t kAlign = 256;
static_assert(kWaves == 4, "the header fixes the tree of four waves");

__global__ __launch_bounds__(kBlock) void seg_mask_kernel(const float* __restrict__ y, const uint8_t* __restrict__ mask, int n_chan, int64_t n,
                                                          uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  bool in = !mask || mask[i] != 0;
  for (int c = 0; c < n_chan; ++c) in = in && finite_bits(y[(int64_t)c * n + i]);
  out[i] = in ? 1 : 0;
}

struct BlurArgs {
  double w[2 * kMaxRadius + 1];
  int32_t classes[kMaxClass];
  const int32_t* labels;  // the x pass: the one-hot image is labels == classes[plane]
  const float* in;        // the y and z passes: K planes
  float* out;
  int64_t n, stride;  // voxels of a plane; elements between neighbours along the axis
  int len, radius;    // size of the axis
};

template <bool ONEHOT> __global__ __launch_bounds__(kBlock) void seg_blur_kernel(const BlurArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const int k = blockIdx.y;
  const int pos = (int)((i / a.stride) % a.len);
  const int lo = pos - a.radius < 0 ? a.radius - pos : 0;  // first tap inside the volume
  const int hi = pos + a.radius > a.len - 1 ? a.radius + (a.len - 1 - pos) : 2 * a.radius;
  double acc = 0.0;
  if (ONEHOT) {
    const int32_t want = a.classes[k];
    const int32_t* p = a.labels + i - (int64_t)a.radius * a.stride;
    for (int j = lo; j <= hi; ++j) acc = acc + a.w[j] * (p[(int64_t)j * a.stride] == want ? 1.0 : 0.0);
  } else {
    const float* p = a.in + (int64_t)k * a.n + i - (int64_t)a.radius * a.stride;
    for (int j = lo; j <= hi; ++j) acc = acc + a.w[j] * (double)p[(int64_t)j * a.stride];
  }
  a.out[(int64_t)k * a.n + i] = (float)acc;
}

__global__ __launch_bounds__(kBlock) void seg_normalise_kernel(const float* __restrict__ prior, const uint8_t* __restrict__ mask, int n_class,
                                                               int64_t n, double floor, float* __restrict__ pi) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const bool in = mask[i] != 0;
  double sum = 0.0;
  if (in)
    for (int l = 0; l < n_class; ++l) sum = sum + (double)prior[(int64_t)l * n + i];
  const double den = sum + (double)n_class * floor;
  for (int k = 0; k < n_class; ++k) pi[(int64_t)k * n + i] = in ? (float)(((double)prior[(int64_t)k * n + i] + floor) / den) : 0.0f;
}

// partials[(k M + m) n_blocks + block]: the moments of class k = blockIdx.y over the workgroup's 1024 voxels
template <int C> __global__ __launch_bounds__(kBlock) void seg_sums_kernel(const float* __restrict__ p, const float* __restrict__ y,
                                                                          const uint8_t* __restrict__ mask, int64_t n, int64_t n_blocks,
                                                                          double* __restrict__ partials) {
  constexpr int M = 1 + C + C * (C + 1) / 2;
  __shared__ double rows[kWaves][M];
  const int k = blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * kVoxPerBlock + threadIdx.x;
  double acc[M];
#pragma unroll
  for (int m = 0; m < M; ++m) acc[m] = 0.0;
#pragma unroll
  for (int j = 0; j < kVoxPerLane; ++j) {
    const int64_t i = base + (int64_t)j * kBlock;
    if (i >= n || mask[i] == 0) continue;
    double yv[C];
    bool fin = true;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float f = y[(int64_t)c * n + i];
      fin = fin && finite_bits(f);
      yv[c] = (double)f;
    }
    if (!fin) continue;
    const double pv = (double)p[(int64_t)k * n + i];
    acc[0] = acc[0] + pv;
    int m = 1 + C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double py = pv * yv[c];
      acc[1 + c] = acc[1 + c] + py;
#pragma unroll
      for (int d = c; d < C; ++d, ++m) acc[m] = acc[m] + py * yv[d];
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const double s = wave_butterfly(acc[m]);
    if (lane == 0) rows[wave][m] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < M) {
    const int m = threadIdx.x;
    partials[((int64_t)k * M + m) * n_blocks + blockIdx.x] = ((rows[0][m] + rows[1][m]) + rows[2][m]) + rows[3][m];
  }
}

struct EstepArgs {
  double model[kMaxClass][kMaxMoments];  // per class: mu (C), the upper triangle of P row-major, c
  int32_t live[kMaxClass];
  const float* p_old;
  const float* pi;
  const float* y;
  const uint8_t* mask;
  float* p_new;
  double beta;
  int64_t n;
  int n_class, nz, ny, nx;
};

template <int C> __global__ __launch_bounds__(kBlock) void seg_estep_kernel(const EstepArgs a) {
  const int x = blockIdx.x * kTileX + (threadIdx.x & (kTileX - 1));
  const int yy = blockIdx.y * kTileY + (threadIdx.x / kTileX);
  if (x >= a.nx || yy >= a.ny) return;
  const int64_t plane = (int64_t)a.ny * a.nx;
  for (int dz = 0; dz < kTileZ; ++dz) {
    const int z = blockIdx.z * kTileZ + dz;
    if (z >= a.nz) return;
    const int64_t i = (int64_t)z * plane + (int64_t)yy * a.nx + x;
    float yf[C];
    bool in = a.mask[i] != 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      yf[c] = a.y[(int64_t)c * a.n + i];
      in = in && finite_bits(yf[c]);
    }
    if (!in) {
      for (int k = 0; k < a.n_class; ++k) a.p_new[(int64_t)k * a.n + i] = 0.0f;
      continue;
    }
    // the neighbours that count, in the order of the sum: -z, -y, -x, +x, +y, +z
    const bool n0 = z > 0 && a.mask[i - plane] != 0, n1 = yy > 0 && a.mask[i - a.nx] != 0, n2 = x > 0 && a.mask[i - 1] != 0;
    const bool n3 = x + 1 < a.nx && a.mask[i + 1] != 0, n4 = yy + 1 < a.ny && a.mask[i + a.nx] != 0,
               n5 = z + 1 < a.nz && a.mask[i + plane] != 0;
    double av[kMaxClass];
    double top = -INFINITY;
#pragma unroll
    for (int k = 0; k < kMaxClass; ++k) {
      av[k] = 0.0;
      if (k < a.n_class && a.live[k]) {
        double t[C];
#pragma unroll
        for (int c = 0; c < C; ++c) t[c] = (double)yf[c] - a.model[k][c];
        double d = 0.0;
        int m = C;
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
          for (int e = c; e < C; ++e, ++m) d = d + (((c == e ? 1.0 : 2.0) * a.model[k][m]) * t[c]) * t[e];
        const float* po = a.p_old + (int64_t)k * a.n + i;
        double nb = 0.0;
        if (n0) nb = nb + (1.0 - (double)po[-plane]);
        if (n1) nb = nb + (1.0 - (double)po[-a.nx]);
        if (n2) nb = nb + (1.0 - (double)po[-1]);
        if (n3) nb = nb + (1.0 - (double)po[1]);
        if (n4) nb = nb + (1.0 - (double)po[a.nx]);
        if (n5) nb = nb + (1.0 - (double)po[plane]);
        av[k] = (a.model[k][C + C * (C + 1) / 2] - 0.5 * d) - a.beta * nb;
        top = av[k] > top ? av[k] : top;
      }
    }
    double q[kMaxClass];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kMaxClass; ++k) {
      q[k] = 0.0;
      if (k < a.n_class && a.live[k]) {
        q[k] = (double)a.pi[(int64_t)k * a.n + i] * exp(av[k] - top);
        s = s + q[k];
      }
    }
#pragma unroll
    for (int k = 0; k < kMaxClass; ++k)
      if (k < a.n_class) a.p_new[(int64_t)k * a.n + i] = a.live[k] ? (float)(q[k] / s) : 0.0f;
  }
}

struct LabelArgs {
  int32_t classes[kMaxClass];
  const float* p;
  const uint8_t* mask;
  int32_t* out;
  int64_t n;
  int n_class;
};

__global__ __launch_bounds__(kBlock) void seg_labels_kernel(const LabelArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  int32_t lab = 0;
  if (a.mask[i] != 0) {
    float best = a.p[i];
    int arg = 0;
    for (int k = 1; k < a.n_class; ++k) {
      const float v = a.p[(int64_t)k * a.n + i];
      if (v > best) best = v, arg = k;
    }
    lab = a.classes[arg];
  }
  a.out[i] = lab;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
int sizes_check(const std::string& w, int n_class, int n_chan, int nz, int ny, int nx, int64_t* n_vox) {
  if (n_class < 2 || n_class > kMaxClass) return t2fit::fail(T2FIT_E_INVALID, w + ": n_class must be 2 .. T2FIT_SEG_MAX_CLASSES");
  if (n_chan < 1 || n_chan > kMaxChan) return t2fit::fail(T2FIT_E_INVALID, w + ": n_chan must be 1 .. T2FIT_SEG_MAX_CHANNELS");
  const int64_t n = count_voxels(n_class > n_chan ? n_class : n_chan, nz, ny, nx);
  if (n < 0 || (int64_t)nz * ny * nx > ((int64_t)1 << 37))
    return t2fit::fail(T2FIT_E_INVALID, w + ": nz, ny, nx must all be >= 1 and the volume at most 2^37 voxels");
  *n_vox = (int64_t)nz * ny * nx;
  return T2FIT_OK;
}

int flat_check(const std::string& w, int n_class, int64_t n_vox) {
  if (n_class < 2 || n_class > kMaxClass) return t2fit::fail(T2FIT_E_INVALID, w + ": n_class must be 2 .. T2FIT_SEG_MAX_CLASSES");
  if (n_vox < 1 || n_vox > ((int64_t)1 << 40) / kMaxClass) return t2fit::fail(T2FIT_E_INVALID, w + ": n_vox must be 1 .. 2^37");
  return T2FIT_OK;
}

size_t sums_bytes(int n_class, int n_chan, int64_t n_vox) {
  const size_t q = (size_t)n_class * (size_t)(1 + n_chan + n_chan * (n_chan + 1) / 2);
  const size_t nb = (size_t)t2fit::ceil_div<int64_t>(n_vox, kVoxPerBlock);
  return align_up(q * nb * 8, kAlign) + align_up(q * t2fit::ceil_div<size_t>(nb, kFan) * 8, kAlign);
}

template <int C> void launch_sums(dim3 grid, hipStream_t st, const float* p, const float* y, const uint8_t* m, int64_t n, int64_t nb, double* part) {
  hipLaunchKernelGGL(seg_sums_kernel<C>, grid, dim3(kBlock), 0, st, p, y, m, n, nb, part);
}

}  // namespace

extern "C" {

int t2fit_seg_workspace_bytes(int n_class, int n_chan, int nz, int ny, int nx, size_t* bytes) {
  const std::string w("t2fit_seg_workspace_bytes");
  if (!bytes) return t2fit::fail(T2FIT_E_INVALID, w + ": bytes is NULL");
  int64_t n = 0;
  const int rc = sizes_check(w, n_class, n_chan, nz, ny, nx, &n);
  if (rc != T2FIT_OK) return rc;
  const size_t blur = align_up((size_t)n_class * (size_t)n * 4, kAlign), sums = sums_bytes(n_class, n_chan, n);
  *bytes = blur > sums ? blur : sums;
  return T2FIT_OK;
}

int t2fit_seg_mask_dev(const float* y_dev, const uint8_t* mask_dev, int n_chan, int64_t n_vox, uint8_t* m_out_dev, void* stream) {
  const std::string w("t2fit_seg_mask_dev");
  if (!y_dev || !m_out_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": y_dev / m_out_dev is NULL");
  if (n_chan < 1 || n_chan > kMaxChan) return t2fit::fail(T2FIT_E_INVALID, w + ": n_chan must be 1 .. T2FIT_SEG_MAX_CHANNELS");
  const int rc = flat_check(w, 2, n_vox);
  if (rc != T2FIT_OK) return rc;
  if (misaligned(y_dev, 4)) return t2fit::fail(T2FIT_E_INVALID, w + ": y_dev is not aligned to 4 bytes");
  hipLaunchKernelGGL(seg_mask_kernel, dim3((unsigned)t2fit::ceil_div<int64_t>(n_vox, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, y_dev, mask_dev,
                     n_chan, n_vox, m_out_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_seg_priors_dev(const int32_t* labels_dev, const int32_t* classes, int n_class, int nz, int ny, int nx, const double* taps_z, int rz,
                         const double* taps_y, int ry, const double* taps_x, int rx, float* prior_out_dev, void* workspace_dev, void* stream) {
  const std::string w("t2fit_seg_priors_dev");
  if (!labels_dev || !classes || !taps_z || !taps_y || !taps_x || !prior_out_dev || !workspace_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": labels_dev / classes / taps_z / taps_y / taps_x / prior_out_dev / workspace_dev is NULL");
  int64_t n = 0;
  const int rc = sizes_check(w, n_class, 1, nz, ny, nx, &n);
  if (rc != T2FIT_OK) return rc;
  if (rz < 0 || rz > kMaxRadius || ry < 0 || ry > kMaxRadius || rx < 0 || rx > kMaxRadius)
    return t2fit::fail(T2FIT_E_INVALID, w + ": rz / ry / rx (the radius of the taps) must be 0 .. T2FIT_SEG_MAX_RADIUS");
  if (misaligned(labels_dev, 4) || misaligned(prior_out_dev, 4) || misaligned(workspace_dev, 4))
    return t2fit::fail(T2FIT_E_INVALID, w + ": labels_dev / prior_out_dev / workspace_dev is not aligned to 4 bytes");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)t2fit::ceil_div<int64_t>(n, kBlock), (unsigned)n_class);
  float* tmp = static_cast<float*>(workspace_dev);
  BlurArgs a = {};
  for (int k = 0; k < n_class; ++k) a.classes[k] = classes[k];
  a.n = n;
  // x: labels -> prior_out;  y: prior_out -> workspace;  z: workspace -> prior_out
  for (int j = 0; j <= 2 * rx; ++j) a.w[j] = taps_x[j];
  a.labels = labels_dev, a.in = nullptr, a.out = prior_out_dev, a.stride = 1, a.len = nx, a.radius = rx;
  hipLaunchKernelGGL(seg_blur_kernel<true>, grid, dim3(kBlock), 0, st, a);
  T2_HIP(hipGetLastError());
  for (int j = 0; j <= 2 * ry; ++j) a.w[j] = taps_y[j];
  a.labels = nullptr, a.in = prior_out_dev, a.out = tmp, a.stride = nx, a.len = ny, a.radius = ry;
  hipLaunchKernelGGL(seg_blur_kernel<false>, grid, dim3(kBlock), 0, st, a);
  T2_HIP(hipGetLastError());
  for (int j = 0; j <= 2 * rz; ++j) a.w[j] = taps_z[j];
  a.in = tmp, a.out = prior_out_dev, a.stride = (int64_t)ny * nx, a.len = nz, a.radius = rz;
  hipLaunchKernelGGL(seg_blur_kernel<false>, grid, dim3(kBlock), 0, st, a);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_seg_normalise_dev(const float* prior_dev, const uint8_t* mask_dev, int n_class, int64_t n_vox, double floor, float* pi_out_dev,
                            void* stream) {
  const std::string w("t2fit_seg_normalise_dev");
  if (!prior_dev || !mask_dev || !pi_out_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": prior_dev / mask_dev / pi_out_dev is NULL");
  const int rc = flat_check(w, n_class, n_vox);
  if (rc != T2FIT_OK) return rc;
  if (!(floor >= 0.0) || !std::isfinite(floor)) return t2fit::fail(T2FIT_E_INVALID, w + ": floor must be finite and >= 0");
  if (misaligned(prior_dev, 4) || misaligned(pi_out_dev, 4))
    return t2fit::fail(T2FIT_E_INVALID, w + ": prior_dev / pi_out_dev is not aligned to 4 bytes");
  hipLaunchKernelGGL(seg_normalise_kernel, dim3((unsigned)t2fit::ceil_div<int64_t>(n_vox, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, prior_dev,
                     mask_dev, n_class, n_vox, floor, pi_out_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_seg_sums_dev(const float* p_dev, const float* y_dev, const uint8_t* mask_dev, int n_class, int n_chan, int nz, int ny, int nx,
                       double* sums_out_dev, void* workspace_dev, void* stream) {
  const std::string w("t2fit_seg_sums_dev");
  if (!p_dev || !y_dev || !mask_dev || !sums_out_dev || !workspace_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": p_dev / y_dev / mask_dev / sums_out_dev / workspace_dev is NULL");
  int64_t n = 0;
  const int rc = sizes_check(w, n_class, n_chan, nz, ny, nx, &n);
  if (rc != T2FIT_OK) return rc;
  if (misaligned(p_dev, 4) || misaligned(y_dev, 4)) return t2fit::fail(T2FIT_E_INVALID, w + ": p_dev / y_dev is not aligned to 4 bytes");
  if (misaligned(sums_out_dev, 8) || misaligned(workspace_dev, 8))
    return t2fit::fail(T2FIT_E_INVALID, w + ": sums_out_dev / workspace_dev is not aligned to 8 bytes");
  const int M = 1 + n_chan + n_chan * (n_chan + 1) / 2, Q = n_class * M;
  const int64_t nb = t2fit::ceil_div<int64_t>(n, kVoxPerBlock);
  hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace_dev);
  const dim3 grid((unsigned)nb, (unsigned)n_class);
  switch (n_chan) {
    case 1: launch_sums<1>(grid, st, p_dev, y_dev, mask_dev, n, nb, part); break;
    case 2: launch_sums<2>(grid, st, p_dev, y_dev, mask_dev, n, nb, part); break;
    case 3: launch_sums<3>(grid, st, p_dev, y_dev, mask_dev, n, nb, part); break;
    default: launch_sums<4>(grid, st, p_dev, y_dev, mask_dev, n, nb, part); break;
  }
  T2_HIP(hipGetLastError());
  // the tree over the partials: passes of 256 until one value is left, at least one; the last one writes the result.  The
  // passes read and write the two parts of the workspace (sums_bytes) in turn
  const size_t second = align_up((size_t)Q * (size_t)nb * 8, kAlign);
  TreePasses tree;
  int pass = 0;
  tree_plan(&tree, nb, [&](int64_t) { return pass++ % 2 == 0 ? (size_t)0 : second; });
  tree_launch(tree, Q, workspace_dev, sums_out_dev, st);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_seg_estep_dev(const float* p_old_dev, const float* pi_dev, const float* y_dev, const uint8_t* mask_dev, const double* model,
                        const int32_t* live, double beta, int n_class, int n_chan, int nz, int ny, int nx, float* p_new_dev, void* stream) {
  const std::string w("t2fit_seg_estep_dev");
  if (!p_old_dev || !pi_dev || !y_dev || !mask_dev || !model || !live || !p_new_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": p_old_dev / pi_dev / y_dev / mask_dev / model / live / p_new_dev is NULL");
  int64_t n = 0;
  const int rc = sizes_check(w, n_class, n_chan, nz, ny, nx, &n);
  if (rc != T2FIT_OK) return rc;
  if (p_new_dev == p_old_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": p_new_dev must not be p_old_dev (the step is not in place)");
  if (!(beta >= 0.0) || !std::isfinite(beta)) return t2fit::fail(T2FIT_E_INVALID, w + ": beta must be finite and >= 0");
  if (misaligned(p_old_dev, 4) || misaligned(pi_dev, 4) || misaligned(y_dev, 4) || misaligned(p_new_dev, 4))
    return t2fit::fail(T2FIT_E_INVALID, w + ": p_old_dev / pi_dev / y_dev / p_new_dev is not aligned to 4 bytes");
  if (t2fit::ceil_div(ny, kTileY) > 65535 || t2fit::ceil_div(nz, kTileZ) > 65535)
    return t2fit::fail(T2FIT_E_INVALID, w + ": ny and nz must be at most 262140");
  const int M = n_chan + n_chan * (n_chan + 1) / 2 + 1;
  EstepArgs a = {};
  bool any = false;
  for (int k = 0; k < n_class; ++k) {
    a.live[k] = live[k] != 0;
    any = any || a.live[k];
    for (int m = 0; m < M; ++m) a.model[k][m] = model[k * M + m];
  }
  if (!any) return t2fit::fail(T2FIT_E_INVALID, w + ": live marks no class");
  a.p_old = p_old_dev, a.pi = pi_dev, a.y = y_dev, a.mask = mask_dev, a.p_new = p_new_dev;
  a.beta = beta, a.n = n, a.n_class = n_class, a.nz = nz, a.ny = ny, a.nx = nx;
  const dim3 grid((unsigned)t2fit::ceil_div(nx, kTileX), (unsigned)t2fit::ceil_div(ny, kTileY), (unsigned)t2fit::ceil_div(nz, kTileZ));
  hipStream_t st = (hipStream_t)stream;
  switch (n_chan) {
    case 1: hipLaunchKernelGGL(seg_estep_kernel<1>, grid, dim3(kBlock), 0, st, a); break;
    case 2: hipLaunchKernelGGL(seg_estep_kernel<2>, grid, dim3(kBlock), 0, st, a); break;
    case 3: hipLaunchKernelGGL(seg_estep_kernel<3>, grid, dim3(kBlock), 0, st, a); break;
    default: hipLaunchKernelGGL(seg_estep_kernel<4>, grid, dim3(kBlock), 0, st, a); break;
  }
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_seg_labels_dev(const float* p_dev, const uint8_t* mask_dev, const int32_t* classes, int n_class, int64_t n_vox, int32_t* labels_out_dev,
                         void* stream) {
  const std::string w("t2fit_seg_labels_dev");
  if (!p_dev || !mask_dev || !classes || !labels_out_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": p_dev / mask_dev / classes / labels_out_dev is NULL");
  const int rc = flat_check(w, n_class, n_vox);
  if (rc != T2FIT_OK) return rc;
  if (misaligned(p_dev, 4) || misaligned(labels_out_dev, 4))
    return t2fit::fail(T2FIT_E_INVALID, w + ": p_dev / labels_out_dev is not aligned to 4 bytes");
  LabelArgs a = {};
  for (int k = 0; k < n_class; ++k) a.classes[k] = classes[k];
  a.p = p_dev, a.mask = mask_dev, a.out = labels_out_dev, a.n = n_vox, a.n_class = n_class;
  hipLaunchKernelGGL(seg_labels_kernel, dim3((unsigned)t2fit::ceil_div<int64_t>(n_vox, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, a);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

}  // extern "C"

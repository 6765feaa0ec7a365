// t2fit_sr_robust.hip -- gfx950 kernels and C ABI of the outlier weighting of the super-resolution loop (include/t2fit.h:
// t2fit_sr_robust_params_default, t2fit_sr_robust_workspace_bytes, t2fit_sr_robust_dev).  The residuals A_s x - y_s of every
// stack are multiplied, in place and between the forward and the adjoint operator, by a slice weight and a Huber sample
// weight, both scaled by a robust noise estimate per echo; fetal_t2mapping_amd/_sr.py (robust_slice_sums, robust_scale,
// robust_apply) restates the three steps in numpy.
//   sr_robust_sums_kernel   one workgroup per slice and chunk of kRobustChunk echoes: the count and the sum of squares of
//                           the counted samples in a fixed tree.  Lanes run along the slice (x fastest), so the reads of r
//                           are coalesced; N and the mask are read once per chunk.
//   sr_robust_scale_kernel  one workgroup per echo: the mean squares of the eligible slices in LDS, their median by ranks
//                           (counting, ties broken by index: exact and independent of order), sigma2 and the slice weights.
//   sr_robust_apply_kernel  one thread per sample and chunk of echoes, streaming: reads sigma2 and the slice weight from the
//                           tables, writes the weighted residual.
// No floating-point atomics; every sum runs in the order the header fixes.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "t2fit_affine.h"
#include "t2fit_error.h"
#include "t2fit_support.h"

namespace {

using t2fit::align_up, t2fit::kBlock, t2fit::count_voxels, t2fit::wave_butterfly, t2fit::finite_bits;

constexpr int kRobustChunk = 4;  // echoes per read of N and the mask, as kSrChunk of the operators
constexpr int kWaves = kBlock / 64;
constexpr size_t kAlign = 256;
static_assert(kWaves == 4, "the header fixes the tree of four waves");

struct RobustStack {
  float* r;             // [n_vol][n_l], in / out
  const double* N;      // [n_l]
  const uint8_t* mask;  // [n_l] or NULL
  int64_t plane, n_l;   // ly lx, lz ly lx
  int64_t block0;       // first workgroup of the stack in the apply grid
  int slice0, lz;       // first slice of the stack in the tables
};

struct RobustArgs {
  RobustStack s[T2FIT_SR_MAX_STACKS];
  double* sums;     // [n_vol][n_slices][2]
  double* weights;  // [n_vol][n_slices]
  double* sigma2;   // [n_vol]
  double tt, huber, floor2;
  int n_stacks, n_vol, n_slices, min_count;
};

__global__ __launch_bounds__(kBlock) void sr_robust_sums_kernel(const RobustArgs a) {
  __shared__ double rows[kWaves][2 * kRobustChunk];
  const int slice = blockIdx.x;
  int s = 0;
  while (s + 1 < a.n_stacks && slice >= a.s[s + 1].slice0) ++s;
  const RobustStack& k = a.s[s];
  const int e0 = blockIdx.y * kRobustChunk;
  const int ne = a.n_vol - e0 < kRobustChunk ? a.n_vol - e0 : kRobustChunk;
  const int64_t base = (int64_t)(slice - k.slice0) * k.plane;
  double c[kRobustChunk], q2[kRobustChunk];
#pragma unroll
  for (int v = 0; v < kRobustChunk; ++v) c[v] = 0.0, q2[v] = 0.0;
  for (int64_t i = threadIdx.x; i < k.plane; i += kBlock) {
    const int64_t j = base + i;
    const bool counts = k.N[j] > 0.0 && (!k.mask || k.mask[j] != 0);
#pragma unroll
    for (int v = 0; v < kRobustChunk; ++v)
      if (v < ne) {
        const float rv = k.r[(int64_t)(e0 + v) * k.n_l + j];
        if (counts && finite_bits(rv)) {
          const double d = (double)rv;
          q2[v] = q2[v] + d * d;
          c[v] = c[v] + 1.0;
        }
      }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < kRobustChunk; ++v) {
    const double cs = wave_butterfly(c[v]), qs = wave_butterfly(q2[v]);
    if (lane == 0) rows[wave][2 * v] = cs, rows[wave][2 * v + 1] = qs;
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * ne) {
    const int q = threadIdx.x;
    a.sums[((int64_t)(e0 + (q >> 1)) * a.n_slices + slice) * 2 + (q & 1)] = ((rows[0][q] + rows[1][q]) + rows[2][q]) + rows[3][q];
  }
}

__global__ __launch_bounds__(kBlock) void sr_robust_scale_kernel(const RobustArgs a) {
  __shared__ double m[T2FIT_SR_ROBUST_MAX_SLICES];  // the mean square of an eligible slice, else -1
  __shared__ double med[2];
  __shared__ int n_eligible;
  const int e = blockIdx.x, tid = threadIdx.x;
  const double* su = a.sums + (int64_t)e * a.n_slices * 2;
  if (tid == 0) n_eligible = 0, med[0] = 0.0, med[1] = 0.0;
  __syncthreads();
  int mine = 0;
  for (int k = tid; k < a.n_slices; k += kBlock) {
    const double c = su[2 * k], q2 = su[2 * k + 1];
    const bool eligible = c >= (double)a.min_count;
    m[k] = eligible ? q2 / c : -1.0;
    mine += eligible ? 1 : 0;
  }
  if (mine) atomicAdd(&n_eligible, mine);  // an integer count: exact in any order
  __syncthreads();
  const int n = n_eligible;
  if (n > 0)
    for (int k = tid; k < a.n_slices; k += kBlock) {
      const double mk = m[k];
      if (!(mk >= 0.0)) continue;
      int rank = 0;
      for (int j = 0; j < a.n_slices; ++j) {
        const double mj = m[j];
        rank += (mj >= 0.0 && (mj < mk || (mj == mk && j < k))) ? 1 : 0;
      }
      if (rank == (n - 1) / 2) med[0] = mk;
      if (rank == n / 2) med[1] = mk;
    }
  __syncthreads();
  double s2 = 0.0;
  if (n > 0) {
    s2 = 0.5 * (med[0] + med[1]);
    s2 = s2 > a.floor2 ? s2 : a.floor2;
    if (!(s2 > 0.0)) s2 = 0.0;
  }
  const bool on = s2 > 0.0;
  const double limit = a.tt * s2;
  for (int k = tid; k < a.n_slices; k += kBlock) {
    const double mk = m[k];
    a.weights[(int64_t)e * a.n_slices + k] = (on && mk >= 0.0 && !(mk <= limit)) ? limit / mk : 1.0;
  }
  if (tid == 0) a.sigma2[e] = s2;
}

__global__ __launch_bounds__(kBlock) void sr_robust_apply_kernel(const RobustArgs a) {
  const int64_t block = blockIdx.x;
  int s = 0;
  while (s + 1 < a.n_stacks && block >= a.s[s + 1].block0) ++s;
  const RobustStack& k = a.s[s];
  const int64_t j = (block - k.block0) * kBlock + threadIdx.x;
  if (j >= k.n_l) return;
  const int e0 = blockIdx.y * kRobustChunk;
  const int ne = a.n_vol - e0 < kRobustChunk ? a.n_vol - e0 : kRobustChunk;
  const int slice = k.slice0 + (int)(j / k.plane);
  const bool counts = k.N[j] > 0.0 && (!k.mask || k.mask[j] != 0);
#pragma unroll
  for (int v = 0; v < kRobustChunk; ++v)
    if (v < ne) {
      const int e = e0 + v;
      const double s2 = a.sigma2[e];
      if (!(s2 > 0.0)) continue;  // robustness is off for this echo: the residual stays as it is
      float* p = k.r + (int64_t)e * k.n_l + j;
      const float rv = *p;
      float out = 0.0f;
      if (counts && finite_bits(rv)) {
        const double delta = a.huber * sqrt(s2), q = a.weights[(int64_t)e * a.n_slices + slice];
        const double d = (double)rv, ad = fabs(d);
        const double w = ad <= delta ? 1.0 : delta / ad;
        out = (float)((q * w) * d);
      }
      *p = out;
    }
}

int params_check(const std::string& w, const t2fit_sr_robust_params* p) {
  if (!p) return t2fit::fail(T2FIT_E_INVALID, w + ": params is NULL");
  if (!(p->slice_threshold > 0.0) || !std::isfinite(p->slice_threshold))
    return t2fit::fail(T2FIT_E_INVALID, w + ": slice_threshold must be finite and > 0");
  if (!(p->huber > 0.0) || !std::isfinite(p->huber)) return t2fit::fail(T2FIT_E_INVALID, w + ": huber must be finite and > 0");
  if (!(p->sigma_floor >= 0.0) || !std::isfinite(p->sigma_floor))
    return t2fit::fail(T2FIT_E_INVALID, w + ": sigma_floor must be finite and >= 0");
  if (p->min_count < 1) return t2fit::fail(T2FIT_E_INVALID, w + ": min_count must be >= 1");
  if (p->flags != 0) return t2fit::fail(T2FIT_E_INVALID, w + ": flags is reserved and must be 0");
  return T2FIT_OK;
}

// n_stacks, n_vol and the sizes; the number of slices of all stacks
int sizes_check(const std::string& w, int n_stacks, const int32_t* lo_size, int n_vol, int* n_slices) {
  if (n_stacks < 1 || n_stacks > T2FIT_SR_MAX_STACKS)
    return t2fit::fail(T2FIT_E_INVALID, w + ": n_stacks must be 1 .. T2FIT_SR_MAX_STACKS");
  int64_t total = 0;
  for (int s = 0; s < n_stacks; ++s) {
    if (count_voxels(n_vol, lo_size[3 * s], lo_size[3 * s + 1], lo_size[3 * s + 2]) < 0)
      return t2fit::fail(T2FIT_E_INVALID, w + ": n_vol and the sizes must all be >= 1 and a stack at most 2^40 elements");
    total += lo_size[3 * s];
  }
  if (total > T2FIT_SR_ROBUST_MAX_SLICES)
    return t2fit::fail(T2FIT_E_INVALID, w + ": more than T2FIT_SR_ROBUST_MAX_SLICES slices in total");
  *n_slices = (int)total;
  return T2FIT_OK;
}

}  // namespace

extern "C" {

int t2fit_sr_robust_params_default(t2fit_sr_robust_params* p) {
  if (!p) return t2fit::fail(T2FIT_E_INVALID, "t2fit_sr_robust_params_default: params is NULL");
  p->slice_threshold = 1.5, p->huber = 2.5, p->sigma_floor = 0.0, p->min_count = 16, p->flags = 0;
  return T2FIT_OK;
}

int t2fit_sr_robust_workspace_bytes(int n_stacks, const int32_t* lo_size, int n_vol, size_t* bytes) {
  const std::string w("t2fit_sr_robust_workspace_bytes");
  if (!lo_size || !bytes) return t2fit::fail(T2FIT_E_INVALID, w + ": lo_size / bytes is NULL");
  int n_slices = 0;
  const int rc = sizes_check(w, n_stacks, lo_size, n_vol, &n_slices);
  if (rc != T2FIT_OK) return rc;
  const size_t cells = (size_t)n_vol * (size_t)n_slices;
  *bytes = align_up(cells * 16, kAlign) + align_up(cells * 8, kAlign) + align_up((size_t)n_vol * 8, kAlign);
  return T2FIT_OK;
}

int t2fit_sr_robust_dev(int n_stacks, float* const* r_dev, const double* const* N_dev, const uint8_t* const* mask_dev,
                        const int32_t* lo_size, int n_vol, const t2fit_sr_robust_params* params, double* sums_dev,
                        double* weights_dev, double* sigma2_dev, void* stream) {
  const std::string w("t2fit_sr_robust_dev");
  if (!r_dev || !N_dev || !lo_size || !sums_dev || !weights_dev || !sigma2_dev)
    return t2fit::fail(T2FIT_E_INVALID, w + ": r_dev / N_dev / lo_size / sums_dev / weights_dev / sigma2_dev is NULL");
  int rc = params_check(w, params);
  if (rc != T2FIT_OK) return rc;
  int n_slices = 0;
  rc = sizes_check(w, n_stacks, lo_size, n_vol, &n_slices);
  if (rc != T2FIT_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(sums_dev) & 7) || (reinterpret_cast<uintptr_t>(weights_dev) & 7) ||
      (reinterpret_cast<uintptr_t>(sigma2_dev) & 7))
    return t2fit::fail(T2FIT_E_INVALID, w + ": sums_dev / weights_dev / sigma2_dev is not aligned to 8 bytes");
  RobustArgs a = {};
  int64_t blocks = 0;
  int slices = 0;
  for (int s = 0; s < n_stacks; ++s) {
    RobustStack& k = a.s[s];
    if (!r_dev[s] || !N_dev[s]) return t2fit::fail(T2FIT_E_INVALID, w + ": a residual or normaliser pointer is NULL");
    if ((reinterpret_cast<uintptr_t>(r_dev[s]) & 3) || (reinterpret_cast<uintptr_t>(N_dev[s]) & 7))
      return t2fit::fail(T2FIT_E_INVALID, w + ": a residual is not aligned to 4 bytes or a normaliser not to 8");
    k.r = r_dev[s], k.N = N_dev[s], k.mask = mask_dev ? mask_dev[s] : nullptr;
    k.lz = lo_size[3 * s];
    k.plane = (int64_t)lo_size[3 * s + 1] * lo_size[3 * s + 2];
    k.n_l = k.plane * k.lz;
    k.slice0 = slices, k.block0 = blocks;
    slices += k.lz;
    blocks += (k.n_l + kBlock - 1) / kBlock;
  }
  if (blocks > INT32_MAX) return t2fit::fail(T2FIT_E_INVALID, w + ": the stacks have more than 2^39 elements");
  a.sums = sums_dev, a.weights = weights_dev, a.sigma2 = sigma2_dev;
  a.tt = params->slice_threshold * params->slice_threshold;
  a.huber = params->huber;
  a.floor2 = params->sigma_floor * params->sigma_floor;
  a.n_stacks = n_stacks, a.n_vol = n_vol, a.n_slices = n_slices, a.min_count = params->min_count;
  const unsigned chunks = (unsigned)((n_vol + kRobustChunk - 1) / kRobustChunk);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sr_robust_sums_kernel, dim3((unsigned)n_slices, chunks), dim3(kBlock), 0, st, a);
  T2_HIP(hipGetLastError());
  hipLaunchKernelGGL(sr_robust_scale_kernel, dim3((unsigned)n_vol), dim3(kBlock), 0, st, a);
  T2_HIP(hipGetLastError());
  hipLaunchKernelGGL(sr_robust_apply_kernel, dim3((unsigned)blocks, chunks), dim3(kBlock), 0, st, a);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

}  // extern "C"

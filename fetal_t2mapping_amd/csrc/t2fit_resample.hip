// t2fit_resample.hip -- gfx950 kernels and C ABI of the orthogonal-stack reconstruction (include/t2fit.h:
// t2fit_resample_dev, t2fit_reconstruct_workspace_bytes, t2fit_reconstruct_dev).  Replaces steps 1 and 2 of the
// reference's run_qmri_reconstruction.py (utils/qmri_utils.py: resample_volume :62-80 through SimpleITK on the host,
// reconstruct_vol_trilinear :82-136 through scipy's RegularGridInterpolator) with the rigid transforms as an input.
//
// One definition of a sample (sample_linear / sample_nearest of t2fit_affine.h, restated in numpy in
// fetal_t2mapping_amd/_resample.py; the wrappers below form the coordinate and apply the pixel type's cast) serves three
// kernels here and t2fit_ffd.hip's warp:
//   resample_kernel     one stage: the output brick of a workgroup is walked along the output axis that maps most
//                       nearly onto the source's fastest axis, so that consecutive lanes read consecutive source
//                       elements whichever way the stack is oriented; the results cross an LDS tile and leave along
//                       output x.
//   merge_kernel        ((H_fixed + R_a) + R_b) / 3 in float64, the last link of the chain of single stages.
//   reconstruct_kernel  the fused form: the fixed stack's stage-1 sample plus, for each moving stack, a stage-2
//                       interpolation whose taps are stage-1 samples formed on the spot (rounded to float32 as the
//                       materialised intermediate would be): no intermediate volume touches memory.
// A weight that is exactly 0 skips the upper tap (part of the definition: an exact-node resample is the identity and
// an Inf next door stays next door).  The skip is a plain branch: when it holds for a whole wave -- axis-aligned stacks
// with 1 mm in-plane voxels -- the wave jumps over the loads, so 8 taps become 2 without a second code path.
// Compiled with -ffp-contract=off: every multiply and add below rounds once, as numpy's do.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "t2fit_affine.h"
#include "t2fit_error.h"
#include "t2fit_support.h"

namespace {

using t2fit::align_up, t2fit::ceil_div, t2fit::kBlock;
using t2fit::Affine, t2fit::Dims, t2fit::coord, t2fit::MemFetch, t2fit::finite12, t2fit::count_voxels;
constexpr int kPerThread = 2;
constexpr int kBrick = kBlock * kPerThread;  // voxels of a workgroup's output brick
constexpr size_t kAlign = 256;

__device__ inline float integer_cast(double r) {  // an int16 pixel type: toward zero, saturating; NaN stays NaN
  r = trunc(r);
  r = r < -32768.0 ? -32768.0 : r;
  r = r > 32767.0 ? 32767.0 : r;
  return (float)r;
}

// Linear sample of a volume of `n` at output index (ix, iy, iz): t2fit_affine.h's sample_linear at the index's image under A,
// then the pixel type's cast.  Outside the volume the result is default_value as it stands and nothing is fetched.
template <typename Fetch>
__device__ inline float sample_linear(const Fetch& fetch, const Dims n, const Affine& A, int ix, int iy, int iz, bool icast,
                                      float default_value) {
  double r;
  if (!t2fit::sample_linear(fetch, n, coord(A, 0, ix, iy, iz), coord(A, 1, ix, iy, iz), coord(A, 2, ix, iy, iz), r)) return default_value;
  return icast ? integer_cast(r) : (float)r;
}

__device__ inline uint32_t sample_nearest(const uint32_t* v, const Dims n, const Affine& A, int ix, int iy, int iz,
                                          uint32_t default_bits) {
  return t2fit::sample_nearest(v, n, coord(A, 0, ix, iy, iz), coord(A, 1, ix, iy, iz), coord(A, 2, ix, iy, iz), default_bits);
}

// ---- one stage -------------------------------------------------------------------------------------------------
// Brick of 512 output voxels.  LA = 0 (lanes along x: the source's fastest axis follows output x): 64 x 4 x 2, read order
// is write order.  LA = 1 / 2 (the source's fastest axis follows output y / z): 16 along x, 32 along that axis, 1 along
// the third; the reads walk the 32 (128 contiguous source bytes per run when the map is a permutation), the results cross
// a 32 x 17 LDS tile (stride 17: neither side conflicts) and the writes walk x in 64-byte runs.
template <int LA>
struct Brick {
  static constexpr int BX = LA == 0 ? 64 : 16;
  static constexpr int BY = LA == 0 ? 4 : (LA == 1 ? 32 : 1);
  static constexpr int BZ = LA == 0 ? 2 : (LA == 1 ? 1 : 32);
  static_assert(BX * BY * BZ == kBrick, "a brick is two voxels per thread");
};

struct ResampleArgs {
  const void* src;
  void* out;
  Dims n, o;
  Affine A;
  int bricks_x, bricks_y, bricks_per_vol;
  int nearest, icast;
  uint32_t default_bits;
};

template <int LA>
__global__ __launch_bounds__(kBlock) void resample_kernel(const ResampleArgs a) {
  using B = Brick<LA>;
  __shared__ uint32_t tile[LA == 0 ? 1 : 32 * 17];
  const int tid = threadIdx.x;
  const int vol = blockIdx.x / a.bricks_per_vol;
  int t = blockIdx.x % a.bricks_per_vol;
  const int bx = t % a.bricks_x;
  t /= a.bricks_x;
  const int by = t % a.bricks_y, bz = t / a.bricks_y;
  const int64_t n_src = (int64_t)a.n.nz * a.n.ny * a.n.nx, n_out = (int64_t)a.o.nz * a.o.ny * a.o.nx;
  const uint32_t* src = static_cast<const uint32_t*>(a.src) + vol * n_src;
  uint32_t* out = static_cast<uint32_t*>(a.out) + vol * n_out;
  const MemFetch fetch{reinterpret_cast<const float*>(src), a.n.ny, a.n.nx};
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int item = tid + k * kBlock;
    int lx, ly, lz;
    if constexpr (LA == 0) {
      lx = item % B::BX, ly = (item / B::BX) % B::BY, lz = item / (B::BX * B::BY);
    } else {
      const int l = item % 32;
      lx = item / 32, ly = LA == 1 ? l : 0, lz = LA == 2 ? l : 0;
    }
    const int x = bx * B::BX + lx, y = by * B::BY + ly, z = bz * B::BZ + lz;
    uint32_t bits = 0;
    if (x < a.o.nx && y < a.o.ny && z < a.o.nz)
      bits = a.nearest ? sample_nearest(src, a.n, a.A, x, y, z, a.default_bits)
                       : __float_as_uint(sample_linear(fetch, a.n, a.A, x, y, z, a.icast != 0, __uint_as_float(a.default_bits)));
    if constexpr (LA == 0) {
      if (x < a.o.nx && y < a.o.ny && z < a.o.nz) out[((int64_t)z * a.o.ny + y) * a.o.nx + x] = bits;
    } else {
      tile[(item % 32) * 17 + item / 32] = bits;
    }
  }
  if constexpr (LA != 0) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const int item = tid + k * kBlock;
      const int lx = item % 16, l = item / 16;
      const int x = bx * B::BX + lx, y = by * B::BY + (LA == 1 ? l : 0), z = bz * B::BZ + (LA == 2 ? l : 0);
      if (x < a.o.nx && y < a.o.ny && z < a.o.nz) out[((int64_t)z * a.o.ny + y) * a.o.nx + x] = tile[l * 17 + lx];
    }
  }
}

// ---- the merge of the chain ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void merge_kernel(float* out, const float* ra, const float* rb, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = (float)((((double)out[i] + (double)ra[i]) + (double)rb[i]) / 3.0);
}

// ---- the fused form --------------------------------------------------------------------------------------------
struct ReconArgs {
  const float* stack[3];  // [fixed, moving a, moving b], n_vol volumes each
  Dims lo[3], hi[3];      // the stacks and their stage-1 grids; hi[0] is the output grid
  Affine A1[3], A2[2];
  float* out;
  int bricks_x, bricks_y, bricks_per_vol;
  int icast;
};

// Brick 16 x 8 x 4, two voxels per thread, read order is write order: a wave covers 16 x and 4 y, so whichever axis a
// stack is thick along, the wave's taps fall into a handful of 64-byte runs of it, and the stores are 64-byte runs.
constexpr int kFX = 16, kFY = 8, kFZ = 4;
static_assert(kFX * kFY * kFZ == kBrick, "a brick is two voxels per thread");

__global__ __launch_bounds__(kBlock) void reconstruct_kernel(const ReconArgs a) {
  const int tid = threadIdx.x;
  const int vol = blockIdx.x / a.bricks_per_vol;
  int t = blockIdx.x % a.bricks_per_vol;
  const int bx = t % a.bricks_x;
  t /= a.bricks_x;
  const int by = t % a.bricks_y, bz = t / a.bricks_y;
  const bool icast = a.icast != 0;
  const Dims o = a.hi[0];
  float* out = a.out + (int64_t)vol * o.nz * o.ny * o.nx;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int item = tid + k * kBlock;
    const int x = bx * kFX + item % kFX, y = by * kFY + (item / kFX) % kFY, z = bz * kFZ + item / (kFX * kFY);
    if (!(x < o.nx && y < o.ny && z < o.nz)) continue;
    double sum = 0.0;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const Dims lo = a.lo[s];
      const MemFetch fetch{a.stack[s] + (int64_t)vol * lo.nz * lo.ny * lo.nx, lo.ny, lo.nx};
      float v;
      if (s == 0) {
        v = sample_linear(fetch, lo, a.A1[0], x, y, z, icast, 0.0f);
      } else {
        const Affine& A1 = a.A1[s];
        auto node = [&](int hx, int hy, int hz) { return (double)sample_linear(fetch, lo, A1, hx, hy, hz, icast, 0.0f); };
        v = sample_linear(node, a.hi[s], a.A2[s - 1], x, y, z, icast, 0.0f);
      }
      sum = s == 0 ? (double)v : sum + (double)v;
    }
    out[((int64_t)z * o.ny + y) * o.nx + x] = (float)(sum / 3.0);
  }
}

// ---- host --------------------------------------------------------------------------------------------------------
// the output axis whose step moves the source's x index most (ties: the lower axis)
int lane_axis(const double* A) {
  int best = 0;
  for (int a = 1; a < 3; ++a)
    if (std::fabs(A[a]) > std::fabs(A[best])) best = a;
  return best;
}

int resample_check(const std::string& w, const void* src, int src_type, int nz, int ny, int nx, const double* A, const void* out,
                   int oz, int oy, int ox, int n_vol, int interp, double default_value, int flags) {
  if (!src || !out || !A) return t2fit::fail(T2FIT_E_INVALID, w + ": src_dev / out_dev / A is NULL");
  if (src_type != T2FIT_RESAMPLE_F32 && src_type != T2FIT_RESAMPLE_I32)
    return t2fit::fail(T2FIT_E_INVALID, w + ": unknown src_type (T2FIT_RESAMPLE_F32 or T2FIT_RESAMPLE_I32)");
  if (interp != T2FIT_INTERP_LINEAR && interp != T2FIT_INTERP_NEAREST)
    return t2fit::fail(T2FIT_E_INVALID, w + ": unknown interp (T2FIT_INTERP_LINEAR or T2FIT_INTERP_NEAREST)");
  if (src_type == T2FIT_RESAMPLE_I32 && interp != T2FIT_INTERP_NEAREST)
    return t2fit::fail(T2FIT_E_INVALID, w + ": an int32 source is resampled with T2FIT_INTERP_NEAREST only");
  if (flags & ~T2FIT_RESAMPLE_INTEGER_CAST) return t2fit::fail(T2FIT_E_INVALID, w + ": flags has bits that are not defined");
  if ((flags & T2FIT_RESAMPLE_INTEGER_CAST) && interp != T2FIT_INTERP_LINEAR)
    return t2fit::fail(T2FIT_E_INVALID, w + ": T2FIT_RESAMPLE_INTEGER_CAST goes with T2FIT_INTERP_LINEAR");
  if (count_voxels(n_vol, nz, ny, nx) < 0 || count_voxels(n_vol, oz, oy, ox) < 0)
    return t2fit::fail(T2FIT_E_INVALID, w + ": n_vol and the sizes must all be >= 1 and a stack at most 2^40 elements");
  if (!finite12(A)) return t2fit::fail(T2FIT_E_INVALID, w + ": A has a non-finite entry");
  if (src_type == T2FIT_RESAMPLE_I32 && !(default_value >= -2147483648.0 && default_value <= 2147483647.0))
    return t2fit::fail(T2FIT_E_INVALID, w + ": default_value does not fit the int32 source");
  if ((reinterpret_cast<uintptr_t>(src) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
    return t2fit::fail(T2FIT_E_INVALID, w + ": src_dev / out_dev is not aligned to 4 bytes");
  if (src == out) return t2fit::fail(T2FIT_E_INVALID, w + ": out_dev must not be src_dev");
  return T2FIT_OK;
}

// queue one stage; the arguments have been checked
int resample_launch(const std::string& w, const void* src, int src_type, Dims n, const double* A, void* out, Dims o, int n_vol,
                    int interp, double default_value, int flags, hipStream_t st) {
  ResampleArgs a;
  a.src = src, a.out = out, a.n = n, a.o = o;
  for (int i = 0; i < 12; ++i) a.A.m[i] = A[i];
  a.nearest = interp == T2FIT_INTERP_NEAREST;
  a.icast = (flags & T2FIT_RESAMPLE_INTEGER_CAST) != 0;
  if (src_type == T2FIT_RESAMPLE_I32) {
    a.default_bits = (uint32_t)(int32_t)default_value;
  } else {
    const float f = (float)default_value;
    static_assert(sizeof(f) == sizeof(a.default_bits), "bit copy");
    __builtin_memcpy(&a.default_bits, &f, 4);
  }
  const int la = lane_axis(A);
  const int bxs = la == 0 ? Brick<0>::BX : 16, bys = la == 0 ? Brick<0>::BY : (la == 1 ? 32 : 1),
            bzs = la == 0 ? Brick<0>::BZ : (la == 2 ? 32 : 1);
  a.bricks_x = ceil_div(o.nx, bxs), a.bricks_y = ceil_div(o.ny, bys);
  const int64_t per_vol = (int64_t)a.bricks_x * a.bricks_y * ceil_div(o.nz, bzs);
  if (per_vol * n_vol > INT32_MAX)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the output has more than 2^31-1 bricks (the launch index is 32-bit)");
  a.bricks_per_vol = (int)per_vol;
  const dim3 grid((unsigned)(per_vol * n_vol)), block(kBlock);
  if (la == 0) hipLaunchKernelGGL(resample_kernel<0>, grid, block, 0, st, a);
  else if (la == 1) hipLaunchKernelGGL(resample_kernel<1>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(resample_kernel<2>, grid, block, 0, st, a);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

struct ReconPlan {
  int64_t n_lo[3], n_hi[3];  // voxels of all n_vol volumes
  size_t h_bytes[3], chain_total;
};

int recon_plan(const std::string& w, int n_vol, const int32_t* lo_size, const int32_t* hi_size, int flags, ReconPlan* plan) {
  if (!lo_size || !hi_size) return t2fit::fail(T2FIT_E_INVALID, w + ": lo_size / hi_size is NULL");
  if (flags & ~(T2FIT_RESAMPLE_INTEGER_CAST | T2FIT_RECON_CHAIN))
    return t2fit::fail(T2FIT_E_INVALID, w + ": flags has bits that are not defined");
  for (int s = 0; s < 3; ++s) {
    plan->n_lo[s] = count_voxels(n_vol, lo_size[3 * s], lo_size[3 * s + 1], lo_size[3 * s + 2]);
    plan->n_hi[s] = count_voxels(n_vol, hi_size[3 * s], hi_size[3 * s + 1], hi_size[3 * s + 2]);
    if (plan->n_lo[s] < 0 || plan->n_hi[s] < 0)
      return t2fit::fail(T2FIT_E_INVALID, w + ": n_vol and the sizes must all be >= 1 and a stack at most 2^40 elements");
    plan->h_bytes[s] = align_up((size_t)plan->n_hi[s] * 4, kAlign);
  }
  plan->chain_total = plan->h_bytes[1] + plan->h_bytes[2] + 2 * plan->h_bytes[0];
  return T2FIT_OK;
}

}  // namespace

extern "C" {

int t2fit_resample_dev(const void* src_dev, int src_type, int nz, int ny, int nx, const double* A, void* out_dev, int oz, int oy,
                       int ox, int n_vol, int interp, double default_value, int flags, void* stream) {
  const std::string w("t2fit_resample_dev");
  const int rc = resample_check(w, src_dev, src_type, nz, ny, nx, A, out_dev, oz, oy, ox, n_vol, interp, default_value, flags);
  if (rc != T2FIT_OK) return rc;
  return resample_launch(w, src_dev, src_type, Dims{nz, ny, nx}, A, out_dev, Dims{oz, oy, ox}, n_vol, interp, default_value, flags,
                         (hipStream_t)stream);
}

int t2fit_reconstruct_workspace_bytes(int n_vol, const int32_t* lo_size, const int32_t* hi_size, int flags, size_t* bytes) {
  if (!bytes) return t2fit::fail(T2FIT_E_INVALID, "t2fit_reconstruct_workspace_bytes: bytes is NULL");
  ReconPlan plan;
  const int rc = recon_plan("t2fit_reconstruct_workspace_bytes", n_vol, lo_size, hi_size, flags, &plan);
  if (rc != T2FIT_OK) return rc;
  *bytes = (flags & T2FIT_RECON_CHAIN) ? plan.chain_total : 0;
  return T2FIT_OK;
}

int t2fit_reconstruct_dev(const float* const* stacks_dev, const int32_t* lo_size, const double* A1, const int32_t* hi_size,
                          const double* A2, float* out_dev, int n_vol, int flags, void* workspace_dev, size_t workspace_bytes,
                          void* stream) {
  const std::string w("t2fit_reconstruct_dev");
  if (!stacks_dev || !A1 || !A2 || !out_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": stacks_dev / A1 / A2 / out_dev is NULL");
  ReconPlan plan;
  const int rc = recon_plan(w, n_vol, lo_size, hi_size, flags, &plan);
  if (rc != T2FIT_OK) return rc;
  for (int s = 0; s < 3; ++s) {
    if (!stacks_dev[s]) return t2fit::fail(T2FIT_E_INVALID, w + ": a stack pointer is NULL");
    if ((reinterpret_cast<uintptr_t>(stacks_dev[s]) & 3) || stacks_dev[s] == out_dev)
      return t2fit::fail(T2FIT_E_INVALID, w + ": a stack pointer is not aligned to 4 bytes or is out_dev");
    if (!finite12(A1 + 12 * s) || (s < 2 && !finite12(A2 + 12 * s)))
      return t2fit::fail(T2FIT_E_INVALID, w + ": A1 / A2 has a non-finite entry");
  }
  if (reinterpret_cast<uintptr_t>(out_dev) & 3) return t2fit::fail(T2FIT_E_INVALID, w + ": out_dev is not aligned to 4 bytes");
  const bool chain = (flags & T2FIT_RECON_CHAIN) != 0;
  if (chain) {
    if (!workspace_dev) return t2fit::fail(T2FIT_E_INVALID, w + ": T2FIT_RECON_CHAIN needs workspace_dev");
    const int ws_rc = t2fit::check_workspace(w, workspace_dev, workspace_bytes, plan.chain_total, "t2fit_reconstruct_workspace_bytes");
    if (ws_rc != T2FIT_OK) return ws_rc;
  }
  Dims lo[3], hi[3];
  for (int s = 0; s < 3; ++s) {
    lo[s] = Dims{lo_size[3 * s], lo_size[3 * s + 1], lo_size[3 * s + 2]};
    hi[s] = Dims{hi_size[3 * s], hi_size[3 * s + 1], hi_size[3 * s + 2]};
  }
  hipStream_t st = (hipStream_t)stream;
  const int cast_flag = flags & T2FIT_RESAMPLE_INTEGER_CAST;
  if (chain) {
    // H_fixed goes straight into out; H_a, H_b, R_a, R_b live in the workspace
    char* ws = static_cast<char*>(workspace_dev);
    float* h[3] = {out_dev, reinterpret_cast<float*>(ws), reinterpret_cast<float*>(ws + plan.h_bytes[1])};
    float* r[2] = {reinterpret_cast<float*>(ws + plan.h_bytes[1] + plan.h_bytes[2]),
                   reinterpret_cast<float*>(ws + plan.h_bytes[1] + plan.h_bytes[2] + plan.h_bytes[0])};
    for (int s = 0; s < 3; ++s) {
      const int e = resample_launch(w, stacks_dev[s], T2FIT_RESAMPLE_F32, lo[s], A1 + 12 * s, h[s], hi[s], n_vol,
                                    T2FIT_INTERP_LINEAR, 0.0, cast_flag, st);
      if (e != T2FIT_OK) return e;
    }
    for (int m = 0; m < 2; ++m) {
      const int e = resample_launch(w, h[m + 1], T2FIT_RESAMPLE_F32, hi[m + 1], A2 + 12 * m, r[m], hi[0], n_vol,
                                    T2FIT_INTERP_LINEAR, 0.0, cast_flag, st);
      if (e != T2FIT_OK) return e;
    }
    const int64_t n = plan.n_hi[0];
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    if (blocks > INT32_MAX) return t2fit::fail(T2FIT_E_INVALID, w + ": the output has more than 2^39 elements");
    hipLaunchKernelGGL(merge_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, out_dev, (const float*)r[0], (const float*)r[1], n);
    T2_HIP(hipGetLastError());
    return T2FIT_OK;
  }
  ReconArgs a;
  for (int s = 0; s < 3; ++s) {
    a.stack[s] = stacks_dev[s], a.lo[s] = lo[s], a.hi[s] = hi[s];
    for (int i = 0; i < 12; ++i) a.A1[s].m[i] = A1[12 * s + i];
    if (s < 2)
      for (int i = 0; i < 12; ++i) a.A2[s].m[i] = A2[12 * s + i];
  }
  a.out = out_dev;
  a.icast = cast_flag != 0;
  a.bricks_x = ceil_div(hi[0].nx, kFX), a.bricks_y = ceil_div(hi[0].ny, kFY);
  const int64_t per_vol = (int64_t)a.bricks_x * a.bricks_y * ceil_div(hi[0].nz, kFZ);
  if (per_vol * n_vol > INT32_MAX)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the output has more than 2^31-1 bricks (the launch index is 32-bit)");
  a.bricks_per_vol = (int)per_vol;
  hipLaunchKernelGGL(reconstruct_kernel, dim3((unsigned)(per_vol * n_vol)), dim3(kBlock), 0, st, a);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

}  // extern "C"

// t2fit_denoise.hip -- gfx950 kernels and C ABI of the total-variation denoiser of the echo stack (include/t2fit.h:
// t2fit_tv_params_default, t2fit_tv_workspace_bytes, t2fit_tv_denoise_dev).  Replaces the host loop of the reference's
// run_denoising (utils/qmri_utils.py:393-405: skimage.restoration.denoise_tv_chambolle on every slice of every echo).
//
// Chambolle's projection iteration keeps one dual field p_a per axis.  One *pass* kernel per iteration reads f and the
// old p and writes the new p into the other half of a ping-pong pair (new p[x] needs old p at x, x + e_a and their
// - e_b neighbours, so nothing is updated in place) and leaves two float64 partial energies per tile; a small *reduce*
// kernel folds the partials of every problem in a fixed tree and applies the stop rule to the per-problem state on the
// device.  Workgroups of a finished problem return at once, so the half of the pair its result lives in stays intact;
// a *finish* kernel writes out = f + d from that half, once.  `out` never touches memory in between.
// Traffic per voxel and iteration: 4 B of f, dims reads and dims writes of p (20 B in 2-D, 28 B in 3-D, float32).
// Nothing here shares a header with the fit kernels except the error plumbing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "t2fit_error.h"
#include "t2fit_support.h"

namespace {

using t2fit::align_up, t2fit::kBlock;
constexpr int kWaves = kBlock / 64;
// A workgroup owns a tile of kTZ x kTY x kTX voxels (x innermost; 2-D: 1 x 32 x 64, 3-D: 4 x 8 x 64), 512 quads of four
// consecutive x: two per thread.  `out` of the tile and of its upper halo (the points x + e_a) is staged in LDS; the
// thread keeps d, out and the old p of its own quads in registers.
constexpr int kTX = 64;
constexpr int kQX = kTX / 4;
constexpr int kRow = kTX + 4;  // entry kTX is the x halo; rows stay 16-byte aligned
constexpr int kQuadsPerThread = 2;
constexpr size_t kAlign = 256;

template <int DIMS>
struct Tile {
  static constexpr int TY = DIMS == 2 ? 32 : 8;
  static constexpr int TZ = DIMS == 2 ? 1 : 4;
  static constexpr int RowsY = TY + 1;
  static constexpr int RowsZ = DIMS == 2 ? 1 : TZ + 1;
  static constexpr int Quads = TZ * TY * kQX;
  static_assert(Quads == kBlock * kQuadsPerThread, "two quads per thread");
};

struct TvState {  // one per problem, written by tv_reduce_kernel only
  double e_init, e_prev, e_last;
  int32_t done, n_iter;
};
static_assert(sizeof(TvState) == 32, "documented in include/t2fit.h");

struct TvArgs {
  const float* f;      // the stack, problems contiguous
  int nz, ny, nx;      // one problem (nz = 1 in 2-D)
  int tiles_x, tiles_y, tiles_per_problem;
  int vec;             // nx % 4 == 0 and f is 16-byte aligned: 128-bit accesses
  int64_t n_problem;   // voxels of one problem
  int64_t n_total;     // voxels of the stack: distance between the p fields of one half
};

template <typename T>
__device__ inline void load4(const T* p, T (&v)[4]) {
  if constexpr (sizeof(T) == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
    v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
  }
}

template <typename T>
__device__ inline void store4(T* p, const T (&v)[4]) {
  if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
    *reinterpret_cast<double2*>(p + 2) = make_double2(v[2], v[3]);
  }
}

// four consecutive x of a row starting at element `off` (x is the first; elements at or beyond nx read as 0)
template <typename T, typename S>
__device__ inline void load_quad(const S* base, int64_t off, int x, int nx, bool vec, T (&v)[4]) {
  if (vec) {
    S t[4];
    load4(base + off, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (T)t[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = x + j < nx ? (T)base[off + j] : (T)0;
  }
}

template <typename T>
__device__ inline void store_quad(T* base, int64_t off, int x, int nx, bool vec, const T (&v)[4]) {
  if (vec) {
    store4(base + off, v);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x + j < nx) base[off + j] = v[j];
  }
}

// sqrt and / of the language: hipcc rounds both correctly for float32 as well (its default
// -fhip-fp32-correctly-rounded-divide-sqrt; the __fsqrt_rn / __fdiv_rn intrinsics are the fast ones in this toolchain)
template <typename T>
__device__ inline T sqrt_rn(T v) {
  if constexpr (sizeof(T) == 4) return __builtin_sqrtf(v);
  else return __builtin_sqrt(v);
}

template <typename T>
__device__ inline T div_rn(T a, T b) {
  return a / b;
}

// d = ((-(p_0 + .. + p_{n-1})) + p_0[x - e_0]) + p_1[x - e_1] .. of four consecutive voxels, a term dropped where
// x - e_a is outside; axis order Z, Y, X (2-D: Y, X).  `own` receives p_a at the voxels themselves.  (z, y, x) inside.
template <typename T, int DIMS>
__device__ inline void d_quad(const TvArgs& a, const T* __restrict__ p, int64_t off, int z, int y, int x, T (&own)[DIMS][4],
                              T (&d)[4]) {
  const bool vec = a.vec != 0;
#pragma unroll
  for (int ax = 0; ax < DIMS; ++ax) load_quad<T, T>(p + ax * a.n_total, off, x, a.nx, vec, own[ax]);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    T s = own[0][j] + own[1][j];
    if constexpr (DIMS == 3) s = s + own[2][j];
    d[j] = -s;
  }
  int ax = 0;
  if constexpr (DIMS == 3) {
    if (z > 0) {
      T up[4];
      load_quad<T, T>(p, off - (int64_t)a.ny * a.nx, x, a.nx, vec, up);
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = d[j] + up[j];
    }
    ax = 1;
  }
  if (y > 0) {
    T up[4];
    load_quad<T, T>(p + ax * a.n_total, off - a.nx, x, a.nx, vec, up);
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = d[j] + up[j];
  }
  const T* px = p + (ax + 1) * a.n_total;
  if (x > 0) d[0] = d[0] + px[off - 1];
#pragma unroll
  for (int j = 1; j < 4; ++j) d[j] = d[j] + own[ax + 1][j - 1];
}

// out = f + d of four consecutive voxels (FIRST: p = 0 and d = 0, nothing of p is read)
template <typename T, int DIMS, bool FIRST>
__device__ inline void out_quad(const TvArgs& a, const float* __restrict__ f, const T* __restrict__ p, int64_t off, int z, int y,
                                int x, T (&own)[DIMS][4], T (&d)[4], T (&out)[4]) {
  T fv[4];
  load_quad<T, float>(f, off, x, a.nx, a.vec != 0, fv);
  if constexpr (FIRST) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      d[j] = (T)0;
#pragma unroll
      for (int ax = 0; ax < DIMS; ++ax) own[ax][j] = (T)0;
    }
  } else {
    d_quad<T, DIMS>(a, p, off, z, y, x, own, d);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = fv[j] + d[j];
}

// the same for one voxel (the x halo of a tile)
template <typename T, int DIMS, bool FIRST>
__device__ inline T out_point(const TvArgs& a, const float* __restrict__ f, const T* __restrict__ p, int64_t off, int z, int y,
                              int x) {
  T d = (T)0;
  if constexpr (!FIRST) {
    T s = p[off] + p[a.n_total + off];
    if constexpr (DIMS == 3) s = s + p[2 * a.n_total + off];
    d = -s;
    int ax = 0;
    if constexpr (DIMS == 3) {
      if (z > 0) d = d + p[off - (int64_t)a.ny * a.nx];
      ax = 1;
    }
    if (y > 0) d = d + p[ax * a.n_total + off - a.nx];
    if (x > 0) d = d + p[(ax + 1) * a.n_total + off - 1];
  }
  return (T)f[off] + d;
}

__device__ inline double wave_sum(double v) {  // fixed butterfly: the same bits on every launch
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// One iteration.  p_old is not read when FIRST; p_new = (p_old - tau g) / (1 + (tau / weight) |g|) with g the forward
// differences of out = f + d.  partial[2 * tile] = sum d^2, partial[2 * tile + 1] = sum |g| over the tile, float64.
template <typename T, int DIMS, bool FIRST>
__global__ __launch_bounds__(kBlock) void tv_pass_kernel(const TvArgs a, const T* __restrict__ p_old, T* __restrict__ p_new,
                                                         const TvState* __restrict__ state, double* __restrict__ partial,
                                                         T tau, T tau_over_weight) {
  using G = Tile<DIMS>;
  __shared__ __attribute__((aligned(16))) T lds_out[G::RowsZ * G::RowsY * kRow];
  __shared__ double lds_sum[2 * kWaves];
  const int tid = threadIdx.x;
  const int problem = blockIdx.x / a.tiles_per_problem;
  if (!FIRST && state[problem].done) return;
  int t = blockIdx.x - problem * a.tiles_per_problem;
  const int bx = t % a.tiles_x;
  t /= a.tiles_x;
  const int by = t % a.tiles_y, bz = t / a.tiles_y;
  const int x0 = bx * kTX, y0 = by * G::TY, z0 = bz * G::TZ;
  const int64_t base = (int64_t)problem * a.n_problem;
  const float* f = a.f + base;
  const T* po = FIRST ? nullptr : p_old + base;
  T* pn = p_new + base;
  const bool vec = a.vec != 0;

  T own[kQuadsPerThread][DIMS][4], out[kQuadsPerThread][4];
  double sum_d = 0.0, sum_n = 0.0;
#pragma unroll
  for (int k = 0; k < kQuadsPerThread; ++k) {
    const int item = tid + k * kBlock;
    const int q = item % kQX, ly = (item / kQX) % G::TY, lz = item / (kQX * G::TY);
    const int x = x0 + 4 * q, y = y0 + ly, z = z0 + lz;
    if (x < a.nx && y < a.ny && z < a.nz) {
      const int64_t off = ((int64_t)z * a.ny + y) * a.nx + x;
      T d[4];
      out_quad<T, DIMS, FIRST>(a, f, po, off, z, y, x, own[k], d, out[k]);
      if constexpr (!FIRST) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x + j < a.nx) sum_d += (double)(d[j] * d[j]);
      }
      store4(lds_out + (lz * G::RowsY + ly) * kRow + 4 * q, out[k]);
    }
  }
  // the upper halo: row ly = TY of every lz, plane lz = TZ (3-D), column lx = TX; a point outside the problem is skipped
  // (its difference is 0 and it is never read)
  constexpr int kHaloY = G::TZ * kQX, kHaloZ = DIMS == 3 ? G::TY * kQX : 0, kHaloX = G::TZ * G::TY;
  for (int item = tid; item < kHaloY + kHaloZ + kHaloX; item += kBlock) {
    if (item < kHaloY + kHaloZ) {
      int q, ly, lz;
      if (item < kHaloY) {
        q = item % kQX, lz = item / kQX, ly = G::TY;
      } else {
        q = (item - kHaloY) % kQX, ly = (item - kHaloY) / kQX, lz = G::TZ;
      }
      const int x = x0 + 4 * q, y = y0 + ly, z = z0 + lz;
      if (x < a.nx && y < a.ny && z < a.nz) {
        T o[DIMS][4], d[4], v[4];
        out_quad<T, DIMS, FIRST>(a, f, po, ((int64_t)z * a.ny + y) * a.nx + x, z, y, x, o, d, v);
        store4(lds_out + (lz * G::RowsY + ly) * kRow + 4 * q, v);
      }
    } else {
      const int r = item - kHaloY - kHaloZ;
      const int ly = r % G::TY, lz = r / G::TY;
      const int x = x0 + kTX, y = y0 + ly, z = z0 + lz;
      if (x < a.nx && y < a.ny && z < a.nz)
        lds_out[(lz * G::RowsY + ly) * kRow + kTX] =
            out_point<T, DIMS, FIRST>(a, f, po, ((int64_t)z * a.ny + y) * a.nx + x, z, y, x);
    }
  }
  __syncthreads();

#pragma unroll
  for (int k = 0; k < kQuadsPerThread; ++k) {
    const int item = tid + k * kBlock;
    const int q = item % kQX, ly = (item / kQX) % G::TY, lz = item / (kQX * G::TY);
    const int x = x0 + 4 * q, y = y0 + ly, z = z0 + lz;
    if (x < a.nx && y < a.ny && z < a.nz) {
      const int64_t off = ((int64_t)z * a.ny + y) * a.nx + x;
      const T* c = lds_out + (lz * G::RowsY + ly) * kRow + 4 * q;
      T g[DIMS][4];
      int ax = 0;
      if constexpr (DIMS == 3) {
        if (z + 1 < a.nz) {
          T n[4];
          load4(c + G::RowsY * kRow, n);
#pragma unroll
          for (int j = 0; j < 4; ++j) g[0][j] = n[j] - out[k][j];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) g[0][j] = (T)0;
        }
        ax = 1;
      }
      if (y + 1 < a.ny) {
        T n[4];
        load4(c + kRow, n);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[ax][j] = n[j] - out[k][j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[ax][j] = (T)0;
      }
      const T right = x + 4 < a.nx ? c[4] : (T)0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const T nb = j < 3 ? out[k][j < 3 ? j + 1 : 3] : right;
        g[ax + 1][j] = x + j + 1 < a.nx ? nb - out[k][j] : (T)0;
      }
      T upd[DIMS][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        T sq = g[0][j] * g[0][j] + g[1][j] * g[1][j];
        if constexpr (DIMS == 3) sq = sq + g[2][j] * g[2][j];
        const T nrm = sqrt_rn(sq);
        if (x + j < a.nx) sum_n += (double)nrm;
        const T den = (T)1 + tau_over_weight * nrm;
#pragma unroll
        for (int b = 0; b < DIMS; ++b) upd[b][j] = div_rn(own[k][b][j] - tau * g[b][j], den);
      }
#pragma unroll
      for (int b = 0; b < DIMS; ++b) store_quad(pn + b * a.n_total, off, x, a.nx, vec, upd[b]);
    }
  }

  sum_d = wave_sum(sum_d);
  sum_n = wave_sum(sum_n);
  if ((tid & 63) == 0) {
    lds_sum[2 * (tid >> 6)] = sum_d;
    lds_sum[2 * (tid >> 6) + 1] = sum_n;
  }
  __syncthreads();
  if (tid == 0) {
    double sd = lds_sum[0], sn = lds_sum[1];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) sd += lds_sum[2 * w], sn += lds_sum[2 * w + 1];
    partial[2 * (int64_t)blockIdx.x] = sd;
    partial[2 * (int64_t)blockIdx.x + 1] = sn;
  }
}

// After pass `iter`: one wave per problem sums its tiles' partials (lane l takes tiles l, l + 64, .. in order, then the
// fixed butterfly) and applies the stop rule.  n_iter = iter at a stop, max_iter - 1 when the loop runs out.
__global__ __launch_bounds__(64) void tv_reduce_kernel(const double* __restrict__ partial, TvState* __restrict__ state,
                                                       int tiles_per_problem, double n_problem, double weight, double eps, int iter,
                                                       int max_iter) {
  const int problem = blockIdx.x;
  TvState* s = state + problem;
  if (iter > 0 && s->done) return;
  const double* part = partial + 2 * (int64_t)problem * tiles_per_problem;
  double sd = 0.0, sn = 0.0;
  for (int t = threadIdx.x; t < tiles_per_problem; t += 64) sd += part[2 * t], sn += part[2 * t + 1];
  sd = wave_sum(sd);
  sn = wave_sum(sn);
  if (threadIdx.x != 0) return;
  const double e = (sd + weight * sn) / n_problem;
  int done = 0;
  if (iter == 0) {
    s->e_init = e;
    s->e_prev = e;
  } else if (fabs(s->e_prev - e) < eps * s->e_init) {
    done = 1;
  } else {
    s->e_prev = e;
  }
  if (iter == max_iter - 1) done = 1;
  s->e_last = e;
  s->n_iter = iter;
  s->done = done;
}

// The result: out = f + d from the half of the pair that iteration n_iter read (d = 0 when n_iter = 0), rounded to
// float32 once.  A thread reads f only at the voxels it writes, so `dst` may be the stack itself.
template <typename T, int DIMS>
__global__ __launch_bounds__(kBlock) void tv_finish_kernel(const TvArgs a, const T* __restrict__ p_even, const T* __restrict__ p_odd,
                                                           const TvState* __restrict__ state, float* dst,
                                                           int32_t* __restrict__ n_iter_out, double* __restrict__ energy_out) {
  using G = Tile<DIMS>;
  const int tid = threadIdx.x;
  const int problem = blockIdx.x / a.tiles_per_problem;
  int t = blockIdx.x - problem * a.tiles_per_problem;
  const int n_iter = state[problem].n_iter;
  if (t == 0 && tid == 0) {
    if (n_iter_out) n_iter_out[problem] = n_iter;
    if (energy_out) energy_out[problem] = state[problem].e_last;
  }
  const int bx = t % a.tiles_x;
  t /= a.tiles_x;
  const int by = t % a.tiles_y, bz = t / a.tiles_y;
  const int64_t base = (int64_t)problem * a.n_problem;
  const float* f = a.f + base;
  const T* p = ((n_iter & 1) ? p_odd : p_even) + base;
  const bool dst_vec = a.vec && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
#pragma unroll
  for (int k = 0; k < kQuadsPerThread; ++k) {
    const int item = tid + k * kBlock;
    const int q = item % kQX, ly = (item / kQX) % G::TY, lz = item / (kQX * G::TY);
    const int x = bx * kTX + 4 * q, y = by * G::TY + ly, z = bz * G::TZ + lz;
    if (x < a.nx && y < a.ny && z < a.nz) {
      const int64_t off = ((int64_t)z * a.ny + y) * a.nx + x;
      T own[DIMS][4], d[4], out[4];
      if (n_iter == 0) out_quad<T, DIMS, true>(a, f, p, off, z, y, x, own, d, out);
      else out_quad<T, DIMS, false>(a, f, p, off, z, y, x, own, d, out);
      float r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = (float)out[j];
      store_quad(dst + base, off, x, a.nx, dst_vec, r);
    }
  }
}

struct TvPlan {
  int64_t n_problems, n_problem, n_total, tiles_per_problem, n_tiles;
  int pnz, tiles_x, tiles_y;
  size_t elem, field_bytes, partial_bytes, state_bytes, total;
};

// argument checks and workspace arithmetic shared by the size query and the call; no HIP
int tv_plan(const char* who, const t2fit_tv_params* p, int n_vol, int nz, int ny, int nx, TvPlan* plan) {
  const std::string w(who);
  if (!p) return t2fit::fail(T2FIT_E_INVALID, w + ": params is NULL");
  if (!(p->weight > 0.0) || !std::isfinite(p->weight)) return t2fit::fail(T2FIT_E_INVALID, w + ": weight must be finite and > 0");
  if (!(p->eps >= 0.0) || !std::isfinite(p->eps)) return t2fit::fail(T2FIT_E_INVALID, w + ": eps must be finite and >= 0");
  if (p->max_iter < 1) return t2fit::fail(T2FIT_E_INVALID, w + ": max_iter must be >= 1");
  if (p->dims != 2 && p->dims != 3) return t2fit::fail(T2FIT_E_INVALID, w + ": dims must be 2 or 3");
  if (p->precision != T2FIT_PREC_F32 && p->precision != T2FIT_PREC_F64)
    return t2fit::fail(T2FIT_E_INVALID, w + ": unknown precision (T2FIT_PREC_F32 or T2FIT_PREC_F64)");
  if (p->flags != 0) return t2fit::fail(T2FIT_E_INVALID, w + ": flags is reserved and must be 0");
  if (n_vol < 1 || nz < 1 || ny < 1 || nx < 1)
    return t2fit::fail(T2FIT_E_INVALID, w + ": n_vol, nz, ny, nx must all be >= 1");
  const int64_t n_total = (int64_t)n_vol * nz * ny * nx;  // four factors below 2^31: compare before the last product
  if ((int64_t)n_vol * nz > (int64_t)1 << 31 || (int64_t)ny * nx > (int64_t)1 << 31 || (int64_t)n_vol * nz > ((int64_t)1 << 40) / ((int64_t)ny * nx))
    return t2fit::fail(T2FIT_E_INVALID, w + ": the stack has more than 2^40 elements");
  plan->n_total = n_total;
  plan->n_problems = p->dims == 2 ? (int64_t)n_vol * nz : n_vol;
  plan->n_problem = n_total / plan->n_problems;
  plan->pnz = p->dims == 2 ? 1 : nz;
  const int ty = p->dims == 2 ? Tile<2>::TY : Tile<3>::TY, tz = p->dims == 2 ? Tile<2>::TZ : Tile<3>::TZ;
  plan->tiles_x = (nx + kTX - 1) / kTX;
  plan->tiles_y = (ny + ty - 1) / ty;
  plan->tiles_per_problem = (int64_t)plan->tiles_x * plan->tiles_y * ((plan->pnz + tz - 1) / tz);
  plan->n_tiles = plan->tiles_per_problem * plan->n_problems;
  if (plan->tiles_per_problem > INT32_MAX || plan->n_tiles > INT32_MAX)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the stack has more than 2^31-1 tiles (the launch index is 32-bit)");
  plan->elem = p->precision == T2FIT_PREC_F32 ? 4 : 8;
  plan->field_bytes = align_up((size_t)p->dims * (size_t)n_total * plan->elem, kAlign);
  plan->partial_bytes = align_up((size_t)plan->n_tiles * 16, kAlign);
  plan->state_bytes = align_up((size_t)plan->n_problems * sizeof(TvState), kAlign);
  plan->total = 2 * plan->field_bytes + plan->partial_bytes + plan->state_bytes;
  return T2FIT_OK;
}

template <typename T, int DIMS>
int tv_run(const t2fit_tv_params* p, const TvPlan& plan, const TvArgs& a, float* out_dev, char* ws, int32_t* n_iter_dev,
           double* energy_dev, hipStream_t st) {
  T* half[2] = {reinterpret_cast<T*>(ws), reinterpret_cast<T*>(ws + plan.field_bytes)};
  double* partial = reinterpret_cast<double*>(ws + 2 * plan.field_bytes);
  TvState* state = reinterpret_cast<TvState*>(ws + 2 * plan.field_bytes + plan.partial_bytes);
  const double tau = 1.0 / (2.0 * DIMS);
  const T tau_t = (T)tau, tw_t = (T)(tau / p->weight);
  const dim3 grid((unsigned)plan.n_tiles), block(kBlock);
  for (int i = 0; i < p->max_iter; ++i) {
    // iteration i reads half i % 2 and writes the other one
    if (i == 0)
      hipLaunchKernelGGL((tv_pass_kernel<T, DIMS, true>), grid, block, 0, st, a, (const T*)half[0], half[1],
                         (const TvState*)state, partial, tau_t, tw_t);
    else
      hipLaunchKernelGGL((tv_pass_kernel<T, DIMS, false>), grid, block, 0, st, a, (const T*)half[i & 1], half[(i + 1) & 1],
                         (const TvState*)state, partial, tau_t, tw_t);
    hipLaunchKernelGGL(tv_reduce_kernel, dim3((unsigned)plan.n_problems), dim3(64), 0, st, (const double*)partial, state,
                       (int)plan.tiles_per_problem, (double)plan.n_problem, p->weight, p->eps, i, p->max_iter);
  }
  hipLaunchKernelGGL((tv_finish_kernel<T, DIMS>), grid, block, 0, st, a, (const T*)half[0], (const T*)half[1],
                     (const TvState*)state, out_dev, n_iter_dev, energy_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

// ---- vector-valued (joint) TV across the channels of a stack (include/t2fit.h: t2fit_tv_joint_denoise_dev) -----------
// The channels of a problem keep a dual field each and share one norm per voxel, sqrt(sum_c |g_c|^2), which needs the
// differences of every channel before any p is updated.  A workgroup owns a spatial tile for all channels and loops them
// twice over the one LDS tile: sweep 1 stages out_c with its halo, ascending, and accumulates S (per voxel, registers)
// and sum d^2; sweep 2 forms the shared denominator once, then re-stages out_c, descending, and writes the new p_c.  The
// last channel of sweep 1 is the first of sweep 2 and is staged once: its tile, out and old p are still in place.
// Channel c of problem k starts at k * n_problem + c * chan_stride in the stack and in every p field (a p field is laid
// out like the stack, fields n_total apart), so the scalar kernel's quad / point helpers are used as they are.
template <typename T, int DIMS, bool FIRST>
__device__ inline void tvj_stage(const TvArgs& a, const float* __restrict__ f, const T* __restrict__ po, int tid, int x0, int y0,
                                 int z0, T* __restrict__ lds_out, T (&own)[kQuadsPerThread][DIMS][4], T (&out)[kQuadsPerThread][4],
                                 bool energy, double& sum_d) {
  using G = Tile<DIMS>;
#pragma unroll
  for (int k = 0; k < kQuadsPerThread; ++k) {
    const int item = tid + k * kBlock;
    const int q = item % kQX, ly = (item / kQX) % G::TY, lz = item / (kQX * G::TY);
    const int x = x0 + 4 * q, y = y0 + ly, z = z0 + lz;
    if (x < a.nx && y < a.ny && z < a.nz) {
      const int64_t off = ((int64_t)z * a.ny + y) * a.nx + x;
      T d[4];
      out_quad<T, DIMS, FIRST>(a, f, po, off, z, y, x, own[k], d, out[k]);
      if constexpr (!FIRST) {
        if (energy) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (x + j < a.nx) sum_d += (double)(d[j] * d[j]);
        }
      }
      store4(lds_out + (lz * G::RowsY + ly) * kRow + 4 * q, out[k]);
    }
  }
  // the upper halo, as tv_pass_kernel fetches it
  constexpr int kHaloY = G::TZ * kQX, kHaloZ = DIMS == 3 ? G::TY * kQX : 0, kHaloX = G::TZ * G::TY;
  for (int item = tid; item < kHaloY + kHaloZ + kHaloX; item += kBlock) {
    if (item < kHaloY + kHaloZ) {
      int q, ly, lz;
      if (item < kHaloY) {
        q = item % kQX, lz = item / kQX, ly = G::TY;
      } else {
        q = (item - kHaloY) % kQX, ly = (item - kHaloY) / kQX, lz = G::TZ;
      }
      const int x = x0 + 4 * q, y = y0 + ly, z = z0 + lz;
      if (x < a.nx && y < a.ny && z < a.nz) {
        T o[DIMS][4], d[4], v[4];
        out_quad<T, DIMS, FIRST>(a, f, po, ((int64_t)z * a.ny + y) * a.nx + x, z, y, x, o, d, v);
        store4(lds_out + (lz * G::RowsY + ly) * kRow + 4 * q, v);
      }
    } else {
      const int r = item - kHaloY - kHaloZ;
      const int ly = r % G::TY, lz = r / G::TY;
      const int x = x0 + kTX, y = y0 + ly, z = z0 + lz;
      if (x < a.nx && y < a.ny && z < a.nz)
        lds_out[(lz * G::RowsY + ly) * kRow + kTX] =
            out_point<T, DIMS, FIRST>(a, f, po, ((int64_t)z * a.ny + y) * a.nx + x, z, y, x);
    }
  }
}

// the forward differences of four consecutive voxels from the staged tile (c: the quad's own entry), 0 past the problem
template <typename T, int DIMS>
__device__ inline void tvj_grad(const TvArgs& a, const T* __restrict__ c, const T (&out)[4], int z, int y, int x, T (&g)[DIMS][4]) {
  using G = Tile<DIMS>;
  int ax = 0;
  if constexpr (DIMS == 3) {
    if (z + 1 < a.nz) {
      T n[4];
      load4(c + G::RowsY * kRow, n);
#pragma unroll
      for (int j = 0; j < 4; ++j) g[0][j] = n[j] - out[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) g[0][j] = (T)0;
    }
    ax = 1;
  }
  if (y + 1 < a.ny) {
    T n[4];
    load4(c + kRow, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) g[ax][j] = n[j] - out[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) g[ax][j] = (T)0;
  }
  const T right = x + 4 < a.nx ? c[4] : (T)0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const T nb = j < 3 ? out[j < 3 ? j + 1 : 3] : right;
    g[ax + 1][j] = x + j + 1 < a.nx ? nb - out[j] : (T)0;
  }
}

// One joint iteration.  partial[2 * tile] = sum over the channels (ascending) and the tile of d^2, partial[2 * tile + 1]
// = sum over the tile of the shared norm: the layout tv_reduce_kernel folds, with n_problem = n_chan * voxels.
template <typename T, int DIMS, bool FIRST>
__global__ __launch_bounds__(kBlock) void tvj_pass_kernel(const TvArgs a, const int n_chan, const int64_t chan_stride,
                                                          const T* __restrict__ p_old, T* __restrict__ p_new,
                                                          const TvState* __restrict__ state, double* __restrict__ partial,
                                                          T tau, T tau_over_weight) {
  using G = Tile<DIMS>;
  __shared__ __attribute__((aligned(16))) T lds_out[G::RowsZ * G::RowsY * kRow];
  __shared__ double lds_sum[2 * kWaves];
  const int tid = threadIdx.x;
  const int problem = blockIdx.x / a.tiles_per_problem;
  if (!FIRST && state[problem].done) return;
  int t = blockIdx.x - problem * a.tiles_per_problem;
  const int bx = t % a.tiles_x;
  t /= a.tiles_x;
  const int by = t % a.tiles_y, bz = t / a.tiles_y;
  const int x0 = bx * kTX, y0 = by * G::TY, z0 = bz * G::TZ;
  const int64_t base = (int64_t)problem * a.n_problem;
  const bool vec = a.vec != 0;

  T own[kQuadsPerThread][DIMS][4], out[kQuadsPerThread][4], s[kQuadsPerThread][4];
#pragma unroll
  for (int k = 0; k < kQuadsPerThread; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) s[k][j] = (T)0;
  double sum_d = 0.0, sum_n = 0.0;

  // steps 0 .. C - 1 are sweep 1 (c ascending: S = sq_0, S = S + sq_c), steps C - 1 .. 2 C - 2 sweep 2 (c descending: the
  // update); step C - 1 belongs to both, and turns S into the shared denominator in between
  for (int step = 0; step < 2 * n_chan - 1; ++step) {
    const bool first_sweep = step < n_chan;
    const int c = first_sweep ? step : 2 * n_chan - 2 - step;
    const int64_t cb = base + c * chan_stride;
    if (step > 0) __syncthreads();  // every thread is done with the tile of the step before
    tvj_stage<T, DIMS, FIRST>(a, a.f + cb, FIRST ? nullptr : p_old + cb, tid, x0, y0, z0, lds_out, own, out, first_sweep, sum_d);
    __syncthreads();
    T* pn = p_new + cb;
#pragma unroll
    for (int k = 0; k < kQuadsPerThread; ++k) {
      const int item = tid + k * kBlock;
      const int q = item % kQX, ly = (item / kQX) % G::TY, lz = item / (kQX * G::TY);
      const int x = x0 + 4 * q, y = y0 + ly, z = z0 + lz;
      if (x < a.nx && y < a.ny && z < a.nz) {
        const int64_t off = ((int64_t)z * a.ny + y) * a.nx + x;
        T g[DIMS][4];
        tvj_grad<T, DIMS>(a, lds_out + (lz * G::RowsY + ly) * kRow + 4 * q, out[k], z, y, x, g);
        if (first_sweep) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            T sq = g[0][j] * g[0][j] + g[1][j] * g[1][j];
            if constexpr (DIMS == 3) sq = sq + g[2][j] * g[2][j];
            s[k][j] = c == 0 ? sq : s[k][j] + sq;
          }
        }
        if (step == n_chan - 1) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const T nrm = sqrt_rn(s[k][j]);
            if (x + j < a.nx) sum_n += (double)nrm;
            s[k][j] = (T)1 + tau_over_weight * nrm;
          }
        }
        if (step >= n_chan - 1) {
          T upd[DIMS][4];
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int b = 0; b < DIMS; ++b) upd[b][j] = div_rn(own[k][b][j] - tau * g[b][j], s[k][j]);
#pragma unroll
          for (int b = 0; b < DIMS; ++b) store_quad(pn + b * a.n_total, off, x, a.nx, vec, upd[b]);
        }
      }
    }
  }

  sum_d = wave_sum(sum_d);
  sum_n = wave_sum(sum_n);
  if ((tid & 63) == 0) {
    lds_sum[2 * (tid >> 6)] = sum_d;
    lds_sum[2 * (tid >> 6) + 1] = sum_n;
  }
  __syncthreads();
  if (tid == 0) {
    double sd = lds_sum[0], sn = lds_sum[1];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) sd += lds_sum[2 * w], sn += lds_sum[2 * w + 1];
    partial[2 * (int64_t)blockIdx.x] = sd;
    partial[2 * (int64_t)blockIdx.x + 1] = sn;
  }
}

// The result of every channel, as tv_finish_kernel writes one: out_c = f_c + d_c from the half that iteration n_iter read.
template <typename T, int DIMS>
__global__ __launch_bounds__(kBlock) void tvj_finish_kernel(const TvArgs a, const int n_chan, const int64_t chan_stride,
                                                            const T* __restrict__ p_even, const T* __restrict__ p_odd,
                                                            const TvState* __restrict__ state, float* dst,
                                                            int32_t* __restrict__ n_iter_out, double* __restrict__ energy_out) {
  using G = Tile<DIMS>;
  const int tid = threadIdx.x;
  const int problem = blockIdx.x / a.tiles_per_problem;
  int t = blockIdx.x - problem * a.tiles_per_problem;
  const int n_iter = state[problem].n_iter;
  if (t == 0 && tid == 0) {
    if (n_iter_out) n_iter_out[problem] = n_iter;
    if (energy_out) energy_out[problem] = state[problem].e_last;
  }
  const int bx = t % a.tiles_x;
  t /= a.tiles_x;
  const int by = t % a.tiles_y, bz = t / a.tiles_y;
  const bool dst_vec = a.vec && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
#pragma unroll
  for (int k = 0; k < kQuadsPerThread; ++k) {
    const int item = tid + k * kBlock;
    const int q = item % kQX, ly = (item / kQX) % G::TY, lz = item / (kQX * G::TY);
    const int x = bx * kTX + 4 * q, y = by * G::TY + ly, z = bz * G::TZ + lz;
    if (x < a.nx && y < a.ny && z < a.nz) {
      const int64_t off = ((int64_t)z * a.ny + y) * a.nx + x;
      for (int c = 0; c < n_chan; ++c) {
        const int64_t cb = (int64_t)problem * a.n_problem + c * chan_stride;
        const T* p = ((n_iter & 1) ? p_odd : p_even) + cb;
        T own[DIMS][4], d[4], out[4];
        if (n_iter == 0) out_quad<T, DIMS, true>(a, a.f + cb, p, off, z, y, x, own, d, out);
        else out_quad<T, DIMS, false>(a, a.f + cb, p, off, z, y, x, own, d, out);
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = (float)out[j];
        store_quad(dst + cb, off, x, a.nx, dst_vec, r);
      }
    }
  }
}

// the scalar plan of the stack (n_chan, nz, ny, nx), then: a problem spans all channels
int tvj_plan(const char* who, const t2fit_tv_params* p, int n_chan, int nz, int ny, int nx, TvPlan* plan) {
  if (n_chan < 1) return t2fit::fail(T2FIT_E_INVALID, std::string(who) + ": n_chan, nz, ny, nx must all be >= 1");
  if (n_chan > T2FIT_TV_JOINT_MAX_CHAN)
    return t2fit::fail(T2FIT_E_INVALID, std::string(who) + ": n_chan is above T2FIT_TV_JOINT_MAX_CHAN (" +
                                            std::to_string(T2FIT_TV_JOINT_MAX_CHAN) + ")");
  const int rc = tv_plan(who, p, n_chan, nz, ny, nx, plan);
  if (rc != T2FIT_OK) return rc;
  plan->n_problems /= n_chan;  // nz slices (dims = 2) or the one stack (dims = 3); n_problem stays the voxels of a channel
  plan->n_tiles = plan->tiles_per_problem * plan->n_problems;
  plan->partial_bytes = align_up((size_t)plan->n_tiles * 16, kAlign);
  plan->state_bytes = align_up((size_t)plan->n_problems * sizeof(TvState), kAlign);
  plan->total = 2 * plan->field_bytes + plan->partial_bytes + plan->state_bytes;
  return T2FIT_OK;
}

template <typename T, int DIMS>
int tvj_run(const t2fit_tv_params* p, const TvPlan& plan, const TvArgs& a, int n_chan, int64_t chan_stride, float* out_dev,
            char* ws, int32_t* n_iter_dev, double* energy_dev, hipStream_t st) {
  T* half[2] = {reinterpret_cast<T*>(ws), reinterpret_cast<T*>(ws + plan.field_bytes)};
  double* partial = reinterpret_cast<double*>(ws + 2 * plan.field_bytes);
  TvState* state = reinterpret_cast<TvState*>(ws + 2 * plan.field_bytes + plan.partial_bytes);
  const double tau = 1.0 / (2.0 * DIMS);
  const T tau_t = (T)tau, tw_t = (T)(tau / p->weight);
  const dim3 grid((unsigned)plan.n_tiles), block(kBlock);
  const double n_joint = (double)n_chan * (double)plan.n_problem;  // N of the energy
  for (int i = 0; i < p->max_iter; ++i) {
    if (i == 0)
      hipLaunchKernelGGL((tvj_pass_kernel<T, DIMS, true>), grid, block, 0, st, a, n_chan, chan_stride, (const T*)half[0], half[1],
                         (const TvState*)state, partial, tau_t, tw_t);
    else
      hipLaunchKernelGGL((tvj_pass_kernel<T, DIMS, false>), grid, block, 0, st, a, n_chan, chan_stride, (const T*)half[i & 1],
                         half[(i + 1) & 1], (const TvState*)state, partial, tau_t, tw_t);
    hipLaunchKernelGGL(tv_reduce_kernel, dim3((unsigned)plan.n_problems), dim3(64), 0, st, (const double*)partial, state,
                       (int)plan.tiles_per_problem, n_joint, p->weight, p->eps, i, p->max_iter);
  }
  hipLaunchKernelGGL((tvj_finish_kernel<T, DIMS>), grid, block, 0, st, a, n_chan, chan_stride, (const T*)half[0],
                     (const T*)half[1], (const TvState*)state, out_dev, n_iter_dev, energy_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

}  // namespace

extern "C" {

int t2fit_tv_params_default(t2fit_tv_params* p) {
  if (!p) return t2fit::fail(T2FIT_E_INVALID, "t2fit_tv_params_default: params is NULL");
  p->weight = 0.1;
  p->eps = 2e-4;
  p->max_iter = 200;
  p->dims = 2;
  p->precision = T2FIT_PREC_F32;
  p->flags = 0;
  return T2FIT_OK;
}

int t2fit_tv_workspace_bytes(const t2fit_tv_params* p, int n_vol, int nz, int ny, int nx, size_t* bytes) {
  if (!bytes) return t2fit::fail(T2FIT_E_INVALID, "t2fit_tv_workspace_bytes: bytes is NULL");
  TvPlan plan;
  const int rc = tv_plan("t2fit_tv_workspace_bytes", p, n_vol, nz, ny, nx, &plan);
  if (rc != T2FIT_OK) return rc;
  *bytes = plan.total;
  return T2FIT_OK;
}

int t2fit_tv_denoise_dev(const t2fit_tv_params* p, const float* in_dev, float* out_dev, int n_vol, int nz, int ny, int nx,
                         void* workspace_dev, size_t workspace_bytes, int32_t* n_iter_dev, double* energy_dev, void* stream) {
  if (!in_dev || !out_dev || !workspace_dev)
    return t2fit::fail(T2FIT_E_INVALID, "t2fit_tv_denoise_dev: in_dev / out_dev / workspace_dev is NULL");
  TvPlan plan;
  const int rc = tv_plan("t2fit_tv_denoise_dev", p, n_vol, nz, ny, nx, &plan);
  if (rc != T2FIT_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(in_dev) & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 3))
    return t2fit::fail(T2FIT_E_INVALID, "t2fit_tv_denoise_dev: in_dev / out_dev is not aligned to 4 bytes");
  if (reinterpret_cast<uintptr_t>(workspace_dev) & (kAlign - 1))
    return t2fit::fail(T2FIT_E_INVALID, "t2fit_tv_denoise_dev: workspace_dev is not aligned to 256 bytes");
  if (workspace_bytes < plan.total)
    return t2fit::fail(T2FIT_E_INVALID, "t2fit_tv_denoise_dev: workspace too small: " + std::to_string(workspace_bytes) +
                                            " bytes given, " + std::to_string(plan.total) +
                                            " needed (t2fit_tv_workspace_bytes)");
  TvArgs a;
  a.f = in_dev;
  a.nz = plan.pnz, a.ny = ny, a.nx = nx;
  a.tiles_x = plan.tiles_x, a.tiles_y = plan.tiles_y, a.tiles_per_problem = (int)plan.tiles_per_problem;
  a.vec = (nx % 4 == 0) && (reinterpret_cast<uintptr_t>(in_dev) & 15) == 0;
  a.n_problem = plan.n_problem;
  a.n_total = plan.n_total;
  char* ws = static_cast<char*>(workspace_dev);
  hipStream_t st = (hipStream_t)stream;
  const bool f32 = p->precision == T2FIT_PREC_F32;
  if (p->dims == 2)
    return f32 ? tv_run<float, 2>(p, plan, a, out_dev, ws, n_iter_dev, energy_dev, st)
               : tv_run<double, 2>(p, plan, a, out_dev, ws, n_iter_dev, energy_dev, st);
  return f32 ? tv_run<float, 3>(p, plan, a, out_dev, ws, n_iter_dev, energy_dev, st)
             : tv_run<double, 3>(p, plan, a, out_dev, ws, n_iter_dev, energy_dev, st);
}

int t2fit_tv_joint_workspace_bytes(const t2fit_tv_params* p, int n_chan, int nz, int ny, int nx, size_t* bytes) {
  if (!bytes) return t2fit::fail(T2FIT_E_INVALID, "t2fit_tv_joint_workspace_bytes: bytes is NULL");
  TvPlan plan;
  const int rc = tvj_plan("t2fit_tv_joint_workspace_bytes", p, n_chan, nz, ny, nx, &plan);
  if (rc != T2FIT_OK) return rc;
  *bytes = plan.total;
  return T2FIT_OK;
}

int t2fit_tv_joint_denoise_dev(const t2fit_tv_params* p, const float* in_dev, float* out_dev, int n_chan, int nz, int ny, int nx,
                               void* workspace_dev, size_t workspace_bytes, int32_t* n_iter_dev, double* energy_dev,
                               void* stream) {
  if (!in_dev || !out_dev || !workspace_dev)
    return t2fit::fail(T2FIT_E_INVALID, "t2fit_tv_joint_denoise_dev: in_dev / out_dev / workspace_dev is NULL");
  TvPlan plan;
  const int rc = tvj_plan("t2fit_tv_joint_denoise_dev", p, n_chan, nz, ny, nx, &plan);
  if (rc != T2FIT_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(in_dev) & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 3))
    return t2fit::fail(T2FIT_E_INVALID, "t2fit_tv_joint_denoise_dev: in_dev / out_dev is not aligned to 4 bytes");
  if (reinterpret_cast<uintptr_t>(workspace_dev) & (kAlign - 1))
    return t2fit::fail(T2FIT_E_INVALID, "t2fit_tv_joint_denoise_dev: workspace_dev is not aligned to 256 bytes");
  if (workspace_bytes < plan.total)
    return t2fit::fail(T2FIT_E_INVALID, "t2fit_tv_joint_denoise_dev: workspace too small: " + std::to_string(workspace_bytes) +
                                            " bytes given, " + std::to_string(plan.total) +
                                            " needed (t2fit_tv_joint_workspace_bytes)");
  TvArgs a;
  a.f = in_dev;
  a.nz = plan.pnz, a.ny = ny, a.nx = nx;
  a.tiles_x = plan.tiles_x, a.tiles_y = plan.tiles_y, a.tiles_per_problem = (int)plan.tiles_per_problem;
  a.vec = (nx % 4 == 0) && (reinterpret_cast<uintptr_t>(in_dev) & 15) == 0;
  a.n_problem = plan.n_problem;
  a.n_total = plan.n_total;
  const int64_t chan_stride = (int64_t)nz * ny * nx;
  char* ws = static_cast<char*>(workspace_dev);
  hipStream_t st = (hipStream_t)stream;
  const bool f32 = p->precision == T2FIT_PREC_F32;
  if (p->dims == 2)
    return f32 ? tvj_run<float, 2>(p, plan, a, n_chan, chan_stride, out_dev, ws, n_iter_dev, energy_dev, st)
               : tvj_run<double, 2>(p, plan, a, n_chan, chan_stride, out_dev, ws, n_iter_dev, energy_dev, st);
  return f32 ? tvj_run<float, 3>(p, plan, a, n_chan, chan_stride, out_dev, ws, n_iter_dev, energy_dev, st)
             : tvj_run<double, 3>(p, plan, a, n_chan, chan_stride, out_dev, ws, n_iter_dev, energy_dev, st);
}

}  // extern "C"

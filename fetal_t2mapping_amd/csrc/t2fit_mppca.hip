// t2fit_mppca.hip -- Marchenko-Pastur PCA denoising and noise maps across the echoes (include/t2fit.h:
// t2fit_mppca_dev; fetal_t2mapping_amd/_mppca.py states every step in numpy and the kernels equal it bit for bit).
//
// Two kernels.  mppca_eigen_kernel: one lane per centre, one wave per workgroup.  The lane forms the Gram matrix of its
// window row by row (three partial accumulators per entry: x, then y, then z), runs cyclic Jacobi on it with A (upper
// triangle) and V in registers, ranks the eigenvalues by counting, walks dwidenoise's estimator, and writes the projector
// onto the kept components (pair-major, so a wave's stores are contiguous), sigma and the rank.  The kernel is a template
// on the echo count for 2..8 so that every index is a constant and nothing lands in scratch memory; 9..16 echoes run the
// same text with run-time loops and the two matrices in scratch.  The sweep loop is per lane; a wave leaves when all its
// lanes have off == 0.  mppca_aggregate_kernel: one lane per voxel; the ordered window sum of the projector field, the
// count of processed centres, then the product with the voxel's own decay.  No atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "t2fit_error.h"
#include "t2fit_support.h"

namespace {

using t2fit::align_up;
using t2fit::ceil_div;

constexpr size_t kAlign = 256;
constexpr int kMaxTe = T2FIT_MPPCA_MAX_TE;
constexpr int kEigenBlock = 64;  // one wave: it retires as soon as its own lanes have converged
constexpr int kMaxSweeps = 16;

struct MpArgs {
  const float* x;       // (m, nz, ny, nx)
  const uint8_t* mask;  // (nz, ny, nx) or NULL
  double* proj;         // (pairs, centres) or NULL (estimate only)
  uint8_t* done;        // (centres) or NULL (estimate only)
  float* out;           // (m, nz, ny, nx)
  float* sigma;         // (nz, ny, nx) or NULL
  uint8_t* rank;        // (nz, ny, nx) or NULL
  int m, nz, ny, nx, r, rz, estimator, n_window;
  int cz, cy, cx;  // centres per axis
  int64_t n_cent, vol;
};

struct MpPlan {
  int cz, cy, cx, rz, n_window, pairs;
  int64_t n_cent, vol;
  size_t proj_bytes, total;
};

int mp_plan(const char* who, const t2fit_mppca_params* p, int n_te, int nz, int ny, int nx, MpPlan* plan) {
  const std::string w(who);
  if (!p) return t2fit::fail(T2FIT_E_INVALID, w + ": params is NULL");
  if (p->dims != 2 && p->dims != 3) return t2fit::fail(T2FIT_E_INVALID, w + ": dims must be 2 or 3");
  if (p->radius < 1 || p->radius > T2FIT_MPPCA_MAX_RADIUS)
    return t2fit::fail(T2FIT_E_INVALID, w + ": radius must be 1.." + std::to_string(T2FIT_MPPCA_MAX_RADIUS));
  if (p->estimator != 1 && p->estimator != 2) return t2fit::fail(T2FIT_E_INVALID, w + ": estimator must be 1 or 2");
  if (p->flags != 0) return t2fit::fail(T2FIT_E_INVALID, w + ": flags must be 0");
  if (n_te < 2 || n_te > kMaxTe)
    return t2fit::fail(T2FIT_E_INVALID, w + ": n_te must be 2.." + std::to_string(kMaxTe) + " (T2FIT_MPPCA_MAX_TE)");
  if (nz < 1 || ny < 1 || nx < 1) return t2fit::fail(T2FIT_E_INVALID, w + ": nz, ny, nx must be >= 1");
  const int width = 2 * p->radius + 1;
  int n_window = width * width;
  if (p->dims == 3) n_window *= width;
  if (n_window <= n_te)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the window of " + std::to_string(n_window) +
                                            " voxels must hold more voxels than there are echoes (" + std::to_string(n_te) + ")");
  if (ny < width || nx < width || (p->dims == 3 && nz < width))
    return t2fit::fail(T2FIT_E_INVALID, w + ": every windowed axis must be at least 2 radius + 1 = " + std::to_string(width) + " long");
  plan->rz = p->dims == 3 ? p->radius : 0;
  plan->cz = nz - 2 * plan->rz, plan->cy = ny - 2 * p->radius, plan->cx = nx - 2 * p->radius;
  plan->n_window = n_window;
  plan->pairs = n_te * (n_te + 1) / 2;
  plan->n_cent = (int64_t)plan->cz * plan->cy * plan->cx;
  plan->vol = (int64_t)nz * ny * nx;
  if (ceil_div<int64_t>(plan->vol, kEigenBlock) > 0x7fffffffLL)
    return t2fit::fail(T2FIT_E_INVALID, w + ": the volume has too many voxels for one launch");
  plan->proj_bytes = align_up((size_t)plan->pairs * (size_t)plan->n_cent * sizeof(double), kAlign);
  plan->total = plan->proj_bytes + align_up((size_t)plan->n_cent, kAlign);
  return T2FIT_OK;
}

// sigma / rank of a centre go to every voxel whose clamped position is that centre: its own voxel, and at the rim of
// the centre region the voxels outside it
__device__ inline void mp_write_maps(const MpArgs& a, int ix, int iy, int iz, float sigma, uint8_t rank) {
  const int x0 = ix == 0 ? 0 : ix + a.r, x1 = ix == a.cx - 1 ? a.nx - 1 : ix + a.r;
  const int y0 = iy == 0 ? 0 : iy + a.r, y1 = iy == a.cy - 1 ? a.ny - 1 : iy + a.r;
  const int z0 = (a.rz && iz == 0) ? 0 : iz + a.rz, z1 = (a.rz && iz == a.cz - 1) ? a.nz - 1 : iz + a.rz;
  for (int z = z0; z <= z1; ++z)
    for (int y = y0; y <= y1; ++y)
      for (int x = x0; x <= x1; ++x) {
        const int64_t v = ((int64_t)z * a.ny + y) * a.nx + x;
        if (a.sigma) a.sigma[v] = sigma;
        if (a.rank) a.rank[v] = rank;
      }
}

// full unrolling where the echo count is a constant (UN = MT), none on the generic path (UN = 1)
#define MP_UNROLL _Pragma("unroll UN")

// MT: the echo count as a constant (2..8), or 0: a.m at run time (9..16)
template <int MT>
__global__ __launch_bounds__(kEigenBlock) void mppca_eigen_kernel(MpArgs a) {
  constexpr int LD = MT ? MT : kMaxTe;
  constexpr int UN = MT ? MT : 1;
  const int M = MT ? MT : a.m;
  const int64_t c = (int64_t)blockIdx.x * kEigenBlock + threadIdx.x;
  if (c >= a.n_cent) return;
  const int ix = (int)(c % a.cx), iy = (int)((c / a.cx) % a.cy), iz = (int)(c / ((int64_t)a.cx * a.cy));
  const int vx = ix + a.r, vy = iy + a.r, vz = iz + a.rz;
  const int pairs = M * (M + 1) / 2;

  double A[LD * LD];  // the upper triangle is used: A[i * LD + j], i <= j
  bool go = !a.mask || a.mask[((int64_t)vz * a.ny + vy) * a.nx + vx] != 0;
  if (go) {
    const int width = 2 * a.r + 1;
    MP_UNROLL
    for (int i = 0; i < M; ++i) {
      double sz[LD], sy[LD], sx[LD];
      MP_UNROLL
      for (int j = i; j < M; ++j) sz[j] = 0.0;
      for (int dz = -a.rz; dz <= a.rz; ++dz) {
        MP_UNROLL
        for (int j = i; j < M; ++j) sy[j] = 0.0;
        for (int dy = -a.r; dy <= a.r; ++dy) {
          const float* row = a.x + ((int64_t)(vz + dz) * a.ny + (vy + dy)) * a.nx + (vx - a.r);
          MP_UNROLL
          for (int j = i; j < M; ++j) sx[j] = 0.0;
          for (int dx = 0; dx < width; ++dx) {
            const double xi = (double)row[i * a.vol + dx];
            MP_UNROLL
            for (int j = i; j < M; ++j) sx[j] = sx[j] + xi * (double)row[j * a.vol + dx];
          }
          MP_UNROLL
          for (int j = i; j < M; ++j) sy[j] = sy[j] + sx[j];
        }
        MP_UNROLL
        for (int j = i; j < M; ++j) sz[j] = sz[j] + sy[j];
      }
      MP_UNROLL
      for (int j = i; j < M; ++j) {
        A[i * LD + j] = sz[j];
        go = go && isfinite(sz[j]);
      }
    }
  }
  if (!go) {  // unprocessed: a zero projector, sigma 0, rank 0
    if (a.proj) {
      for (int k = 0; k < pairs; ++k) a.proj[(size_t)k * a.n_cent + c] = 0.0;
      a.done[c] = 0;
    }
    mp_write_maps(a, ix, iy, iz, 0.0f, 0);
    return;
  }

  double V[LD * LD];
  MP_UNROLL
  for (int i = 0; i < M; ++i) {
    MP_UNROLL
    for (int j = 0; j < M; ++j) V[i * LD + j] = i == j ? 1.0 : 0.0;
  }
#pragma unroll 1
  for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
    double off = 0.0;
    MP_UNROLL
    for (int p = 0; p < M - 1; ++p) {
      MP_UNROLL
      for (int q = p + 1; q < M; ++q) off = off + A[p * LD + q] * A[p * LD + q];
    }
    if (off == 0.0) break;
    MP_UNROLL
    for (int p = 0; p < M - 1; ++p) {
      MP_UNROLL
      for (int q = p + 1; q < M; ++q) {
        const double app = A[p * LD + p], aqq = A[q * LD + q];
        double apq = A[p * LD + q];
        const double g = fabs(apq);
        if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) apq = 0.0;
        A[p * LD + q] = apq;
        if (apq != 0.0) {
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double cs = 1.0 / sqrt(t * t + 1.0);
          const double sn = t * cs;
          MP_UNROLL
          for (int k = 0; k < M; ++k) {
            if (k != p && k != q) {
              const int kp = k < p ? k * LD + p : p * LD + k, kq = k < q ? k * LD + q : q * LD + k;
              const double akp = A[kp], akq = A[kq];
              A[kp] = cs * akp - sn * akq;
              A[kq] = sn * akp + cs * akq;
            }
          }
          A[p * LD + p] = app - t * apq;
          A[q * LD + q] = aqq + t * apq;
          A[p * LD + q] = 0.0;
          MP_UNROLL
          for (int k = 0; k < M; ++k) {
            const double vkp = V[k * LD + p], vkq = V[k * LD + q];
            V[k * LD + p] = cs * vkp - sn * vkq;
            V[k * LD + q] = sn * vkp + cs * vkq;
          }
        }
      }
    }
  }

  // ascending order, ties by index: a rank by counting
  int pos[LD];
  MP_UNROLL
  for (int i = 0; i < M; ++i) {
    int n = 0;
    MP_UNROLL
    for (int j = 0; j < M; ++j) {
      if (j != i) {
        const double wi = A[i * LD + i], wj = A[j * LD + j];
        n += (wj < wi || (wj == wi && j < i)) ? 1 : 0;
      }
    }
    pos[i] = n;
  }

  // dwidenoise's estimator on the ascending eigenvalues
  const double q = (double)a.n_window;
  double lam_r = 0.0, clam = 0.0, sigsq = 0.0;
  int cut = 0;
  MP_UNROLL
  for (int p = 0; p < M; ++p) {
    double sp = 0.0;
    MP_UNROLL
    for (int i = 0; i < M; ++i) sp = pos[i] == p ? A[i * LD + i] : sp;
    const double lam = (sp > 0.0 ? sp : 0.0) / q;  // max(s_p, 0) / q
    if (p == 0) lam_r = lam;
    clam = clam + lam;
    const double gam = (double)(p + 1) / (a.estimator == 2 ? (double)(a.n_window - (M - p - 1)) : q);
    const double ea = clam / (double)(p + 1);
    const double eb = (lam - lam_r) / (4.0 * sqrt(gam));
    if (eb < ea) {
      sigsq = ea;
      cut = p + 1;
    }
  }
  mp_write_maps(a, ix, iy, iz, (float)sqrt(sigsq), (uint8_t)(M - cut));
  if (!a.proj) return;

  // the projector onto the components at the positions cut .. M - 1, added in ascending position from 0.0; A is free
  MP_UNROLL
  for (int i = 0; i < M; ++i) {
    MP_UNROLL
    for (int j = i; j < M; ++j) A[i * LD + j] = 0.0;
  }
  MP_UNROLL
  for (int k = 0; k < M; ++k) {
    if (k >= cut) {
      double vec[LD];
      MP_UNROLL
      for (int i = 0; i < M; ++i) {
        vec[i] = 0.0;
        MP_UNROLL
        for (int col = 0; col < M; ++col) vec[i] = pos[col] == k ? V[i * LD + col] : vec[i];
      }
      MP_UNROLL
      for (int i = 0; i < M; ++i) {
        MP_UNROLL
        for (int j = i; j < M; ++j) A[i * LD + j] = A[i * LD + j] + vec[i] * vec[j];
      }
    }
  }
  int pair = 0;
  MP_UNROLL
  for (int i = 0; i < M; ++i) {
    MP_UNROLL
    for (int j = i; j < M; ++j) {
      a.proj[(size_t)pair * a.n_cent + c] = A[i * LD + j];
      ++pair;
    }
  }
  a.done[c] = 1;
}

template <int MT>
__global__ __launch_bounds__(t2fit::kBlock) void mppca_aggregate_kernel(MpArgs a) {
  constexpr int LD = MT ? MT : kMaxTe;
  constexpr int UN = MT ? MT : 1;
  const int M = MT ? MT : a.m;
  const int64_t v = (int64_t)blockIdx.x * t2fit::kBlock + threadIdx.x;
  if (v >= a.vol) return;
  const int x = (int)(v % a.nx), y = (int)((v / a.nx) % a.ny), z = (int)(v / ((int64_t)a.nx * a.ny));
  // centre indices of the window around the voxel, clipped to the centres that exist; the skipped ones are zeros of the
  // ordered sum, which never change it (no partial sum is -0.0: each starts from +0.0)
  const int x_lo = max(x - a.r, a.r) - a.r, x_hi = min(x + a.r, a.nx - 1 - a.r) - a.r;
  const int y_lo = max(y - a.r, a.r) - a.r, y_hi = min(y + a.r, a.ny - 1 - a.r) - a.r;
  const int z_lo = max(z - a.rz, a.rz) - a.rz, z_hi = min(z + a.rz, a.nz - 1 - a.rz) - a.rz;
  int cnt = 0;
  for (int cz = z_lo; cz <= z_hi; ++cz)
    for (int cy = y_lo; cy <= y_hi; ++cy) {
      const uint8_t* row = a.done + ((int64_t)cz * a.cy + cy) * a.cx;
      for (int cx = x_lo; cx <= x_hi; ++cx) cnt += row[cx];
    }
  float xs[LD];
  MP_UNROLL
  for (int j = 0; j < M; ++j) xs[j] = a.x[j * a.vol + v];
  if (cnt == 0) {
    MP_UNROLL
    for (int j = 0; j < M; ++j) a.out[j * a.vol + v] = xs[j];
    return;
  }
  double pb[LD * LD];
  int pair = 0;
  MP_UNROLL
  for (int i = 0; i < M; ++i) {
    MP_UNROLL
    for (int j = i; j < M; ++j) {
      const double* field = a.proj + (size_t)pair * a.n_cent;
      double sz = 0.0;
      for (int cz = z_lo; cz <= z_hi; ++cz) {
        double sy = 0.0;
        for (int cy = y_lo; cy <= y_hi; ++cy) {
          const double* row = field + ((int64_t)cz * a.cy + cy) * a.cx;
          double sx = 0.0;
          for (int cx = x_lo; cx <= x_hi; ++cx) sx = sx + row[cx];
          sy = sy + sx;
        }
        sz = sz + sy;
      }
      pb[i * LD + j] = sz;
      ++pair;
    }
  }
  const double n = (double)cnt;
  MP_UNROLL
  for (int i = 0; i < M; ++i) {
    double acc = 0.0;
    MP_UNROLL
    for (int j = 0; j < M; ++j) acc = acc + pb[i < j ? i * LD + j : j * LD + i] * (double)xs[j];
    a.out[i * a.vol + v] = (float)(acc / n);
  }
}

template <int MT>
int mp_launch(const MpArgs& a, bool aggregate, hipStream_t st) {
  mppca_eigen_kernel<MT><<<dim3((unsigned)ceil_div<int64_t>(a.n_cent, kEigenBlock)), dim3(kEigenBlock), 0, st>>>(a);
  T2_HIP(hipGetLastError());
  if (aggregate) {
    mppca_aggregate_kernel<MT><<<dim3((unsigned)ceil_div<int64_t>(a.vol, t2fit::kBlock)), dim3(t2fit::kBlock), 0, st>>>(a);
    T2_HIP(hipGetLastError());
  }
  return T2FIT_OK;
}

}  // namespace

extern "C" {

int t2fit_mppca_params_default(t2fit_mppca_params* p) {
  if (!p) return t2fit::fail(T2FIT_E_INVALID, "t2fit_mppca_params_default: params is NULL");
  p->radius = 2;
  p->dims = 2;
  p->estimator = 2;
  p->flags = 0;
  return T2FIT_OK;
}

int t2fit_mppca_workspace_bytes(const t2fit_mppca_params* p, int n_te, int nz, int ny, int nx, size_t* bytes) {
  if (!bytes) return t2fit::fail(T2FIT_E_INVALID, "t2fit_mppca_workspace_bytes: bytes is NULL");
  MpPlan plan;
  const int rc = mp_plan("t2fit_mppca_workspace_bytes", p, n_te, nz, ny, nx, &plan);
  if (rc != T2FIT_OK) return rc;
  *bytes = plan.total;
  return T2FIT_OK;
}

int t2fit_mppca_dev(const t2fit_mppca_params* p, const float* in_dev, const uint8_t* mask_dev, float* out_dev, float* sigma_dev,
                    uint8_t* rank_dev, int n_te, int nz, int ny, int nx, void* workspace_dev, size_t workspace_bytes, void* stream) {
  const char* who = "t2fit_mppca_dev";
  if (!in_dev) return t2fit::fail(T2FIT_E_INVALID, std::string(who) + ": in_dev is NULL");
  if (!out_dev && !sigma_dev && !rank_dev)
    return t2fit::fail(T2FIT_E_INVALID, std::string(who) + ": out_dev, sigma_dev and rank_dev are all NULL: nothing to compute");
  MpPlan plan;
  const int rc = mp_plan(who, p, n_te, nz, ny, nx, &plan);
  if (rc != T2FIT_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(in_dev) & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 3) ||
      (reinterpret_cast<uintptr_t>(sigma_dev) & 3))
    return t2fit::fail(T2FIT_E_INVALID, std::string(who) + ": in_dev / out_dev / sigma_dev is not aligned to 4 bytes");
  if (out_dev) {
    if (!workspace_dev) return t2fit::fail(T2FIT_E_INVALID, std::string(who) + ": workspace_dev is NULL (only out_dev = NULL needs none)");
    if (reinterpret_cast<uintptr_t>(workspace_dev) & (kAlign - 1))
      return t2fit::fail(T2FIT_E_INVALID, std::string(who) + ": workspace_dev is not aligned to 256 bytes");
    if (workspace_bytes < plan.total)
      return t2fit::fail(T2FIT_E_INVALID, std::string(who) + ": workspace too small: " + std::to_string(workspace_bytes) +
                                              " bytes given, " + std::to_string(plan.total) + " needed (t2fit_mppca_workspace_bytes)");
  }
  MpArgs a;
  a.x = in_dev, a.mask = mask_dev, a.out = out_dev, a.sigma = sigma_dev, a.rank = rank_dev;
  a.proj = out_dev ? static_cast<double*>(workspace_dev) : nullptr;
  a.done = out_dev ? static_cast<uint8_t*>(workspace_dev) + plan.proj_bytes : nullptr;
  a.m = n_te, a.nz = nz, a.ny = ny, a.nx = nx, a.r = p->radius, a.rz = plan.rz, a.estimator = p->estimator;
  a.n_window = plan.n_window;
  a.cz = plan.cz, a.cy = plan.cy, a.cx = plan.cx;
  a.n_cent = plan.n_cent, a.vol = plan.vol;
  hipStream_t st = (hipStream_t)stream;
  const bool agg = out_dev != nullptr;
  switch (n_te) {
    case 2: return mp_launch<2>(a, agg, st);
    case 3: return mp_launch<3>(a, agg, st);
    case 4: return mp_launch<4>(a, agg, st);
    case 5: return mp_launch<5>(a, agg, st);
    case 6: return mp_launch<6>(a, agg, st);
    case 7: return mp_launch<7>(a, agg, st);
    case 8: return mp_launch<8>(a, agg, st);
    default: return mp_launch<0>(a, agg, st);
  }
}

}  // extern "C"

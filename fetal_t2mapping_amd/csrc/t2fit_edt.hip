// t2fit_edt.hip -- gfx950 kernels and C ABI of the exact Euclidean distance transform (include/t2fit.h:
// t2fit_edt_workspace_bytes, t2fit_edt_dev, t2fit_edt_fill_dev).  fetal_t2mapping_amd/_edt.py states every result in
// numpy: three exact 1-D minimisations in the order z, y, x over (g float64, key int32), a candidate being compared by
// (value, key) -- the smaller value, on equal values the lower key, a key of -1 never.  That order is total, so the
// minimum does not depend on the order in which candidates are met, and the device equals the statement in every bit.
// No atomics, no scratch, no wave waits for another; every loop is bounded by an axis length.
//   z pass   a lane owns a column (y, x), lanes along x.  An upward sweep carries the nearest site below and writes its
//            (s dz)^2 and key; a downward sweep carries the nearest site above and replaces what is strictly larger (on a
//            tie the site below stays: in a column the lower z is the lower key).
//   y pass   a lane owns a voxel, lanes along x, and scans its column of the plane outward: both neighbours at distance
//            k while (s k)^2 <= best.  fl(g + t) >= t for g >= 0, and (s k)^2 does not fall with k, so nothing beyond
//            the stop can win or tie.  The rows are read through L1 / L2: a step of a wave reads 64 neighbouring g and
//            64 neighbouring keys per side, and the tile of a plane that would serve a wave (ny x 64 x 12 bytes) is too
//            large for LDS at the sizes that matter.
//   x pass   the same scan along the row, which a workgroup first stages in LDS (12 bytes an element, at most 24 KiB:
//            an axis has at most 2048 elements); short rows share a workgroup.
// The scan's body is selects only; a lane that has stopped waits for the longest lane of its wave.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>
#include <string>

#include "t2fit_error.h"
#include "t2fit_support.h"

namespace {

using t2fit::kBlock;

constexpr int kMaxAxis = T2FIT_EDT_MAX_AXIS;
static_assert(kMaxAxis == 2048, "the x pass stages a whole row: 12 bytes x 2048 in LDS");

struct Best {
  double g;
  int key;
};

// (value, key) order: the smaller value, on equal values the lower key; a candidate without a site never wins
__device__ __forceinline__ void consider(Best& b, double cand, int key) {
  const bool take = key >= 0 && (cand < b.g || (cand == b.g && (b.key < 0 || key < b.key)));
  b.g = take ? cand : b.g;
  b.key = take ? key : b.key;
}

// The exact minimum of g[j] + (float64(i - j) s)^2 over the n elements g[j * stride], key[j * stride], scanning outward
// from i.  k runs to n - 1 at the most.
template <class G, class K>
__device__ __forceinline__ Best scan_outward(G g, K key, int stride, int i, int n, double s) {
  Best b{g[(int64_t)i * stride], key[(int64_t)i * stride]};
  const int reach = i > n - 1 - i ? i : n - 1 - i;  // the farther end of the row
  for (int k = 1; k <= reach; ++k) {
    const double t = (double)k * s;
    const double tt = t * t;
    if (!(tt <= b.g)) break;  // strictly beyond the best: an equal value may still tie with a lower key
    const int lo = i - k, hi = i + k;
    const bool has_lo = lo >= 0, has_hi = hi < n;
    const int64_t a_lo = (int64_t)(has_lo ? lo : i) * stride, a_hi = (int64_t)(has_hi ? hi : i) * stride;
    const double g_lo = g[a_lo], g_hi = g[a_hi];
    const int k_lo = key[a_lo], k_hi = key[a_hi];
    consider(b, g_lo + tt, has_lo ? k_lo : -1);
    consider(b, g_hi + tt, has_hi ? k_hi : -1);
  }
  return b;
}

// ---- z pass: from the volume to (g, key) ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void edt_z_kernel(const uint8_t* __restrict__ vol, int invert, int nz, int plane, double s,
                                                       double* __restrict__ g, int32_t* __restrict__ key) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= plane) return;
  const double inf = std::numeric_limits<double>::infinity();
  int last = -1;
  for (int z = 0; z < nz; ++z) {
    const int64_t v = (int64_t)z * plane + c;
    const bool site = (vol[v] != 0) != (invert != 0);
    last = site ? z : last;
    const double t = (double)(z - last) * s;
    g[v] = last >= 0 ? t * t : inf;
    key[v] = last >= 0 ? (int32_t)((int64_t)last * plane + c) : -1;
  }
  last = -1;
  for (int z = nz - 1; z >= 0; --z) {
    const int64_t v = (int64_t)z * plane + c;
    const bool site = (vol[v] != 0) != (invert != 0);
    last = site ? z : last;
    if (last < 0) continue;
    const double t = (double)(last - z) * s;
    const double tt = t * t;
    if (tt < g[v]) {
      g[v] = tt;
      key[v] = (int32_t)((int64_t)last * plane + c);
    }
  }
}

// ---- y pass: a lane per voxel, lanes along x, rows through L1 / L2 -----------------------------------------------------
__global__ __launch_bounds__(kBlock) void edt_y_kernel(const double* __restrict__ g, const int32_t* __restrict__ key, int ny, int nx,
                                                       int n_vox, double s, double* __restrict__ g_out, int32_t* __restrict__ key_out) {
  const int64_t v64 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v64 >= n_vox) return;
  const int v = (int)v64;  // n_vox < 2^31
  const int y = (v / nx) % ny;
  const int64_t base = (int64_t)v - (int64_t)y * nx;  // (z, 0, x)
  const Best b = scan_outward(g + base, key + base, nx, y, ny, s);
  g_out[v] = b.g;
  key_out[v] = b.key;
}

// ---- x pass: rows staged in LDS -------------------------------------------------------------------------------------------
// A workgroup takes `rows` whole rows, which are contiguous: rows * nx elements from `first`, at most kMaxAxis.
__global__ __launch_bounds__(kBlock) void edt_x_kernel(const double* __restrict__ g, const int32_t* __restrict__ key, int nx, int rows,
                                                       int64_t n_rows, double s, double* __restrict__ g_out,
                                                       int32_t* __restrict__ key_out) {
  __shared__ double sg[kMaxAxis];
  __shared__ int32_t sk[kMaxAxis];
  const int64_t row0 = (int64_t)blockIdx.x * rows;
  const int64_t left = n_rows - row0;
  const int count = (int)(left < rows ? left : rows) * nx;  // <= kMaxAxis: rows = 1 when nx > kBlock, else rows * nx <= kBlock
  const int64_t first = row0 * nx;
  for (int e = threadIdx.x; e < count; e += kBlock) {
    sg[e] = g[first + e];
    sk[e] = key[first + e];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < count; e += kBlock) {
    const int r = e / nx, i = e - r * nx;
    const Best b = scan_outward(sg + r * nx, sk + r * nx, 1, i, nx, s);
    if (g_out) g_out[first + e] = b.g;
    if (key_out) key_out[first + e] = b.key;
  }
}

// ---- fill: out[v] = labels[index[v]] where asked ----------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void edt_fill_kernel(const int32_t* __restrict__ labels, const uint8_t* __restrict__ where,
                                                          const int32_t* __restrict__ index, int64_t n, int32_t* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n) return;
  const int32_t j = index[v];
  const bool take = where[v] != 0 && j >= 0 && (int64_t)j < n;  // an index outside the volume is no site
  out[v] = labels[take ? (int64_t)j : v];
}

// ---- host side ----------------------------------------------------------------------------------------------------------
using namespace t2fit;

int check_volume(const std::string& who, int nz, int ny, int nx) {
  if (nz < 1 || ny < 1 || nx < 1 || nz > kMaxAxis || ny > kMaxAxis || nx > kMaxAxis)
    return fail(T2FIT_E_INVALID, who + ": nz, ny, nx must each be in 1.." + std::to_string(kMaxAxis));
  if ((int64_t)nz * ny * nx >= (1LL << 31)) return fail(T2FIT_E_INVALID, who + ": the volume has 2^31 voxels or more");
  return T2FIT_OK;
}

size_t workspace_need(int64_t n_vox) { return 2 * align_up((size_t)n_vox * sizeof(double), 256) + 2 * align_up((size_t)n_vox * sizeof(int32_t), 256); }

}  // namespace

extern "C" {

int t2fit_edt_workspace_bytes(int nz, int ny, int nx, size_t* bytes) {
  if (!bytes) return fail(T2FIT_E_INVALID, "t2fit_edt_workspace_bytes: bytes is NULL");
  if (int rc = check_volume("t2fit_edt_workspace_bytes", nz, ny, nx)) return rc;
  *bytes = workspace_need((int64_t)nz * ny * nx);
  return T2FIT_OK;
}

int t2fit_edt_dev(const uint8_t* vol_dev, int invert, int nz, int ny, int nx, const double* spacing, double* d2_dev, int32_t* index_dev,
                  void* workspace_dev, size_t workspace_bytes, void* stream) {
  const std::string who = "t2fit_edt_dev";
  if (!vol_dev) return fail(T2FIT_E_INVALID, who + ": vol_dev is NULL");
  if (!d2_dev && !index_dev) return fail(T2FIT_E_INVALID, who + ": d2_dev and index_dev are both NULL, nothing to compute");
  if (invert != 0 && invert != 1) return fail(T2FIT_E_INVALID, who + ": invert must be 0 or 1");
  if (int rc = check_volume(who, nz, ny, nx)) return rc;
  double s[3] = {1.0, 1.0, 1.0};
  for (int a = 0; spacing && a < 3; ++a) {
    s[a] = spacing[a];
    if (!std::isfinite(s[a]) || !(s[a] > 0.0)) return fail(T2FIT_E_INVALID, who + ": spacing must be three finite numbers > 0");
  }
  if ((reinterpret_cast<uintptr_t>(d2_dev) & 7u) || (reinterpret_cast<uintptr_t>(index_dev) & 3u))
    return fail(T2FIT_E_INVALID, who + ": d2_dev / index_dev is not aligned to its element size");
  const int n_vox = (int)((int64_t)nz * ny * nx);
  const size_t need = workspace_need(n_vox);
  if (!workspace_dev) return fail(T2FIT_E_INVALID, who + ": workspace_dev is NULL");
  if (reinterpret_cast<uintptr_t>(workspace_dev) & 255u) return fail(T2FIT_E_INVALID, who + ": workspace_dev is not aligned to 256 bytes");
  if (workspace_bytes < need)
    return fail(T2FIT_E_INVALID, who + ": the workspace has " + std::to_string(workspace_bytes) + " bytes, the call needs " +
                                     std::to_string(need) + " (t2fit_edt_workspace_bytes)");

  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace_dev);
  const size_t g_bytes = align_up((size_t)n_vox * sizeof(double), 256), k_bytes = align_up((size_t)n_vox * sizeof(int32_t), 256);
  double* g_a = reinterpret_cast<double*>(ws);
  double* g_b = reinterpret_cast<double*>(ws + g_bytes);
  int32_t* k_a = reinterpret_cast<int32_t*>(ws + 2 * g_bytes);
  int32_t* k_b = reinterpret_cast<int32_t*>(ws + 2 * g_bytes + k_bytes);
  const int plane = ny * nx;
  hipLaunchKernelGGL(edt_z_kernel, dim3(ceil_div(plane, kBlock)), dim3(kBlock), 0, st, vol_dev, invert, nz, plane, s[0], g_a, k_a);
  hipLaunchKernelGGL(edt_y_kernel, dim3(ceil_div(n_vox, kBlock)), dim3(kBlock), 0, st, (const double*)g_a, (const int32_t*)k_a, ny, nx,
                     n_vox, s[1], g_b, k_b);
  const int rows = nx > kBlock ? 1 : kBlock / nx;
  const int64_t n_rows = (int64_t)nz * ny;
  hipLaunchKernelGGL(edt_x_kernel, dim3((unsigned)ceil_div<int64_t>(n_rows, rows)), dim3(kBlock), 0, st, (const double*)g_b,
                     (const int32_t*)k_b, nx, rows, n_rows, s[2], d2_dev, index_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_edt_fill_dev(const int32_t* labels_dev, const uint8_t* where_dev, const int32_t* index_dev, int64_t n, int32_t* out_dev,
                       void* stream) {
  const std::string who = "t2fit_edt_fill_dev";
  if (!labels_dev || !where_dev || !index_dev || !out_dev)
    return fail(T2FIT_E_INVALID, who + ": labels_dev / where_dev / index_dev / out_dev is NULL");
  if (n < 1 || n >= (1LL << 31)) return fail(T2FIT_E_INVALID, who + ": n must be in 1..2^31-1");
  if ((reinterpret_cast<uintptr_t>(labels_dev) & 3u) || (reinterpret_cast<uintptr_t>(index_dev) & 3u) ||
      (reinterpret_cast<uintptr_t>(out_dev) & 3u))
    return fail(T2FIT_E_INVALID, who + ": an int32 buffer is not aligned to 4 bytes");
  if (out_dev == labels_dev) return fail(T2FIT_E_INVALID, who + ": out_dev must not be labels_dev");
  hipLaunchKernelGGL(edt_fill_kernel, dim3((unsigned)ceil_div<int64_t>(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, labels_dev,
                     where_dev, index_dev, n, out_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

}  // extern "C"

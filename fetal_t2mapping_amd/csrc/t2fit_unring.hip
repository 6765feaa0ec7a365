// t2fit_unring.hip -- Gibbs-ringing removal by local sub-voxel shifts (include/t2fit.h: t2fit_unring_*;
// fetal_t2mapping_amd/_unring.py states the result in numpy and the kernels equal it bit for bit).
//
// Two kernels on v_mfma_f32_32x32x2_f32, whose accumulator is the ordered float32 fma chain of the statement (two contracted
// indices per instruction, ascending).
//
// unring_product_kernel: (stacked DFT table) . (data) for the four DFT stages of the split.  A workgroup owns 32 data columns
// of one slice, staged once in LDS as [contracted index][column] (the B operand of a k-step is 64 consecutive floats); its
// four waves share the row tiles of the table, which stream through LDS in chunks of 32 contracted indices ([row][33]: the A
// operand is read without a bank conflict).  The stacked tables are never built: an element is +-C or +-S by the quadrant it
// lies in.  Operands and results are addressed by (quotient, remainder, column) strides, so no stage needs a transposed
// copy.  The filter table and the subtraction X - I1 are epilogues.
//
// unring_rows_kernel: a workgroup owns 32 lines, in LDS as [position][line].  For every shift it forms Y_j = H_j . X on the
// matrix cores (the circulant's A operand is read from the shift's n taps in LDS, the four waves share the position tiles,
// two accumulators per wave) into a second LDS image, then every lane evaluates the windows of its own samples (line l & 31,
// positions (l >> 5) + 8 i) from that image and keeps the running best (tv, value, shift) in registers.  The shifted copies
// never reach global memory.  The kernel is a template on the samples per lane so that every register index is a constant:
// no scratch.  No atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "t2fit_error.h"
#include "t2fit_support.h"

namespace {

using t2fit::align_up;
using t2fit::ceil_div;
using t2fit::fail;
using t2fit::misaligned;

constexpr uint32_t kMagic = 0x52553254u;
constexpr int kTile = 32;        // rows and columns of one matrix instruction
constexpr int kKC = 32;          // contracted indices of a table chunk in LDS
constexpr int kChunkSlices = 64; // slices the whole stage and the split work on at a time (bounds the workspace)
constexpr double kPi = 3.14159265358979323846;

struct UnringHeader {  // 128 bytes; include/t2fit.h documents the block
  uint32_t magic;
  int32_t nx, ny, K;
  uint32_t reserved[4];
  uint64_t off[8];  // cx, sx, cy, sy, g, hx, hy, ab
  uint64_t bytes;
  uint64_t pad[3];
};
static_assert(sizeof(UnringHeader) == 128, "header layout");

bool sizes_ok(int ny, int nx) { return nx >= T2FIT_UNRING_MIN_N && nx <= T2FIT_UNRING_MAX_N && ny >= T2FIT_UNRING_MIN_N && ny <= T2FIT_UNRING_MAX_N; }
bool shifts_ok(int K) { return K >= 1 && K <= T2FIT_UNRING_MAX_SHIFTS; }

std::string size_message(const char* who, int ny, int nx, int K) {
  return std::string(who) + ": nx and ny must be " + std::to_string(T2FIT_UNRING_MIN_N) + " .. " + std::to_string(T2FIT_UNRING_MAX_N) +
         " and K 1 .. " + std::to_string(T2FIT_UNRING_MAX_SHIFTS) + ", got nx " + std::to_string(nx) + ", ny " + std::to_string(ny) + ", K " +
         std::to_string(K);
}

int check_params(const char* who, const t2fit_unring_params* p, int ny, int nx) {
  if (!p) return fail(T2FIT_E_INVALID, std::string(who) + ": params is NULL");
  if (!sizes_ok(ny, nx) || !shifts_ok(p->K)) return fail(T2FIT_E_INVALID, size_message(who, ny, nx, p->K));
  if (p->min_w < 1 || p->max_w < p->min_w || p->max_w > T2FIT_UNRING_MAX_WINDOW)
    return fail(T2FIT_E_INVALID, std::string(who) + ": the window must be 1 <= min_w <= max_w <= " + std::to_string(T2FIT_UNRING_MAX_WINDOW) +
                                     ", got " + std::to_string(p->min_w) + ", " + std::to_string(p->max_w));
  const int need = 2 * (p->max_w + 1) + 1;
  if (nx < need || ny < need)
    return fail(T2FIT_E_INVALID, std::string(who) + ": the window " + std::to_string(p->min_w) + ", " + std::to_string(p->max_w) +
                                     " needs rows of at least " + std::to_string(need) + " samples, got nx " + std::to_string(nx) + " and ny " +
                                     std::to_string(ny));
  if (p->flags != 0) return fail(T2FIT_E_INVALID, std::string(who) + ": params.flags must be 0");
  return T2FIT_OK;
}

UnringHeader header_for(int ny, int nx, int K) {
  UnringHeader h;
  std::memset(&h, 0, sizeof(h));
  h.magic = kMagic;
  h.nx = nx;
  h.ny = ny;
  h.K = K;
  const size_t nj = 2 * size_t(K) + 1;
  const size_t floats[8] = {size_t(nx) * nx, size_t(nx) * nx, size_t(ny) * ny, size_t(ny) * ny, size_t(ny) * nx, nj * nx, nj * ny, 2 * nj};
  size_t off = sizeof(UnringHeader);
  for (int i = 0; i < 8; ++i) {
    h.off[i] = off;
    off += align_up(floats[i] * sizeof(float), 16);
  }
  h.bytes = off;
  return h;
}

size_t chunk_slices(int n_slices) { return size_t(n_slices < kChunkSlices ? (n_slices < 1 ? 1 : n_slices) : kChunkSlices); }

// workspace: [W1: 2 planes][W2: 2 planes][I1][I2], each plane one image of a chunk of slices, then two flag bytes per slice
struct Workspace {
  size_t plane;  // floats of a chunk of slices
  size_t off_flags, bytes;
};
Workspace workspace_for(int n_slices, int ny, int nx) {
  Workspace w;
  w.plane = chunk_slices(n_slices) * size_t(ny) * nx;
  w.off_flags = align_up(6 * w.plane * sizeof(float), 256);
  w.bytes = w.off_flags + align_up(2 * size_t(n_slices < 1 ? 1 : n_slices), 256);
  return w;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- the table product ------------------------------------------------------------------------------------------------

struct ProductArgs {
  const float* tc;  // the cosine and the sine table, n x n each (symmetric)
  const float* ts;
  int n;
  int M, L;      // rows of the stacked table, contracted length
  int sel, neg;  // bit 2 (m / n) + (k / n): the quadrant is S instead of C; it is negated
  const float* in;  // element (k, c) of slice b at in[b in_batch + (k / kd) skh + (k % kd) skl + c sc]
  int64_t in_batch;
  int kd;
  int64_t skh, skl, sc;
  int ncols;
  float* out;  // element (m, c) at out[b out_batch + (m / md) smh + (m % md) sml + c soc]
  int64_t out_batch;
  int md;
  int64_t smh, sml, soc;
  const float* scale;  // or NULL: the result is multiplied by scale[(m % scale_mod) scale_sm + c]
  int scale_mod;
  int64_t scale_sm;
  const float* minuend;  // or NULL: out2[..] = minuend[..] - result, both addressed as out
  float* out2;
};

__global__ __launch_bounds__(t2fit::kBlock) void unring_product_kernel(ProductArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5;
  const int Lp = (a.L + 1) & ~1;
  float* dl = lds;                                           // the data: [Lp][32]
  float* aw = lds + Lp * kTile + wave * (kTile * (kKC + 1)); // this wave's table chunk: [32 rows][kKC + 1]
  const int c0 = blockIdx.x * kTile;
  const float* in = a.in + int64_t(blockIdx.y) * a.in_batch;
  float* out = a.out + int64_t(blockIdx.y) * a.out_batch;

  for (int i = tid; i < Lp * kTile; i += t2fit::kBlock) {
    int k, c;
    if (a.sc == 1) {
      c = i & 31;
      k = i >> 5;
    } else {
      k = i % Lp;
      c = i / Lp;
    }
    float v = 0.0f;
    if (k < a.L && c0 + c < a.ncols) v = in[int64_t(k / a.kd) * a.skh + int64_t(k % a.kd) * a.skl + int64_t(c0 + c) * a.sc];
    dl[k * kTile + c] = v;
  }

  const int n_mt = ceil_div(a.M, kTile), rounds = ceil_div(n_mt, 4);
  for (int round = 0; round < rounds; ++round) {
    const int m0 = (round * 4 + wave) * kTile;
    const bool valid = m0 < a.M;  // wave-uniform; every wave takes part in the barriers
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int k0 = 0; k0 < Lp; k0 += kKC) {
      __syncthreads();  // the chunk before has been read (and, the first time, the data are staged)
      for (int i = lane; i < kTile * kKC; i += 64) {
        const int r = i >> 5, kk = i & 31, m = m0 + r, k = k0 + kk;
        float v = 0.0f;
        if (m < a.M && k < a.L) {
          const int bit = 2 * (m / a.n) + k / a.n;
          const float* t = ((a.sel >> bit) & 1) ? a.ts : a.tc;
          v = t[(m % a.n) * a.n + k % a.n];
          if ((a.neg >> bit) & 1) v = -v;
        }
        aw[r * (kKC + 1) + kk] = v;
      }
      __syncthreads();
      if (valid) {
        const int steps = (Lp - k0 < kKC ? Lp - k0 : kKC) / 2;
        for (int s = 0; s < steps; ++s) {
          const float av = aw[col * (kKC + 1) + 2 * s + half];     // A[row l & 31][k = 2 s + (l >> 5)]
          const float bv = dl[(k0 + 2 * s + half) * kTile + col];  // B[k = 2 s + (l >> 5)][column l & 31]
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
      }
    }
    const int c = c0 + col;
    if (valid && c < a.ncols) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m >= a.M) continue;
        float v = acc[r];
        if (a.scale) v = v * a.scale[int64_t(m % a.scale_mod) * a.scale_sm + c];
        const int64_t off = int64_t(m / a.md) * a.smh + int64_t(m % a.md) * a.sml + int64_t(c) * a.soc;
        out[off] = v;
        if (a.out2) a.out2[int64_t(blockIdx.y) * a.out_batch + off] = a.minuend[int64_t(blockIdx.y) * a.out_batch + off] - v;
      }
    }
  }
}

size_t product_lds_bytes(int L) { return (size_t((L + 1) & ~1) * kTile + 4 * size_t(kTile) * (kKC + 1)) * sizeof(float); }

hipError_t launch_product(const ProductArgs& a, int n_slices, hipStream_t st) {
  const size_t lds = product_lds_bytes(a.L);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&unring_product_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(unring_product_kernel, dim3(unsigned(ceil_div(a.ncols, kTile)), unsigned(n_slices)), dim3(t2fit::kBlock), lds, st, a);
  return hipGetLastError();
}

// X (n_slices, ny, nx) -> I1, I2; w1 and w2: per slice two planes [part][ny][nx] each
hipError_t split_chunk(const unsigned char* tables, const UnringHeader& h, const float* x, int n_slices, float* w1, float* w2, float* i1,
                       float* i2, hipStream_t st) {
  const int nx = h.nx, ny = h.ny;
  const int64_t plane = int64_t(ny) * nx;
  const float* cx = reinterpret_cast<const float*>(tables + h.off[0]);
  const float* sx = reinterpret_cast<const float*>(tables + h.off[1]);
  const float* cy = reinterpret_cast<const float*>(tables + h.off[2]);
  const float* sy = reinterpret_cast<const float*>(tables + h.off[3]);
  const float* g = reinterpret_cast<const float*>(tables + h.off[4]);
  hipError_t e;
  ProductArgs a;
  // row DFT: [P; Q][kx, y] = [Cx; Sx] . X^T, written as [part][y][kx]
  std::memset(&a, 0, sizeof(a));
  a.tc = cx; a.ts = sx; a.n = nx; a.M = 2 * nx; a.L = nx; a.sel = 0b0100; a.neg = 0;
  a.in = x; a.in_batch = plane; a.kd = nx; a.skh = 0; a.skl = 1; a.sc = nx; a.ncols = ny;
  a.out = w1; a.out_batch = 2 * plane; a.md = nx; a.smh = plane; a.sml = 1; a.soc = nx;
  if ((e = launch_product(a, n_slices, st)) != hipSuccess) return e;
  // column DFT and filter: [A; B] = [[Cy, -Sy], [Sy, Cy]] . [P; Q], times G, written as [part][ky][kx]
  std::memset(&a, 0, sizeof(a));
  a.tc = cy; a.ts = sy; a.n = ny; a.M = 2 * ny; a.L = 2 * ny; a.sel = 0b0110; a.neg = 0b0010;
  a.in = w1; a.in_batch = 2 * plane; a.kd = ny; a.skh = plane; a.skl = nx; a.sc = 1; a.ncols = nx;
  a.out = w2; a.out_batch = 2 * plane; a.md = ny; a.smh = plane; a.sml = nx; a.soc = 1;
  a.scale = g; a.scale_mod = ny; a.scale_sm = nx;
  if ((e = launch_product(a, n_slices, st)) != hipSuccess) return e;
  // inverse column DFT: [Vr; Vi] = [[Cy, Sy], [Sy, -Cy]] . [A; B], written as [part][y][kx]
  a.sel = 0b0110; a.neg = 0b1000;
  a.in = w2; a.out = w1; a.scale = nullptr;
  if ((e = launch_product(a, n_slices, st)) != hipSuccess) return e;
  // real part of the inverse row DFT: I1[x, y] = [Cx, -Sx] . [Vr; Vi]^T, written as [y][x]; I2 = X - I1
  std::memset(&a, 0, sizeof(a));
  a.tc = cx; a.ts = sx; a.n = nx; a.M = nx; a.L = 2 * nx; a.sel = 0b0010; a.neg = 0b0010;
  a.in = w1; a.in_batch = 2 * plane; a.kd = nx; a.skh = plane; a.skl = 1; a.sc = nx; a.ncols = ny;
  a.out = i1; a.out_batch = plane; a.md = nx; a.smh = 0; a.sml = 1; a.soc = nx;
  a.minuend = x; a.out2 = i2;
  return launch_product(a, n_slices, st);
}

// ---- the fused shift and select ---------------------------------------------------------------------------------------

struct RowsArgs {
  const float* taps;  // [2K+1][n]
  const float* ab;    // [2][2K+1]
  int nj, K, n, min_w, max_w;
  const float* in;  // sample l of line r at in[(r / lps) slice_stride + (r % lps) line_stride + l se]
  int64_t n_lines;
  int lps;
  int64_t slice_stride, line_stride, se;
  float* out;  // addressed as in; accumulate: out += result (one float32 addition)
  int accumulate;
  int8_t* shift;  // or NULL
  float* tv;      // or NULL
};

template <int NS>
__global__ __launch_bounds__(t2fit::kBlock) void unring_rows_kernel(RowsArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5;
  const int n = a.n, np = (n + 1) & ~1;
  float* xl = lds;               // the lines: [np][32], the padded position 0.0
  float* yl = xl + np * kTile;   // Y_j: [n][32]
  float* hl = yl + n * kTile;    // the taps of the shift: [n]
  const int64_t r0 = int64_t(blockIdx.x) * kTile;

  for (int i = tid; i < np * kTile; i += t2fit::kBlock) {
    int l, c;
    if (a.se == 1) {
      l = i % np;
      c = i / np;
    } else {
      c = i & 31;
      l = i >> 5;
    }
    const int64_t r = r0 + c;
    float v = 0.0f;
    if (l < n && r < a.n_lines) v = a.in[(r / a.lps) * a.slice_stride + (r % a.lps) * a.line_stride + int64_t(l) * a.se];
    xl[l * kTile + c] = v;
  }
  __syncthreads();

  // this lane's samples: line tid & 31, positions (tid >> 5) + 8 i
  const int scol = tid & 31, srow = tid >> 5;
  float best_tv[NS], best_val[NS];
  int best_j[NS];

  auto select = [&](const float* src, int j) {
    const float wa = a.ab[j], wb = a.ab[a.nj + j];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      int l = srow + 8 * i;
      asm volatile("" : "+v"(l));  // keeps the sample's LDS addresses out of registers between the shifts (they are cheap to form again)
      if (l >= n) continue;
      auto at = [&](int p) {
        if (p < 0) p += n;
        if (p >= n) p -= n;
        return src[p * kTile + scol];
      };
      float tvl = 0.0f, tvr = 0.0f;
      float hi = at(l - a.min_w);
      for (int t = a.min_w; t <= a.max_w; ++t) {  // d[l - t] = |Y[l - t] - Y[l - t - 1]|
        const float lo = at(l - t - 1);
        tvl = tvl + fabsf(hi - lo);
        hi = lo;
      }
      float lo2 = at(l + a.min_w);
      for (int t = a.min_w; t <= a.max_w; ++t) {  // d[l + t + 1] = |Y[l + t + 1] - Y[l + t]|
        const float up = at(l + t + 1);
        tvr = tvr + fabsf(up - lo2);
        lo2 = up;
      }
      const float tv = (tvl != tvl) ? tvl : ((tvr < tvl || tvr != tvr) ? tvr : tvl);  // numpy's minimum: a NaN stays
      if (j == 0) {
        best_tv[i] = tv;
        best_val[i] = at(l);
        best_j[i] = 0;
      } else if (tv < best_tv[i]) {
        const float y = at(l), o = at(j <= a.K ? l - 1 : l + 1);
        const float p = y * wa, q = o * wb;
        best_tv[i] = tv;
        best_val[i] = p + q;
        best_j[i] = j;
      }
      __builtin_amdgcn_sched_barrier(0);  // one sample at a time: interleaving the unrolled samples costs registers, and LDS latency is hidden by the other waves
    }
  };
  select(xl, 0);

  const int n_lt = ceil_div(n, kTile);
  for (int j = 1; j < a.nj; ++j) {
    for (int i = tid; i < n; i += t2fit::kBlock) hl[i] = a.taps[int64_t(j) * n + i];
    __syncthreads();  // (also: every lane has read the Y of the shift before)
    for (int base = 0; base < n_lt; base += 8) {
      const int l0 = (base + wave) * kTile, l1 = (base + 4 + wave) * kTile;
      if (l0 >= n) break;
      const bool two = l1 < n;
      f32x16 acc0, acc1;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
      // A[row][m] = h[(l - m) mod n] at l = l0 + (lane & 31), m = 2 s + (lane >> 5)
      int i0 = (l0 + col - half + n) % n, i1 = (l1 + col - half + n) % n;
      for (int s = 0; s < np / 2; ++s) {
        const int m = 2 * s + half;
        const float bv = xl[m * kTile + col];
        const float a0 = m < n ? hl[i0] : 0.0f;
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc0, 0, 0, 0);
        if (two) {
          const float a1 = m < n ? hl[i1] : 0.0f;
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc1, 0, 0, 0);
        }
        i0 -= 2;
        if (i0 < 0) i0 += n;
        i1 -= 2;
        if (i1 < 0) i1 += n;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        if (l0 + row < n) yl[(l0 + row) * kTile + col] = acc0[r];
        if (two && l1 + row < n) yl[(l1 + row) * kTile + col] = acc1[r];
      }
    }
    __syncthreads();
    select(yl, j);
  }

  const int64_t r = r0 + scol;
  if (r < a.n_lines) {
    const int64_t base = (r / a.lps) * a.slice_stride + (r % a.lps) * a.line_stride;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int l = srow + 8 * i;
      if (l >= n) continue;
      const int64_t off = base + int64_t(l) * a.se;
      a.out[off] = a.accumulate ? a.out[off] + best_val[i] : best_val[i];
      if (a.shift) a.shift[off] = int8_t(best_j[i]);
      if (a.tv) a.tv[off] = best_tv[i];
    }
  }
}

size_t rows_lds_bytes(int n) { return (size_t((n + 1) & ~1) * kTile + size_t(n) * kTile + size_t(n)) * sizeof(float); }

template <int NS> hipError_t launch_rows_ns(const RowsArgs& a, hipStream_t st) {
  const size_t lds = rows_lds_bytes(a.n);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&unring_rows_kernel<NS>), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(unring_rows_kernel<NS>, dim3(unsigned(ceil_div<int64_t>(a.n_lines, kTile))), dim3(t2fit::kBlock), lds, st, a);
  return hipGetLastError();
}

// axis 0: the lines run along x; axis 1: along y (by addressing)
hipError_t launch_rows(const unsigned char* tables, const UnringHeader& h, const t2fit_unring_params& p, const float* in, int n_slices, int ny,
                       int nx, int axis, float* out, bool accumulate, int8_t* shift, float* tv, hipStream_t st) {
  RowsArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n = axis == 0 ? nx : ny;
  a.taps = reinterpret_cast<const float*>(tables + h.off[axis == 0 ? 5 : 6]);
  a.ab = reinterpret_cast<const float*>(tables + h.off[7]);
  a.K = h.K;
  a.nj = 2 * h.K + 1;
  a.min_w = p.min_w;
  a.max_w = p.max_w;
  a.in = in;
  a.lps = axis == 0 ? ny : nx;
  a.n_lines = int64_t(n_slices) * a.lps;
  a.slice_stride = int64_t(ny) * nx;
  a.line_stride = axis == 0 ? nx : 1;
  a.se = axis == 0 ? 1 : nx;
  a.out = out;
  a.accumulate = accumulate ? 1 : 0;
  a.shift = shift;
  a.tv = tv;
  if (a.n <= 64) return launch_rows_ns<8>(a, st);
  if (a.n <= 128) return launch_rows_ns<16>(a, st);
  if (a.n <= 256) return launch_rows_ns<32>(a, st);
  return launch_rows_ns<64>(a, st);
}

// ---- slices that are copied through -----------------------------------------------------------------------------------

// flags: [0][s] = 1 when slice s holds a non-finite sample, [1][s] = 1 when a sample differs from the slice's first
// (plain stores of the constant 1: no atomics)
__global__ __launch_bounds__(t2fit::kBlock) void unring_flags_kernel(const float* __restrict__ x, int64_t plane, int n_slices,
                                                                     uint8_t* __restrict__ flags) {
  const int s = blockIdx.x;
  const float* p = x + int64_t(s) * plane;
  const float first = p[0];
  bool nonfinite = false, varies = false;
  for (int64_t i = threadIdx.x; i < plane; i += t2fit::kBlock) {
    const float v = p[i];
    nonfinite = nonfinite || !isfinite(v);
    varies = varies || v != first;
  }
  if (nonfinite) flags[s] = 1;
  if (varies) flags[n_slices + s] = 1;
}

__global__ __launch_bounds__(t2fit::kBlock) void unring_copy_kernel(const float* __restrict__ x, int64_t plane, int n_slices,
                                                                    const uint8_t* __restrict__ flags, float* __restrict__ out) {
  const int s = blockIdx.x;
  if (flags[s] == 0 && flags[n_slices + s] != 0) return;
  for (int64_t i = threadIdx.x; i < plane; i += t2fit::kBlock) out[int64_t(s) * plane + i] = x[int64_t(s) * plane + i];
}

// reads the header back from the device (one copy and one wait on the stream) and checks it against the call (a size or K
// of 0 is not compared: the rows along one axis read the tables of that axis only)
int read_header(const char* who, const void* tables_dev, int ny, int nx, int K, hipStream_t st, UnringHeader* h) {
  T2_HIP(hipMemcpyAsync(h, tables_dev, sizeof(*h), hipMemcpyDeviceToHost, st));
  T2_HIP(hipStreamSynchronize(st));
  if (h->magic != kMagic) return fail(T2FIT_E_INVALID, std::string(who) + ": tables_dev does not hold the tables of t2fit_unring_tables_host (magic)");
  if ((nx > 0 && h->nx != nx) || (ny > 0 && h->ny != ny) || (K > 0 && h->K != K))
    return fail(T2FIT_E_INVALID, std::string(who) + ": the tables were built for nx " + std::to_string(h->nx) + ", ny " + std::to_string(h->ny) +
                                     ", K " + std::to_string(h->K) + ", the call has nx " + std::to_string(nx) + ", ny " + std::to_string(ny) +
                                     (K > 0 ? ", K " + std::to_string(K) : std::string()));
  if (!shifts_ok(h->K)) return fail(T2FIT_E_INVALID, std::string(who) + ": the table header has K out of range");
  if (!sizes_ok(h->ny, h->nx)) return fail(T2FIT_E_INVALID, std::string(who) + ": the table header has sizes out of range");
  const UnringHeader want = header_for(h->ny, h->nx, h->K);
  if (std::memcmp(h->off, want.off, sizeof(want.off)) != 0 || h->bytes != want.bytes)
    return fail(T2FIT_E_INVALID, std::string(who) + ": the table header is not what t2fit_unring_tables_host writes");
  return T2FIT_OK;
}

int check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need) {
  if (!ws || misaligned(ws, 256)) return fail(T2FIT_E_INVALID, std::string(who) + ": workspace_dev is NULL or not aligned to 256 bytes");
  if (ws_bytes < need)
    return fail(T2FIT_E_INVALID, std::string(who) + ": the workspace has " + std::to_string(ws_bytes) + " bytes, the call needs " + std::to_string(need));
  return T2FIT_OK;
}

}  // namespace

extern "C" {

int t2fit_unring_params_default(t2fit_unring_params* p) {
  if (!p) return fail(T2FIT_E_INVALID, "t2fit_unring_params_default: params is NULL");
  p->K = 20;
  p->min_w = 1;
  p->max_w = 3;
  p->flags = 0;
  return T2FIT_OK;
}

int t2fit_unring_tables_bytes(int ny, int nx, int K, size_t* bytes) {
  if (!bytes) return fail(T2FIT_E_INVALID, "t2fit_unring_tables_bytes: bytes is NULL");
  if (!sizes_ok(ny, nx) || !shifts_ok(K)) return fail(T2FIT_E_INVALID, size_message("t2fit_unring_tables_bytes", ny, nx, K));
  *bytes = header_for(ny, nx, K).bytes;
  return T2FIT_OK;
}

int t2fit_unring_tables_host(int ny, int nx, int K, void* tables_host, size_t bytes) {
  if (!sizes_ok(ny, nx) || !shifts_ok(K)) return fail(T2FIT_E_INVALID, size_message("t2fit_unring_tables_host", ny, nx, K));
  if (!tables_host) return fail(T2FIT_E_INVALID, "t2fit_unring_tables_host: tables_host is NULL");
  const UnringHeader h = header_for(ny, nx, K);
  if (bytes < h.bytes)
    return fail(T2FIT_E_INVALID, "t2fit_unring_tables_host: the buffer has " + std::to_string(bytes) + " bytes, the tables need " +
                                     std::to_string(h.bytes));
  unsigned char* out = static_cast<unsigned char*>(tables_host);
  std::memset(out, 0, h.bytes);
  std::memcpy(out, &h, sizeof(h));
  const int nj = 2 * K + 1;
  std::vector<double> shift(nj, 0.0);
  for (int j = 1; j <= K; ++j) {
    shift[j] = double(j) / double(nj);
    shift[K + j] = -double(j) / double(nj);
  }
  for (int axis = 0; axis < 2; ++axis) {
    const int n = axis == 0 ? nx : ny;
    float* c = reinterpret_cast<float*>(out + h.off[2 * axis]);
    float* s = reinterpret_cast<float*>(out + h.off[2 * axis + 1]);
    for (int k = 0; k < n; ++k)
      for (int m = 0; m < n; ++m) {
        const double arg = 2.0 * kPi * double((int64_t(k) * m) % n) / double(n);
        c[size_t(k) * n + m] = float(std::cos(arg));
        s[size_t(k) * n + m] = float(std::sin(arg));
      }
    float* t = reinterpret_cast<float*>(out + h.off[5 + axis]);
    t[0] = 1.0f;  // row 0: the identity, which no product reads
    for (int j = 1; j < nj; ++j)
      for (int d = 0; d < n; ++d) {
        const double u = double(d) + shift[j];
        double acc = 1.0;
        for (int k = 1; k < (n + 1) / 2; ++k) acc = acc + 2.0 * std::cos(2.0 * kPi * double(k) * u / double(n));
        if (n % 2 == 0) acc = acc + std::cos(kPi * double(d)) * std::cos(kPi * shift[j]);
        t[size_t(j) * n + d] = float(acc / double(n));
      }
  }
  float* g = reinterpret_cast<float*>(out + h.off[4]);
  for (int ky = 0; ky < ny; ++ky)
    for (int kx = 0; kx < nx; ++kx) {
      const double cx = 1.0 + std::cos(2.0 * kPi * double(kx) / double(nx)), cy = 1.0 + std::cos(2.0 * kPi * double(ky) / double(ny));
      const double den = cx + cy;
      g[size_t(ky) * nx + kx] = float((den == 0.0 ? 0.5 : cy / den) / double(nx * ny));
    }
  float* ab = reinterpret_cast<float*>(out + h.off[7]);
  for (int j = 0; j < nj; ++j) {
    ab[j] = float(1.0 - std::fabs(shift[j]));
    ab[nj + j] = float(std::fabs(shift[j]));
  }
  return T2FIT_OK;
}

int t2fit_unring_workspace_bytes(const t2fit_unring_params* params, int n_slices, int ny, int nx, size_t* bytes) {
  if (!bytes) return fail(T2FIT_E_INVALID, "t2fit_unring_workspace_bytes: bytes is NULL");
  if (int rc = check_params("t2fit_unring_workspace_bytes", params, ny, nx)) return rc;
  if (n_slices < 0) return fail(T2FIT_E_INVALID, "t2fit_unring_workspace_bytes: n_slices is negative");
  *bytes = workspace_for(n_slices, ny, nx).bytes;
  return T2FIT_OK;
}

int t2fit_unring_split_dev(const void* tables_dev, const float* in_dev, int n_slices, int ny, int nx, float* i1_dev, float* i2_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream) {
  const char* who = "t2fit_unring_split_dev";
  if (!tables_dev || !in_dev || !i1_dev || !i2_dev) return fail(T2FIT_E_INVALID, std::string(who) + ": tables_dev, in_dev, i1_dev or i2_dev is NULL");
  if (!sizes_ok(ny, nx)) return fail(T2FIT_E_INVALID, size_message(who, ny, nx, 1));
  if (n_slices < 0) return fail(T2FIT_E_INVALID, std::string(who) + ": n_slices is negative");
  if (misaligned(in_dev, 4) || misaligned(i1_dev, 4) || misaligned(i2_dev, 4) || misaligned(tables_dev, 16))
    return fail(T2FIT_E_INVALID, std::string(who) + ": in_dev, i1_dev and i2_dev must be aligned to 4 bytes, tables_dev to 16");
  if (i1_dev == in_dev || i2_dev == in_dev || i1_dev == i2_dev) return fail(T2FIT_E_INVALID, std::string(who) + ": in_dev, i1_dev and i2_dev must differ");
  const Workspace w = workspace_for(n_slices, ny, nx);
  if (int rc = check_workspace(who, workspace_dev, workspace_bytes, w.bytes)) return rc;
  if (n_slices == 0) return T2FIT_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  UnringHeader h;
  if (int rc = read_header(who, tables_dev, ny, nx, 0, st, &h)) return rc;
  float* ws = static_cast<float*>(workspace_dev);
  const int64_t plane = int64_t(ny) * nx;
  const int chunk = int(chunk_slices(n_slices));
  for (int s0 = 0; s0 < n_slices; s0 += chunk) {
    const int sc = n_slices - s0 < chunk ? n_slices - s0 : chunk;
    T2_HIP(split_chunk(static_cast<const unsigned char*>(tables_dev), h, in_dev + s0 * plane, sc, ws, ws + 2 * w.plane, i1_dev + s0 * plane,
                       i2_dev + s0 * plane, st));
  }
  return T2FIT_OK;
}

int t2fit_unring_rows_dev(const t2fit_unring_params* params, const void* tables_dev, const float* in_dev, int n_slices, int ny, int nx, int axis,
                          float* out_dev, int8_t* shift_dev, float* tv_dev, void* stream) {
  const char* who = "t2fit_unring_rows_dev";
  if (axis != 0 && axis != 1) return fail(T2FIT_E_INVALID, std::string(who) + ": axis must be 0 (along x) or 1 (along y), got " + std::to_string(axis));
  // the limits hold for the axis the rows run along; across it, any count from 1 to the largest size
  const int n = axis == 0 ? nx : ny, across = axis == 0 ? ny : nx;
  if (int rc = check_params(who, params, n, n)) return rc;
  if (across < 1 || across > T2FIT_UNRING_MAX_N)
    return fail(T2FIT_E_INVALID, std::string(who) + ": the size across the rows must be 1 .. " + std::to_string(T2FIT_UNRING_MAX_N) + ", got " +
                                     std::to_string(across));
  if (!tables_dev || !in_dev || !out_dev) return fail(T2FIT_E_INVALID, std::string(who) + ": tables_dev, in_dev or out_dev is NULL");
  if (n_slices < 0) return fail(T2FIT_E_INVALID, std::string(who) + ": n_slices is negative");
  if (misaligned(in_dev, 4) || misaligned(out_dev, 4) || misaligned(tv_dev, 4) || misaligned(tables_dev, 16))
    return fail(T2FIT_E_INVALID, std::string(who) + ": in_dev, out_dev and tv_dev must be aligned to 4 bytes, tables_dev to 16");
  if (out_dev == in_dev) return fail(T2FIT_E_INVALID, std::string(who) + ": out_dev must not be in_dev");
  if (n_slices == 0) return T2FIT_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  UnringHeader h;
  if (int rc = read_header(who, tables_dev, axis == 1 ? ny : 0, axis == 0 ? nx : 0, params->K, st, &h)) return rc;
  T2_HIP(launch_rows(static_cast<const unsigned char*>(tables_dev), h, *params, in_dev, n_slices, ny, nx, axis, out_dev, false, shift_dev, tv_dev,
                     st));
  return T2FIT_OK;
}

int t2fit_unring_dev(const t2fit_unring_params* params, const void* tables_dev, const float* in_dev, int n_slices, int ny, int nx, float* out_dev,
                     int8_t* shift_dev, float* tv_dev, int64_t* skipped, void* workspace_dev, size_t workspace_bytes, void* stream) {
  const char* who = "t2fit_unring_dev";
  if (int rc = check_params(who, params, ny, nx)) return rc;
  if (!tables_dev || !in_dev || !out_dev) return fail(T2FIT_E_INVALID, std::string(who) + ": tables_dev, in_dev or out_dev is NULL");
  if (n_slices < 0) return fail(T2FIT_E_INVALID, std::string(who) + ": n_slices is negative");
  if (misaligned(in_dev, 4) || misaligned(out_dev, 4) || misaligned(tv_dev, 4) || misaligned(tables_dev, 16))
    return fail(T2FIT_E_INVALID, std::string(who) + ": in_dev, out_dev and tv_dev must be aligned to 4 bytes, tables_dev to 16");
  if (out_dev == in_dev) return fail(T2FIT_E_INVALID, std::string(who) + ": out_dev must not be in_dev");
  const Workspace w = workspace_for(n_slices, ny, nx);
  if (int rc = check_workspace(who, workspace_dev, workspace_bytes, w.bytes)) return rc;
  if (skipped) *skipped = 0;
  if (n_slices == 0) return T2FIT_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  UnringHeader h;
  if (int rc = read_header(who, tables_dev, ny, nx, params->K, st, &h)) return rc;
  const unsigned char* tables = static_cast<const unsigned char*>(tables_dev);
  float* ws = static_cast<float*>(workspace_dev);
  uint8_t* flags = static_cast<uint8_t*>(workspace_dev) + w.off_flags;
  const int64_t plane = int64_t(ny) * nx, all = int64_t(n_slices) * plane;
  const int chunk = int(chunk_slices(n_slices));
  float* i1 = ws + 4 * w.plane;
  float* i2 = ws + 5 * w.plane;
  for (int s0 = 0; s0 < n_slices; s0 += chunk) {
    const int sc = n_slices - s0 < chunk ? n_slices - s0 : chunk;
    const int64_t o = s0 * plane;
    T2_HIP(split_chunk(tables, h, in_dev + o, sc, ws, ws + 2 * w.plane, i1, i2, st));
    T2_HIP(launch_rows(tables, h, *params, i1, sc, ny, nx, 0, out_dev + o, false, shift_dev ? shift_dev + o : nullptr, tv_dev ? tv_dev + o : nullptr, st));
    T2_HIP(launch_rows(tables, h, *params, i2, sc, ny, nx, 1, out_dev + o, true, shift_dev ? shift_dev + all + o : nullptr,
                       tv_dev ? tv_dev + all + o : nullptr, st));
  }
  T2_HIP(hipMemsetAsync(flags, 0, 2 * size_t(n_slices), st));
  hipLaunchKernelGGL(unring_flags_kernel, dim3(unsigned(n_slices)), dim3(t2fit::kBlock), 0, st, in_dev, plane, n_slices, flags);
  T2_HIP(hipGetLastError());
  hipLaunchKernelGGL(unring_copy_kernel, dim3(unsigned(n_slices)), dim3(t2fit::kBlock), 0, st, in_dev, plane, n_slices, flags, out_dev);
  T2_HIP(hipGetLastError());
  if (skipped) {
    std::vector<uint8_t> host(size_t(n_slices), 0);
    T2_HIP(hipMemcpyAsync(host.data(), flags, size_t(n_slices), hipMemcpyDeviceToHost, st));
    T2_HIP(hipStreamSynchronize(st));
    int64_t count = 0;
    for (uint8_t f : host) count += f != 0;
    *skipped = count;
  }
  return T2FIT_OK;
}

}  // extern "C"

// devprobe.hip -- TEST INFRASTRUCTURE: the device-side mirror of tests/hostsim.  It compiles the per-lane headers for
// gfx950 -- the side of every `#if defined(__HIP_DEVICE_COMPILE__)` that the host simulator never sees -- and wraps the
// single sequences (exp, square roots, reciprocals, quotients, log, i0e, the wave paths of t2_log_i0e4, one evaluation of
// the lane solver) into small kernels, one thread per element; and one kernel that issues the matrix instruction of the
// dictionary fit as DESIGN.md section 8r documents it and returns its float32 scores.  It is built by tests/devprobe/probe.py into
// tests/devprobe/libt2fit_devprobe.so and loaded only by tests/; the product library and its ABI know nothing of it.
//
// Kernel rules: workgroups of exactly 64 lanes (one wave: the caller decides which elements share the wave-level
// decisions, element i sits in wave i / 64), `if (i < n)` around the work (a partial last wave is exercised too).
// Launchers take host pointers: allocate, copy, launch on the null stream, synchronise, copy back, free; they return the
// HIP error code (0 = hipSuccess) and leave no error pending.  Output buffers are filled with 0xff bytes (NaN) before
// the launch, so an element no lane wrote cannot pass for a result.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../fetal_t2mapping_amd/csrc/t2fit_config.h"
#include "../../fetal_t2mapping_amd/csrc/t2fit_dispatch.h"

using namespace t2fit;

namespace {

constexpr int kWave = 64;

// `n_in` host inputs and `n_out` host outputs (pointer, bytes) -> device buffers d[0 .. n_in + n_out), `launch(d)`
template <class F>
int with_buffers(int n_in, const void* const* in, const size_t* in_bytes, int n_out, void* const* out,
                 const size_t* out_bytes, F&& launch) {
  constexpr int kMax = 8;
  void* d[kMax] = {};
  if (n_in + n_out > kMax) return (int)hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  for (int i = 0; i < n_in + n_out && e == hipSuccess; ++i) {
    const size_t b = i < n_in ? in_bytes[i] : out_bytes[i - n_in];
    e = hipMalloc(&d[i], b ? b : 8);
  }
  for (int i = 0; i < n_in && e == hipSuccess; ++i)
    if (in_bytes[i]) e = hipMemcpy(d[i], in[i], in_bytes[i], hipMemcpyHostToDevice);
  for (int i = 0; i < n_out && e == hipSuccess; ++i)
    if (out_bytes[i]) e = hipMemset(d[n_in + i], 0xff, out_bytes[i]);
  if (e == hipSuccess) {
    launch(d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  for (int i = 0; i < n_out && e == hipSuccess; ++i)
    if (out_bytes[i]) e = hipMemcpy(out[i], d[n_in + i], out_bytes[i], hipMemcpyDeviceToHost);
  for (int i = 0; i < n_in + n_out; ++i)
    if (d[i]) {
      const hipError_t f = hipFree(d[i]);
      if (e == hipSuccess) e = f;
    }
  (void)hipGetLastError();  // nothing stays pending for the next call
  return (int)e;
}

inline unsigned waves(int64_t n) { return (unsigned)((n + kWave - 1) / kWave); }

// ---- unary float64 ----------------------------------------------------------------------------------------------
enum { U_EXP_CORE = 0, U_EXP_LIB, U_SQRT_CORE, U_SQRT_LIB, U_FAST_RCP, U_FAST_RSQRT, U_LOG_LEAN, U_I0E, U_SQRT_CORE_H, U_COUNT };

template <int OP>
__global__ __launch_bounds__(kWave) void k_unary(const double* x, double* y, double* y2, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (i < n) {
    const double v = x[i];
    double r, h = 0.0;
    if constexpr (OP == U_EXP_CORE) r = t2_exp_core(v);
    else if constexpr (OP == U_EXP_LIB) r = exp(v);
    else if constexpr (OP == U_SQRT_CORE) r = t2_sqrt_core(v);
    else if constexpr (OP == U_SQRT_LIB) r = sqrt(v);
    else if constexpr (OP == U_FAST_RCP) r = t2_fast_rcp(v);
    else if constexpr (OP == U_FAST_RSQRT) r = t2_fast_rsqrt(v);
    else if constexpr (OP == U_LOG_LEAN) r = t2_log_lean(v);
    else if constexpr (OP == U_I0E) r = t2_i0e(v);
    else r = t2_sqrt_core_h(v, h);
    y[i] = r;
    y2[i] = h;
  }
}

// ---- binary float64 ---------------------------------------------------------------------------------------------
enum { B_FDIV = 0, B_DIV_BY_RCP, B_DIV_IEEE, B_COUNT };

template <int OP>
__global__ __launch_bounds__(kWave) void k_binary(const double* a, const double* b, double* q, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (i < n) {
    if constexpr (OP == B_FDIV) q[i] = t2_fdiv(a[i], b[i]);
    else if constexpr (OP == B_DIV_BY_RCP) q[i] = t2_div_by_rcp(a[i], b[i], t2_rcp_for_div(b[i]));
    else q[i] = a[i] / b[i];
  }
}

// the shared-seed roots: h from t2_sqrt_core_h(x), then the three ways to the root of a nearby a
__global__ __launch_bounds__(kWave) void k_sqrt_near(const double* x, const double* a, double* near, double* half,
                                                     double* from_h, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (i < n) {
    double h;
    (void)t2_sqrt_core_h(x[i], h);
    near[i] = t2_sqrt_near(a[i], h);
    const double hn = t2_rsqrt_half_near(a[i], h);
    half[i] = hn;
    from_h[i] = t2_sqrt_from_h(a[i], hn);
  }
}

// ---- log(i0e) on rows of four: the wave paths -------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void k_log_i0e4(const double* x, double* out, int64_t n, int near) {
  const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (i < n) {
    double xx[4], r[4];
    for (int j = 0; j < 4; ++j) xx[j] = x[4 * i + j];
    t2_log_i0e4(xx, r, near != 0);
    for (int j = 0; j < 4; ++j) out[4 * i + j] = r[j];
  }
}

// the shared 30-step loop called directly; each row's four arguments on one side of 8 (the caller's business)
__global__ __launch_bounds__(kWave) void k_i0e4_by_lane(const double* x, double* out, int64_t n, int near) {
  const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (i < n) {
    double ax[4], r[4];
    for (int j = 0; j < 4; ++j) ax[j] = x[4 * i + j] < 0 ? -x[4 * i + j] : x[4 * i + j];
    t2_i0e4_by_lane(ax, ax[0] <= 8.0, r, near != 0);
    for (int j = 0; j < 4; ++j) out[4 * i + j] = r[j];
  }
}

// ---- float32 intrinsics of the LM path ----------------------------------------------------------------------------
enum { F_EXP = 0, F_LOG, F_RSQRT, F_RCP, F_COUNT };

template <int OP>
__global__ __launch_bounds__(kWave) void k_unary_f32(const float* x, float* y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (i < n) {
    if constexpr (OP == F_EXP) y[i] = t2_exp(x[i]);
    else if constexpr (OP == F_LOG) y[i] = t2_log(x[i]);
    else if constexpr (OP == F_RSQRT) y[i] = t2_rsqrt(x[i]);
    else y[i] = t2_rcp(x[i]);
  }
}

// ---- one evaluation of the lane solver ----------------------------------------------------------------------------
// The solver is set up the way hostsim_rician_eval does it on the host: samples prepared, bounds of the lane, init(), the
// point written into x, (specialised echo count: the samples into the solver's registers), one eval().
template <int MODEL, int NTE>
__global__ __launch_bounds__(kWave) void k_eval(const LaneParams P, const float* rows, const double* xs, double* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (i < n) {
    float buf[T2FIT_MAX_TE];
    for (int e = 0; e < P.n_te; ++e) buf[e] = rows[i * P.n_te + e];
    bool finite;
    float y0_raw;
    const ObjCtx c = prepare_samples(P, buf, 1, finite, y0_raw);
    double lb[3], ub[3];
    lane_bounds(P, y0_raw, lb, ub);
    Lbfgsb<MODEL, NTE> s;
    s.init(xs + 3 * i, lb, ub, nullptr, 1);
    for (int j = 0; j < s.N; ++j) s.x[j] = xs[3 * i + j];
    if constexpr (NTE > 0)
      for (int e = 0; e < NTE; ++e) s.ys[e] = buf[e];
    s.eval(c);
    out[4 * i] = s.f;
    for (int j = 0; j < 3; ++j) out[4 * i + 1 + j] = j < s.N ? s.g[j] : 0.0;
  }
}

// ---- the float32 scores of the dictionary fit on the matrix cores ------------------------------------------------------
// What DESIGN.md section 8r documents, written from the document and not from the product kernel: one wave per 32-atom
// tile and 32-voxel group; lane l supplies A[row l & 31][k = l >> 5] (a normalised atom, from the packed block's
// [tile][echo][32 rows]) and B[k = l >> 5][voxel l & 31] (a sample); one v_mfma_f32_32x32x2_f32 per pair of echoes, in
// ascending order, into one accumulator; accumulator register r of lane l is the score of row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5) for the voxel l & 31.  out: (n_vox, 32 n_tiles) float32.
struct DictBlockHeader {  // the 64-byte header of the packed dictionary (include/t2fit.h)
  uint32_t magic;
  int32_t n_atoms, n_te, k_pad, n_tiles;
  float dmax;
  uint32_t reserved[2];
  uint64_t off_tiles, off_atoms, off_norm2, bytes;
};
static_assert(sizeof(DictBlockHeader) == 64, "header layout");

typedef float probe_f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(kWave) void k_dict_scores(const unsigned char* packed, const float* y, int64_t n_vox, float* out) {
  const DictBlockHeader* h = reinterpret_cast<const DictBlockHeader*>(packed);
  const int tile = blockIdx.x, lane = threadIdx.x, col = lane & 31, half = lane >> 5;
  const int n_te = h->n_te, k_pad = h->k_pad;
  const int64_t width = (int64_t)h->n_tiles * 32;
  const float* rows = reinterpret_cast<const float*>(packed + h->off_tiles) + (size_t)tile * k_pad * 32;
  const int64_t v = (int64_t)blockIdx.y * 32 + col;
  probe_f32x16 acc;
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  for (int s = 0; s < k_pad / 2; ++s) {  // (all 64 lanes take every step: the instruction needs the whole wave)
    const int k = 2 * s + half;
    const float a = rows[k * 32 + col];
    const float b = (k < n_te && v < n_vox) ? y[(int64_t)k * n_vox + v] : 0.0f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
  if (v < n_vox)
    for (int r = 0; r < 16; ++r) out[v * width + tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * half] = acc[r];
}

}  // namespace

#define PROBE_CASE(K, OP, ...) \
  case OP: hipLaunchKernelGGL((K<OP>), dim3(waves(n)), dim3(kWave), 0, 0, __VA_ARGS__); break;

// op: U_* above.  y2 receives h of t2_sqrt_core_h (0 for the other operations).
extern "C" int devprobe_unary(int op, const double* x, int64_t n, double* y, double* y2) {
  if (op < 0 || op >= U_COUNT || n < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t b = (size_t)n * sizeof(double);
  const void* in[] = {x};
  void* out[] = {y, y2};
  const size_t inb[] = {b}, outb[] = {b, b};
  return with_buffers(1, in, inb, 2, out, outb, [&](void** d) {
    const double* dx = (const double*)d[0];
    double *dy = (double*)d[1], *dy2 = (double*)d[2];
    switch (op) {
      PROBE_CASE(k_unary, U_EXP_CORE, dx, dy, dy2, n)
      PROBE_CASE(k_unary, U_EXP_LIB, dx, dy, dy2, n)
      PROBE_CASE(k_unary, U_SQRT_CORE, dx, dy, dy2, n)
      PROBE_CASE(k_unary, U_SQRT_LIB, dx, dy, dy2, n)
      PROBE_CASE(k_unary, U_FAST_RCP, dx, dy, dy2, n)
      PROBE_CASE(k_unary, U_FAST_RSQRT, dx, dy, dy2, n)
      PROBE_CASE(k_unary, U_LOG_LEAN, dx, dy, dy2, n)
      PROBE_CASE(k_unary, U_I0E, dx, dy, dy2, n)
      PROBE_CASE(k_unary, U_SQRT_CORE_H, dx, dy, dy2, n)
    }
  });
}

// op: B_* above.
extern "C" int devprobe_binary(int op, const double* a, const double* b, int64_t n, double* q) {
  if (op < 0 || op >= B_COUNT || n < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t bytes = (size_t)n * sizeof(double);
  const void* in[] = {a, b};
  void* out[] = {q};
  const size_t inb[] = {bytes, bytes}, outb[] = {bytes};
  return with_buffers(2, in, inb, 1, out, outb, [&](void** d) {
    const double *da = (const double*)d[0], *db = (const double*)d[1];
    double* dq = (double*)d[2];
    switch (op) {
      PROBE_CASE(k_binary, B_FDIV, da, db, dq, n)
      PROBE_CASE(k_binary, B_DIV_BY_RCP, da, db, dq, n)
      PROBE_CASE(k_binary, B_DIV_IEEE, da, db, dq, n)
    }
  });
}

extern "C" int devprobe_sqrt_near(const double* x, const double* a, int64_t n, double* near, double* half, double* from_h) {
  if (n < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t bytes = (size_t)n * sizeof(double);
  const void* in[] = {x, a};
  void* out[] = {near, half, from_h};
  const size_t inb[] = {bytes, bytes}, outb[] = {bytes, bytes, bytes};
  return with_buffers(2, in, inb, 3, out, outb, [&](void** d) {
    hipLaunchKernelGGL(k_sqrt_near, dim3(waves(n)), dim3(kWave), 0, 0, (const double*)d[0], (const double*)d[1],
                       (double*)d[2], (double*)d[3], (double*)d[4], n);
  });
}

// x, out: n rows of four.  by_lane != 0: t2_i0e4_by_lane directly (values of i0e), else t2_log_i0e4 (their logarithms).
extern "C" int devprobe_i0e4(int by_lane, const double* x, int64_t n, int near, double* out) {
  if (n < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t bytes = (size_t)n * 4 * sizeof(double);
  const void* in[] = {x};
  void* outp[] = {out};
  const size_t inb[] = {bytes}, outb[] = {bytes};
  return with_buffers(1, in, inb, 1, outp, outb, [&](void** d) {
    if (by_lane) hipLaunchKernelGGL(k_i0e4_by_lane, dim3(waves(n)), dim3(kWave), 0, 0, (const double*)d[0], (double*)d[1], n, near);
    else hipLaunchKernelGGL(k_log_i0e4, dim3(waves(n)), dim3(kWave), 0, 0, (const double*)d[0], (double*)d[1], n, near);
  });
}

// op: F_* above.
extern "C" int devprobe_unary_f32(int op, const float* x, int64_t n, float* y) {
  if (op < 0 || op >= F_COUNT || n < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t bytes = (size_t)n * sizeof(float);
  const void* in[] = {x};
  void* out[] = {y};
  const size_t inb[] = {bytes}, outb[] = {bytes};
  return with_buffers(1, in, inb, 1, out, outb, [&](void** d) {
    const float* dx = (const float*)d[0];
    float* dy = (float*)d[1];
    switch (op) {
      PROBE_CASE(k_unary_f32, F_EXP, dx, dy, n)
      PROBE_CASE(k_unary_f32, F_LOG, dx, dy, n)
      PROBE_CASE(k_unary_f32, F_RSQRT, dx, dy, n)
      PROBE_CASE(k_unary_f32, F_RCP, dx, dy, n)
    }
  });
}

// One Lbfgsb<MODEL>::eval per row: rows (n, cfg.n_te) float32, xs (n, 3) float64 -> out (n, 4) = f, g0, g1, g2.
// nte_special != 0: the echo-count specialisation (built for six echoes only), else the run-time echo count.
extern "C" int devprobe_eval(const t2fit_config* cfg, const float* rows, const double* xs, int64_t n, int nte_special,
                             double* out) {
  const char* why;
  const int rc = config_check(cfg, &why);
  if (rc != T2FIT_OK || n < 0) return (int)hipErrorInvalidValue;
  if (nte_special && cfg->n_te != 6) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const LaneParams P = make_lane_params(*cfg);
  const void* in[] = {rows, xs};
  void* outp[] = {out};
  const size_t inb[] = {(size_t)n * cfg->n_te * sizeof(float), (size_t)n * 3 * sizeof(double)}, outb[] = {(size_t)n * 4 * sizeof(double)};
  return with_buffers(2, in, inb, 1, outp, outb, [&](void** d) {
    const float* dr = (const float*)d[0];
    const double* dx = (const double*)d[1];
    double* dout = (double*)d[2];
    const dim3 g(waves(n)), b(kWave);
    auto go = [&](auto MC) {
      constexpr int M = decltype(MC)::value;
      if (nte_special) hipLaunchKernelGGL((k_eval<M, 6>), g, b, 0, 0, P, dr, dx, dout, n);
      else hipLaunchKernelGGL((k_eval<M, 0>), g, b, 0, 0, P, dr, dx, dout, n);
    };
    if (P.model == T2FIT_MODEL_GAUSSIAN) go(std::integral_constant<int, T2FIT_MODEL_GAUSSIAN>{});
    else if (P.model == T2FIT_MODEL_GAUSSIAN_RICIAN) go(std::integral_constant<int, T2FIT_MODEL_GAUSSIAN_RICIAN>{});
    else go(std::integral_constant<int, T2FIT_MODEL_RICIAN>{});
  });
}

// packed: a block as _dict.pack / t2fit_dict_pack_host writes it (`bytes` long); y: (n_te, n_vox) float32;
// out: (n_vox, 32 n_tiles) float32, the float32 score of every (voxel, row of a tile), padded rows included.
extern "C" int devprobe_dict_scores(const void* packed, size_t bytes, const float* y, int n_te, int64_t n_vox, float* out) {
  if (!packed || !y || !out || bytes < sizeof(DictBlockHeader) || n_vox < 0 || n_vox > (1 << 20)) return (int)hipErrorInvalidValue;
  DictBlockHeader h;
  memcpy(&h, packed, sizeof(h));
  // the header is what the kernel indexes with: nothing is launched unless it describes this block
  if (h.magic != 0x54443254u || h.n_te != n_te || n_te < 2 || n_te > T2FIT_MAX_TE || h.k_pad != (n_te + 1) / 2 * 2 || h.n_atoms < 1 ||
      h.n_atoms > T2FIT_DICT_MAX_ATOMS || h.n_tiles != (h.n_atoms + 31) / 32 || h.off_tiles != sizeof(DictBlockHeader) || h.bytes != bytes ||
      h.off_tiles + (uint64_t)h.n_tiles * h.k_pad * 32 * sizeof(float) > bytes)
    return (int)hipErrorInvalidValue;
  if (n_vox == 0) return 0;
  const int64_t groups = (n_vox + 31) / 32;
  const void* in[] = {packed, y};
  void* outp[] = {out};
  const size_t inb[] = {bytes, (size_t)n_te * n_vox * sizeof(float)}, outb[] = {(size_t)n_vox * h.n_tiles * 32 * sizeof(float)};
  return with_buffers(2, in, inb, 1, outp, outb, [&](void** d) {
    hipLaunchKernelGGL(k_dict_scores, dim3((unsigned)h.n_tiles, (unsigned)groups), dim3(kWave), 0, 0, (const unsigned char*)d[0],
                       (const float*)d[1], n_vox, (float*)d[2]);
  });
}

extern "C" int devprobe_config_default(t2fit_config* cfg, int model, int low_field) {
  return config_default_impl(cfg, model, low_field);
}

// number of devices this process can see (0 and the error swallowed where there is none)
extern "C" int devprobe_device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  (void)hipGetLastError();
  return n;
}

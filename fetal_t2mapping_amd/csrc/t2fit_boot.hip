// t2fit_boot.hip -- gfx950 kernels and C ABI of the parametric bootstrap (include/t2fit.h: t2fit_boot_background_dev,
// t2fit_boot_synth_dev, t2fit_bootstrap_dev).  No reference counterpart: the reference has no uncertainty map.
//
// The estimator whose spread is wanted is the fit as it is run: solver, bounds, prior and stop rules included.  So the
// acquisition is simulated from the fitted (k, T2) with Rician noise, refitted by the SAME entry point
// (t2fit_volume_dev, untouched) and the per-voxel distribution of the R refits is reduced to bias, standard deviation
// and a percentile interval.  Four kernels: the replica synthesis (counter-based Philox4x32-10, so a sample is a
// function of (seed, voxel, echo, replica) alone), the accumulation after each refit (one lane owns one voxel and the
// replicas arrive in order: no atomics, sums fixed), the finalisation (moments, exact rank select on values staged in
// LDS) and the background noise level.  Nothing here shares a header with the fit kernels except the error plumbing,
// the argument checks of t2fit_config.h and the context's streams.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "t2fit_config.h"
#include "t2fit_context.h"
#include "t2fit_error.h"
#include "t2fit_support.h"

namespace {

using t2fit::kBlock;
constexpr int kMaxIntervalReplicas = 512;  // R values of 64 voxels staged in LDS: 512 x 256 B = 128 KiB of the CU's 160 KiB

// ---- the replica stream -----------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of two
// 32 x 32 -> 64 multiplies.  key = (seed low, seed high), counter = (voxel low, voxel high, echo, replica); words 0 and 1
// of the block feed one Box-Muller pair, words 2 and 3 are not used.  fetal_t2mapping_amd/_philox.py restates it in numpy.
__device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                     uint32_t& w0, uint32_t& w1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w0 = c0;
  w1 = c1;
}

// u = ((w >> 9) + 0.5) 2^-23: an odd multiple of 2^-24 below 1, 24 significant bits, so exact in float32 and never 0 or
// 1 (24 bits of w plus the half would need 25).  |n| <= sqrt(-2 ln 2^-24) = 5.77.
template <bool kRician>
__device__ inline float boot_sample(float clean, float s, uint32_t w0, uint32_t w1) {
  const float u1 = ((float)(w0 >> 9) + 0.5f) * 0x1p-23f;
  const float u2 = ((float)(w1 >> 9) + 0.5f) * 0x1p-23f;
  const float rad = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincospif(2.0f * u2, &sn, &cs);
  const float a = clean + s * (rad * cs);
  if (!kRician) return a;
  const float b = s * (rad * sn);
  return sqrtf(a * a + b * b);
}

struct SynthArgs {
  const float* t2;
  const float* k;
  const float* noise_map;  // or nullptr: noise_scalar everywhere
  const uint8_t* mask;     // or nullptr: every voxel
  float* out;              // (n_te, n_vox)
  int64_t n_vox;
  uint64_t voxel_offset;   // flat index of voxel 0 in the volume the counters refer to
  uint32_t key0, key1, replica;
  int n_te;
  float noise_scalar;
  float te[T2FIT_MAX_TE];
};

// One lane makes kV consecutive voxels of every echo: kV = 4 with 128-bit loads and stores when the rows allow it
// (n_vox % 4 == 0, 16-byte aligned buffers), kV = 1 otherwise.  Same samples either way.
template <int kV, bool kRician>
__global__ __launch_bounds__(kBlock) void boot_synth_kernel(const SynthArgs a) {
  const int64_t v0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kV;
  if (v0 >= a.n_vox) return;  // (kV = 4: n_vox % 4 == 0, so v0 + 3 < n_vox as well)
  float t2[kV], k[kV], s[kV], rinv[kV];
  bool in[kV];
  if constexpr (kV == 4) {
    const float4 t = *reinterpret_cast<const float4*>(a.t2 + v0);
    const float4 kk = *reinterpret_cast<const float4*>(a.k + v0);
    t2[0] = t.x; t2[1] = t.y; t2[2] = t.z; t2[3] = t.w;
    k[0] = kk.x; k[1] = kk.y; k[2] = kk.z; k[3] = kk.w;
    if (a.noise_map) {
      const float4 n = *reinterpret_cast<const float4*>(a.noise_map + v0);
      s[0] = n.x; s[1] = n.y; s[2] = n.z; s[3] = n.w;
    } else {
      s[0] = s[1] = s[2] = s[3] = a.noise_scalar;
    }
    const uint32_t m = a.mask ? *reinterpret_cast<const uint32_t*>(a.mask + v0) : 0x01010101u;
#pragma unroll
    for (int i = 0; i < 4; ++i) in[i] = ((m >> (8 * i)) & 255u) != 0u;
  } else {
    t2[0] = a.t2[v0];
    k[0] = a.k[v0];
    s[0] = a.noise_map ? a.noise_map[v0] : a.noise_scalar;
    in[0] = a.mask ? a.mask[v0] != 0 : true;
  }
#pragma unroll
  for (int i = 0; i < kV; ++i) rinv[i] = 1.0f / t2[i];
  for (int j = 0; j < a.n_te; ++j) {
    float o[kV];
#pragma unroll
    for (int i = 0; i < kV; ++i) {
      const uint64_t g = a.voxel_offset + (uint64_t)(v0 + i);
      uint32_t w0, w1;
      philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)j, a.replica, a.key0, a.key1, w0, w1);
      const float clean = k[i] * expf(-a.te[j] * rinv[i]);
      o[i] = in[i] ? boot_sample<kRician>(clean, s[i], w0, w1) : 0.0f;
    }
    float* row = a.out + (int64_t)j * a.n_vox + v0;
    if constexpr (kV == 4) *reinterpret_cast<float4*>(row) = make_float4(o[0], o[1], o[2], o[3]);
    else row[0] = o[0];
  }
}

// ---- accumulation -------------------------------------------------------------------------------------------------------
// Per masked voxel m (rank in the mask) and requested parameter p, about the original fitted value c: sum (x - c),
// sum (x - c)^2 in float64 (shifted, so the variance does not cancel), min and max (all replicas equal <=> std = 0
// exactly) and the count of replicas that count: status CONVERGED and every requested value finite.
//
// The shift is a device for the rounding, not part of the result: a fitted value that is not finite (T2 = +inf of a
// flat signal, handed in as a map) still has finite refits, and their mean and std must not become inf - inf.  Such a
// centre shifts by 0; a finite one by itself, bit for bit as before.  Both kernels use this one function.
__device__ inline double boot_shift(float centre) { return isfinite(centre) ? (double)centre : 0.0; }
struct AccumArgs {
  const int64_t* idx;
  int64_t n_masked;
  const float* rep[3];     // the replica's maps (dense); nullptr = parameter not requested
  const float* centre[3];  // the original fit's maps (dense)
  const uint8_t* status;   // the replica's status map (dense)
  double* sum[3];          // [n_masked] per requested parameter
  double* sumsq[3];
  float* vmin[3];
  float* vmax[3];
  int32_t* n_ok;           // [n_masked]
  float* vals[3];          // (R, n_masked) per parameter or nullptr (moments only)
  int replica;
};

__global__ __launch_bounds__(kBlock) void boot_accum_kernel(const AccumArgs a) {
  const int64_t m = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (m >= a.n_masked) return;
  const int64_t v = a.idx[m];
  float x[3] = {0.0f, 0.0f, 0.0f};
  bool ok = a.status[v] == T2FIT_ST_CONVERGED;
#pragma unroll
  for (int p = 0; p < 3; ++p)
    if (a.rep[p]) {
      x[p] = a.rep[p][v];
      ok = ok && isfinite(x[p]);
    }
  const int32_t n = a.n_ok[m];
  if (ok) a.n_ok[m] = n + 1;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    if (!a.rep[p]) continue;
    if (ok) {
      const double d = (double)x[p] - boot_shift(a.centre[p][v]);
      a.sum[p][m] += d;
      a.sumsq[p][m] += d * d;
      a.vmin[p][m] = n == 0 ? x[p] : fminf(a.vmin[p][m], x[p]);
      a.vmax[p][m] = n == 0 ? x[p] : fmaxf(a.vmax[p][m], x[p]);
    }
    if (a.vals[p]) a.vals[p][(int64_t)a.replica * a.n_masked + m] = ok ? x[p] : INFINITY;
  }
}

// ---- finalisation ---------------------------------------------------------------------------------------------------
struct FinalArgs {
  const int64_t* idx;
  int64_t n_masked;
  const float* centre;   // dense
  const double* sum;     // this parameter's [n_masked]
  const double* sumsq;
  const float* vmin;
  const float* vmax;
  const int32_t* n_ok;
  const float* vals;     // (R, n_masked) or nullptr
  int n_replicas;
  double q_lo, q_hi;     // alpha / 2, 1 - alpha / 2
  float* mean;           // dense outputs, each may be nullptr
  float* bias;
  float* std;
  float* ci_lo;
  float* ci_hi;
  int32_t* n_ok_out;
};

// order-preserving image of a float: a < b  <=>  key(a) < key(b) (no NaN gets here: they are stored as +inf)
__device__ inline uint32_t boot_key(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float boot_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// numpy's default ("linear") percentile of the n smallest of the lane's R staged keys (the others are +inf): the order
// statistics at floor(q (n - 1)) and the one after it, found exactly -- bisection over the 32 bits of the key, one pass
// over the lane's column per bit -- and interpolated in float64 as numpy's _lerp does.
__device__ inline double boot_percentile(const uint32_t* col, int n_replicas, int n, double q) {
  const double pos = q * (double)(n - 1);
  const double fl = floor(pos);
  const int rank = (int)fl;
  const double t = pos - fl;
  uint32_t key = 0u;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t trial = key | (1u << bit);
    int below = 0;
    for (int r = 0; r < n_replicas; ++r) below += col[r * 64] < trial ? 1 : 0;
    if (below <= rank) key = trial;
  }
  int not_above = 0;
  uint32_t next = 0xffffffffu;
  for (int r = 0; r < n_replicas; ++r) {
    const uint32_t c = col[r * 64];
    not_above += c <= key ? 1 : 0;
    next = (c > key && c < next) ? c : next;
  }
  const double lo = (double)boot_unkey(key);
  const double hi = (not_above >= rank + 2 || rank + 1 >= n) ? lo : (double)boot_unkey(next);
  const double diff = hi - lo;
  return t >= 0.5 ? hi - diff * (1.0 - t) : lo + diff * t;
}

// One wave handles 64 voxels.  kInterval: the R values of each lane's voxel are staged in LDS lane-major (word
// r * 64 + lane: a wave's access touches each bank once), R * 256 bytes per workgroup, requested at launch.
template <bool kInterval>
__global__ __launch_bounds__(64) void boot_final_kernel(const FinalArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t staged[];
  const int lane = threadIdx.x;
  const int64_t m = (int64_t)blockIdx.x * 64 + lane;
  const bool act = m < a.n_masked;
  const int64_t mm = act ? m : 0;
  const int n = act ? a.n_ok[mm] : 0;
  const int64_t v = a.idx[mm];
  const double c = (double)a.centre[v], shift = boot_shift(a.centre[v]);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double dmean = nan, sd = nan;
  if (n >= 1) dmean = a.sum[mm] / (double)n;
  if (n >= 2) {
    const double var = (a.sumsq[mm] - a.sum[mm] * dmean) / (double)(n - 1);
    sd = (a.vmin[mm] == a.vmax[mm] || !(var > 0.0)) ? 0.0 : sqrt(var);
  }
  double lo = nan, hi = nan;
  if constexpr (kInterval) {
    for (int r = 0; r < a.n_replicas; ++r)
      staged[r * 64 + lane] = act ? boot_key(a.vals[(int64_t)r * a.n_masked + mm]) : 0xffffffffu;
    const int nn = n >= 1 ? n : 1;  // every lane walks the same loops; lanes without a counted replica discard the result
    const double plo = boot_percentile(staged + lane, a.n_replicas, nn, a.q_lo);
    const double phi = boot_percentile(staged + lane, a.n_replicas, nn, a.q_hi);
    if (n >= 1) {
      lo = plo;
      hi = phi;
    }
  }
  if (!act) return;
  const double mean = shift + dmean;
  if (a.mean) a.mean[v] = (float)mean;
  // a finite centre: the shifted mean is the bias, unrounded; otherwise mean - c by IEEE rules (-inf for c = +inf, NaN for NaN)
  if (a.bias) a.bias[v] = (float)(shift == c ? dmean : mean - c);
  if (a.std) a.std[v] = (float)sd;
  if (a.ci_lo) a.ci_lo[v] = (float)lo;
  if (a.ci_hi) a.ci_hi[v] = (float)hi;
  if (a.n_ok_out) a.n_ok_out[v] = n;
}

// ---- background noise level ---------------------------------------------------------------------------------------------
// sum of S^2 and number of samples over the voxels outside the mask, float64.  The launch is fixed (kBgBlocks x kBlock
// lanes, lane t of block b takes voxels b * kBlock + t + i * kBgBlocks * kBlock) and so is every tree: the result is a
// function of the data alone.
constexpr int kBgBlocks = 1024;

__device__ inline void bg_block_reduce(double s, long long c, double* sh_s, long long* sh_c, double* out_s, long long* out_c,
                                       int slot) {
  const int tid = threadIdx.x;
  sh_s[tid] = s;
  sh_c[tid] = c;
  __syncthreads();
  for (int stride = kBlock / 2; stride >= 1; stride >>= 1) {
    if (tid < stride) {
      sh_s[tid] += sh_s[tid + stride];
      sh_c[tid] += sh_c[tid + stride];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out_s[slot] = sh_s[0];
    out_c[slot] = sh_c[0];
  }
}

__global__ __launch_bounds__(kBlock) void boot_background_kernel(const float* __restrict__ echoes, int layout,
                                                                 const uint8_t* __restrict__ mask, int n_te, int64_t n_vox,
                                                                 double* part_sum, long long* part_cnt) {
  __shared__ double sh_s[kBlock];
  __shared__ long long sh_c[kBlock];
  double s = 0.0;
  long long c = 0;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n_vox; v += (int64_t)kBgBlocks * kBlock) {
    if (mask[v] != 0) continue;
    for (int j = 0; j < n_te; ++j) {
      const double x = (double)(layout == T2FIT_LAYOUT_TE_MAJOR ? echoes[(int64_t)j * n_vox + v] : echoes[v * n_te + j]);
      s += x * x;
    }
    c += n_te;
  }
  bg_block_reduce(s, c, sh_s, sh_c, part_sum, part_cnt, blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void boot_background_final_kernel(const double* part_sum, const long long* part_cnt,
                                                                       double* out_sum, long long* out_cnt) {
  __shared__ double sh_s[kBlock];
  __shared__ long long sh_c[kBlock];
  double s = 0.0;
  long long c = 0;
  for (int i = threadIdx.x; i < kBgBlocks; i += kBlock) {
    s += part_sum[i];
    c += part_cnt[i];
  }
  bg_block_reduce(s, c, sh_s, sh_c, out_sum, out_cnt, 0);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
using t2fit::aligned16;
using t2fit::fail;

// -DT2FIT_BOOT_PHASES (a diagnostic build, never the product): host-clock time of the phases of a bootstrap call on stderr
#ifdef T2FIT_BOOT_PHASES
struct Phases {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void mark(const char* name) {
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[t2fit boot phase] %-28s %9.3f ms\n", name, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};
#else
struct Phases {
  void mark(const char*) {}
};
#endif

// everything a bootstrap call owns; released on every way out of the call
struct BootWorkspace {
  std::vector<void*> dev;
  hipStream_t streams[2] = {nullptr, nullptr};
  bool own_streams = false;
  std::vector<hipEvent_t> events;
  ~BootWorkspace() {
    Phases ph;
    for (hipStream_t s : streams)  // an early way out may leave launches that still use the buffers
      if (s) (void)hipStreamSynchronize(s);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    if (own_streams)
      for (hipStream_t s : streams)
        if (s) (void)hipStreamDestroy(s);
    ph.mark("release: sync, events, streams");
    for (void* p : dev) (void)hipFree(p);
    ph.mark("release: hipFree");
  }
  hipError_t alloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e == hipSuccess) dev.push_back(*p);
    return e;
  }
  hipError_t event(hipEvent_t* e) {
    const hipError_t rc = hipEventCreateWithFlags(e, hipEventDisableTiming);
    if (rc == hipSuccess) events.push_back(*e);
    return rc;
  }
};

std::string gib(double bytes) {
  char b[48];
  snprintf(b, sizeof b, "%.2f GiB", bytes / (1024.0 * 1024.0 * 1024.0));
  return b;
}

int synth_check(const char* who, const t2fit_config* cfg, const float* t2_dev, const float* k_dev, double noise_scalar,
                const float* noise_map_dev, int64_t n_vox, int noise_kind) {
  const char* why;
  const int rc = t2fit::config_check(cfg, &why);
  if (rc != T2FIT_OK) return fail(rc, std::string(who) + ": " + why);
  if (cfg->norm)
    return fail(T2FIT_E_INVALID, std::string(who) + ": cfg.norm = 1 is not supported (the maps of a normalised fit are in "
                                 "per-voxel units of the largest sample, and the noise level would have to be too)");
  if (!t2_dev || !k_dev) return fail(T2FIT_E_INVALID, std::string(who) + ": t2_dev / k_dev is NULL");
  if (n_vox < 1 || n_vox >= (1LL << 32)) return fail(T2FIT_E_INVALID, std::string(who) + ": n_vox must be in 1..2^32-1");
  if (noise_kind != T2FIT_BOOT_NOISE_RICIAN && noise_kind != T2FIT_BOOT_NOISE_GAUSSIAN)
    return fail(T2FIT_E_INVALID, std::string(who) + ": unknown noise_kind");
  if (!noise_map_dev && !(noise_scalar >= 0.0 && noise_scalar <= 3.0e38))
    return fail(T2FIT_E_INVALID, std::string(who) + ": noise_scalar must be finite and >= 0 (or give noise_map_dev)");
  return T2FIT_OK;
}

int synth_launch(const t2fit_config* cfg, const float* t2_dev, const float* k_dev, double noise_scalar,
                 const float* noise_map_dev, const uint8_t* mask_dev, int64_t n_vox, int64_t voxel_offset, uint64_t seed,
                 int replica, int noise_kind, float* out, hipStream_t st) {
  SynthArgs a{};
  a.t2 = t2_dev; a.k = k_dev; a.noise_map = noise_map_dev; a.mask = mask_dev; a.out = out;
  a.n_vox = n_vox;
  a.voxel_offset = (uint64_t)voxel_offset;
  a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32); a.replica = (uint32_t)replica;
  a.n_te = cfg->n_te;
  a.noise_scalar = (float)noise_scalar;
  for (int j = 0; j < cfg->n_te; ++j) a.te[j] = (float)cfg->te_ms[j];
  const bool vec = n_vox % 4 == 0 && aligned16(t2_dev) && aligned16(k_dev) && aligned16(out) &&
                   (!noise_map_dev || aligned16(noise_map_dev)) && (reinterpret_cast<uintptr_t>(mask_dev) & 3u) == 0;
  const bool rician = noise_kind == T2FIT_BOOT_NOISE_RICIAN;
  const int64_t lanes = vec ? n_vox / 4 : n_vox;
  const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock));
  if (vec && rician) hipLaunchKernelGGL((boot_synth_kernel<4, true>), grid, dim3(kBlock), 0, st, a);
  else if (vec) hipLaunchKernelGGL((boot_synth_kernel<4, false>), grid, dim3(kBlock), 0, st, a);
  else if (rician) hipLaunchKernelGGL((boot_synth_kernel<1, true>), grid, dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL((boot_synth_kernel<1, false>), grid, dim3(kBlock), 0, st, a);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

}  // namespace

extern "C" {

int t2fit_boot_background_dev(const float* echoes_dev, int layout, const uint8_t* mask_dev, int n_te, int64_t n_vox,
                              double* sigma_out, int64_t* count_out, void* stream) {
  if (!echoes_dev || !mask_dev || !sigma_out || !count_out)
    return fail(T2FIT_E_INVALID, "t2fit_boot_background_dev: echoes_dev / mask_dev / sigma_out / count_out is NULL");
  if (layout != T2FIT_LAYOUT_TE_MAJOR && layout != T2FIT_LAYOUT_VOXEL_MAJOR)
    return fail(T2FIT_E_INVALID, "t2fit_boot_background_dev: unknown layout");
  if (n_te < 1 || n_te > T2FIT_MAX_TE) return fail(T2FIT_E_INVALID, "t2fit_boot_background_dev: n_te outside 1..32");
  if (n_vox < 1 || n_vox >= (1LL << 32)) return fail(T2FIT_E_INVALID, "t2fit_boot_background_dev: n_vox must be in 1..2^32-1");
  hipStream_t st = (hipStream_t)stream;
  BootWorkspace ws;
  char* base = nullptr;
  const size_t part = (size_t)kBgBlocks * 8;
  T2_HIP(ws.alloc((void**)&base, 2 * part + 16));
  double* part_sum = reinterpret_cast<double*>(base);
  long long* part_cnt = reinterpret_cast<long long*>(base + part);
  double* out_sum = reinterpret_cast<double*>(base + 2 * part);
  long long* out_cnt = reinterpret_cast<long long*>(base + 2 * part + 8);
  hipLaunchKernelGGL(boot_background_kernel, dim3(kBgBlocks), dim3(kBlock), 0, st, echoes_dev, layout, mask_dev, n_te, n_vox,
                     part_sum, part_cnt);
  hipLaunchKernelGGL(boot_background_final_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)part_sum,
                     (const long long*)part_cnt, out_sum, out_cnt);
  T2_HIP(hipGetLastError());
  struct { double sum; long long cnt; } h{0.0, 0};
  T2_HIP(hipMemcpyAsync(&h, out_sum, 16, hipMemcpyDeviceToHost, st));
  T2_HIP(hipStreamSynchronize(st));
  if (h.cnt == 0)
    return fail(T2FIT_E_INVALID, "t2fit_boot_background_dev: the mask covers every voxel: there is no background to "
                                 "measure the noise level on (give the level instead)");
  *sigma_out = std::sqrt(h.sum / (2.0 * (double)h.cnt));
  *count_out = (int64_t)h.cnt;
  return T2FIT_OK;
}

int t2fit_boot_synth_dev(const t2fit_config* cfg, const float* t2_dev, const float* k_dev, double noise_scalar,
                         const float* noise_map_dev, const uint8_t* mask_dev, int64_t n_vox, int64_t voxel_offset,
                         uint64_t seed, int replica, int noise_kind, float* echoes_out_dev, void* stream) {
  const int rc = synth_check("t2fit_boot_synth_dev", cfg, t2_dev, k_dev, noise_scalar, noise_map_dev, n_vox, noise_kind);
  if (rc != T2FIT_OK) return rc;
  if (!echoes_out_dev) return fail(T2FIT_E_INVALID, "t2fit_boot_synth_dev: echoes_out_dev is NULL");
  if (replica < 0) return fail(T2FIT_E_INVALID, "t2fit_boot_synth_dev: replica is negative");
  if (voxel_offset < 0) return fail(T2FIT_E_INVALID, "t2fit_boot_synth_dev: voxel_offset is negative");
  return synth_launch(cfg, t2_dev, k_dev, noise_scalar, noise_map_dev, mask_dev, n_vox, voxel_offset, seed, replica,
                      noise_kind, echoes_out_dev, (hipStream_t)stream);
}

int t2fit_bootstrap_dev(t2fit_context* ctx, const t2fit_config* cfg, const float* t2_dev, const float* k_dev,
                        const float* sigma_dev, double noise_scalar, const float* noise_map_dev, int noise_kind,
                        const uint8_t* mask_dev, int64_t n_vox, int n_replicas, uint64_t seed, double alpha,
                        int which_params, const t2fit_boot_maps* out, int flags, void* stream) {
  const char* who = "t2fit_bootstrap_dev";
  // ---- arguments, before any device work ----
  int rc = synth_check(who, cfg, t2_dev, k_dev, noise_scalar, noise_map_dev, n_vox, noise_kind);
  if (rc != T2FIT_OK) return rc;
  if (!mask_dev) return fail(T2FIT_E_INVALID, "t2fit_bootstrap_dev: mask_dev is NULL (pass a mask of ones to take every voxel)");
  if (!out) return fail(T2FIT_E_INVALID, "t2fit_bootstrap_dev: out is NULL");
  if (which_params < 1 || which_params > 7) return fail(T2FIT_E_INVALID, "t2fit_bootstrap_dev: which_params must be a non-empty set of T2FIT_BOOT_PARAM_*");
  if ((which_params & T2FIT_BOOT_PARAM_SIGMA) && cfg->model == T2FIT_MODEL_GAUSSIAN)
    return fail(T2FIT_E_INVALID, "t2fit_bootstrap_dev: T2FIT_BOOT_PARAM_SIGMA asked of the 2-parameter gaussian model, which has no sigma");
  if ((which_params & T2FIT_BOOT_PARAM_SIGMA) && !sigma_dev)
    return fail(T2FIT_E_INVALID, "t2fit_bootstrap_dev: sigma_dev is NULL but T2FIT_BOOT_PARAM_SIGMA is requested");
  if (flags != 0) return fail(T2FIT_E_INVALID, "t2fit_bootstrap_dev: flags is reserved and must be 0");
  if (n_replicas < 1) return fail(T2FIT_E_INVALID, "t2fit_bootstrap_dev: n_replicas must be at least 1");
  bool interval = false;
  int n_par = 0;
  for (int p = 0; p < 3; ++p)
    if (which_params & (1 << p)) {
      ++n_par;
      interval = interval || out->ci_lo[p] || out->ci_hi[p];
    }
  if (interval) {
    if (n_replicas < 2) return fail(T2FIT_E_INVALID, "t2fit_bootstrap_dev: a percentile interval needs at least 2 replicas");
    if (n_replicas > kMaxIntervalReplicas)
      return fail(T2FIT_E_INVALID, "t2fit_bootstrap_dev: a percentile interval is computed for at most 512 replicas (their "
                                   "values are staged on chip); with more, ask for the moments only (ci_lo = ci_hi = NULL)");
    if (!(alpha > 0.0 && alpha < 1.0)) return fail(T2FIT_E_INVALID, "t2fit_bootstrap_dev: alpha must lie in (0, 1)");
  }
  // ---- workspace, computed before any device work.  The mask has not been read yet, so the per-masked-voxel part is
  // bounded by n_masked <= n_vox; it is allocated for the actual count. ----
  const double n = (double)n_vox;
  const double fixed_b = 2.0 * cfg->n_te * 4.0 * n  // two replica blocks
                         + 17.0 * n                // the replica's t2 / k / sigma / res / status maps
                         + 9.0 * n + 8.0;          // mask indices, union mask, count
  const double per_masked_b = n_par * 24.0 + 4.0 + (interval ? n_par * 4.0 * (double)n_replicas : 0.0);
  const double bound_b = fixed_b + per_masked_b * n;
  // T2FIT_BOOT_MEM_LIMIT (bytes): the most this call may take, whatever is free (a share of a device that others use
  // too); a call beyond it is refused here, before the HIP runtime is touched
  double limit_b = -1.0;
  if (const char* e = std::getenv("T2FIT_BOOT_MEM_LIMIT")) limit_b = std::strtod(e, nullptr);
  auto refuse = [&](double avail_b, const char* what) {
    return fail(T2FIT_E_HIP, std::string(who) + ": the workspace needs up to " + gib(bound_b) + " (" + gib(fixed_b) +
                             " for two replica blocks and one set of maps, " + gib(per_masked_b * n) + " for the sums" +
                             (interval ? " and the (R, n_masked) values of the interval" : "") + " if every voxel is masked) but " +
                             gib(avail_b) + what + "; use fewer replicas, moments only, or slabs");
  };
  if (limit_b >= 0.0 && bound_b > limit_b) return refuse(limit_b, " are allowed by T2FIT_BOOT_MEM_LIMIT");
  Phases ph;
  int device = 0;
  if (ctx) T2_HIP(hipSetDevice(ctx->device));
  T2_HIP(hipGetDevice(&device));
  size_t free_b = 0, total_b = 0;
  T2_HIP(hipMemGetInfo(&free_b, &total_b));
  if (bound_b > (double)free_b) return refuse((double)free_b, " of device memory are free");
  ph.mark("device, hipMemGetInfo");

  std::unique_lock<std::mutex> busy;
  if (ctx) busy = std::unique_lock<std::mutex>(ctx->busy);
  BootWorkspace ws;
  hipStream_t caller = (hipStream_t)stream;
  if (ctx) {
    ws.streams[0] = ctx->s_in;
    ws.streams[1] = ctx->s_fit;
  } else {
    ws.own_streams = true;
    T2_HIP(hipStreamCreateWithFlags(&ws.streams[0], hipStreamNonBlocking));
    T2_HIP(hipStreamCreateWithFlags(&ws.streams[1], hipStreamNonBlocking));
  }
  hipStream_t s_fit = ws.streams[1];
  // T2FIT_BOOT_STREAMS=1: synthesis and fit on one stream (for measurements: the results are the same bits)
  const char* streams_env = std::getenv("T2FIT_BOOT_STREAMS");
  hipStream_t s_syn = (streams_env && std::atoi(streams_env) == 1) ? s_fit : ws.streams[0];

  // ---- mask indices (np.where order) and their count ----
  int64_t* idx = nullptr;
  uint8_t* mask1 = nullptr;
  int64_t* count_d = nullptr;
  T2_HIP(ws.alloc((void**)&idx, (size_t)n_vox * 8));
  T2_HIP(ws.alloc((void**)&mask1, (size_t)n_vox));
  T2_HIP(ws.alloc((void**)&count_d, 8));
  hipEvent_t ev_in = nullptr;
  T2_HIP(ws.event(&ev_in));
  T2_HIP(hipEventRecord(ev_in, caller));  // the caller's maps are ready once its stream gets here
  T2_HIP(hipStreamWaitEvent(s_fit, ev_in, 0));
  if (s_syn != s_fit) T2_HIP(hipStreamWaitEvent(s_syn, ev_in, 0));
  rc = t2fit_union_mask_dev(mask_dev, 1, n_vox, mask1, idx, count_d, s_fit);
  if (rc != T2FIT_OK) return rc;
  int64_t n_masked = 0;
  T2_HIP(hipMemcpyAsync(&n_masked, count_d, 8, hipMemcpyDeviceToHost, s_fit));
  T2_HIP(hipStreamSynchronize(s_fit));
  ph.mark("streams, mask indices");

  // dense outputs: zeros outside the mask like every other map
  float* const* groups[5] = {out->mean, out->bias, out->std, out->ci_lo, out->ci_hi};
  for (int p = 0; p < 3; ++p)
    if (which_params & (1 << p))
      for (auto g : groups)
        if (g[p]) T2_HIP(hipMemsetAsync(g[p], 0, (size_t)n_vox * 4, s_fit));
  if (out->n_ok) T2_HIP(hipMemsetAsync(out->n_ok, 0, (size_t)n_vox * 4, s_fit));
  if (n_masked > 0) {
    // ---- buffers ----
    float* block[2] = {nullptr, nullptr};
    float* rep[4] = {nullptr, nullptr, nullptr, nullptr};  // t2, k, sigma, res
    uint8_t* rep_status = nullptr;
    for (auto& b : block) T2_HIP(ws.alloc((void**)&b, (size_t)cfg->n_te * (size_t)n_vox * 4));
    for (auto& r : rep) T2_HIP(ws.alloc((void**)&r, (size_t)n_vox * 4));
    T2_HIP(ws.alloc((void**)&rep_status, (size_t)n_vox));
    const size_t nm = (size_t)n_masked;
    double *sum[3] = {nullptr, nullptr, nullptr}, *sumsq[3] = {nullptr, nullptr, nullptr};
    float *vmin[3] = {nullptr, nullptr, nullptr}, *vmax[3] = {nullptr, nullptr, nullptr};
    float* vals[3] = {nullptr, nullptr, nullptr};
    int32_t* n_ok = nullptr;
    const float* centre[3] = {t2_dev, k_dev, sigma_dev};
    T2_HIP(ws.alloc((void**)&n_ok, nm * 4));
    T2_HIP(hipMemsetAsync(n_ok, 0, nm * 4, s_fit));
    for (int p = 0; p < 3; ++p) {
      if (!(which_params & (1 << p))) continue;
      T2_HIP(ws.alloc((void**)&sum[p], nm * 8));
      T2_HIP(ws.alloc((void**)&sumsq[p], nm * 8));
      T2_HIP(ws.alloc((void**)&vmin[p], nm * 4));
      T2_HIP(ws.alloc((void**)&vmax[p], nm * 4));
      T2_HIP(hipMemsetAsync(sum[p], 0, nm * 8, s_fit));
      T2_HIP(hipMemsetAsync(sumsq[p], 0, nm * 8, s_fit));
      if (interval) T2_HIP(ws.alloc((void**)&vals[p], (size_t)n_replicas * nm * 4));
    }
    ph.mark("hipMalloc of the workspace");
#ifdef T2FIT_BOOT_PHASES
    T2_HIP(hipStreamSynchronize(s_fit));
    ph.mark("memsets done");
#endif
    hipEvent_t ev_syn[2], ev_fit[2];
    for (int b = 0; b < 2; ++b) {
      T2_HIP(ws.event(&ev_syn[b]));
      T2_HIP(ws.event(&ev_fit[b]));
    }
    t2fit_maps rm{};
    rm.t2 = rep[0]; rm.k = rep[1]; rm.sigma = rep[2]; rm.res = rep[3]; rm.status = rep_status;
    AccumArgs acc{};
    acc.idx = idx; acc.n_masked = n_masked; acc.status = rep_status;
    acc.n_ok = n_ok;
    for (int p = 0; p < 3; ++p) {
      acc.sum[p] = sum[p]; acc.sumsq[p] = sumsq[p]; acc.vmin[p] = vmin[p]; acc.vmax[p] = vmax[p];
      acc.rep[p] = (which_params & (1 << p)) ? rep[p] : nullptr;
      acc.centre[p] = centre[p];
      acc.vals[p] = vals[p];
    }
    const dim3 acc_grid((unsigned)((n_masked + kBlock - 1) / kBlock));
    // ---- the loop: replica r + 1 is synthesised on one stream while replica r is fitted on the other ----
    auto synth = [&](int r) -> int {
      const int b = r & 1;
      if (r >= 2 && s_syn != s_fit) T2_HIP(hipStreamWaitEvent(s_syn, ev_fit[b], 0));  // block b was read by the fit of r - 2
      const int src = synth_launch(cfg, t2_dev, k_dev, noise_scalar, noise_map_dev, mask1, n_vox, 0, seed, r, noise_kind,
                                   block[b], s_syn);
      if (src != T2FIT_OK) return src;
      if (s_syn != s_fit) T2_HIP(hipEventRecord(ev_syn[b], s_syn));
      return T2FIT_OK;
    };
    if ((rc = synth(0)) != T2FIT_OK) return rc;
    for (int r = 0; r < n_replicas; ++r) {
      const int b = r & 1;
      if (r + 1 < n_replicas && (rc = synth(r + 1)) != T2FIT_OK) return rc;
      if (s_syn != s_fit) T2_HIP(hipStreamWaitEvent(s_fit, ev_syn[b], 0));
      rc = t2fit_volume_dev(cfg, block[b], T2FIT_LAYOUT_TE_MAJOR, mask1, n_vox, &rm, s_fit);
      if (rc != T2FIT_OK) return rc;
      acc.replica = r;
      hipLaunchKernelGGL(boot_accum_kernel, acc_grid, dim3(kBlock), 0, s_fit, acc);
      T2_HIP(hipGetLastError());
      if (s_syn != s_fit) T2_HIP(hipEventRecord(ev_fit[b], s_fit));
#ifdef T2FIT_BOOT_PHASES
      if (r < 3 || r + 1 == n_replicas) {
        T2_HIP(hipStreamSynchronize(s_fit));
        ph.mark(r == 0 ? "replica 0 done" : r == 1 ? "replica 1 done" : r == 2 ? "replica 2 done" : "replicas 3.. done");
      }
#endif
    }
    // ---- finalisation, one launch per parameter ----
    const size_t lds = interval ? (size_t)n_replicas * 256 : 0;
    if (lds > 65536)
      T2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&boot_final_kernel<true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 fin_grid((unsigned)((n_masked + 63) / 64));
    bool first = true;
    for (int p = 0; p < 3; ++p) {
      if (!(which_params & (1 << p))) continue;
      FinalArgs f{};
      f.idx = idx; f.n_masked = n_masked; f.centre = centre[p];
      f.sum = sum[p]; f.sumsq = sumsq[p]; f.vmin = vmin[p]; f.vmax = vmax[p];
      f.n_ok = n_ok; f.vals = vals[p]; f.n_replicas = n_replicas;
      f.q_lo = alpha / 2.0; f.q_hi = 1.0 - alpha / 2.0;
      f.mean = out->mean[p]; f.bias = out->bias[p]; f.std = out->std[p]; f.ci_lo = out->ci_lo[p]; f.ci_hi = out->ci_hi[p];
      f.n_ok_out = first ? out->n_ok : nullptr;
      first = false;
      if (interval) hipLaunchKernelGGL(boot_final_kernel<true>, fin_grid, dim3(64), lds, s_fit, f);
      else hipLaunchKernelGGL(boot_final_kernel<false>, fin_grid, dim3(64), 0, s_fit, f);
      T2_HIP(hipGetLastError());
    }
  }
  // the workspace is freed on return: wait for everything that uses it (the maps are complete on return)
  if (s_syn != s_fit) T2_HIP(hipStreamSynchronize(s_syn));
  T2_HIP(hipStreamSynchronize(s_fit));
  ph.mark("finalisation done");
  return T2FIT_OK;
}

}  // extern "C"

// t2fit_kernels.hip -- gfx950 (MI355X, CDNA4) kernels of the per-voxel T2 fit, their launch dispatch and the device
// entry points of include/t2fit.h (t2fit_volume_dev, t2fit_residuals_dev, timing, reserve).  The host seam is
// t2fit_host.hip, which reaches launch_fit through t2fit_launch.h; the mask union and the per-label statistics are
// t2fit_masks.hip.  Built with:  hipcc -O3 --offload-arch=gfx950 -shared -fPIC
//
// Mapping: one lane fits one voxel at a time, 256-thread workgroups (4 wave64).  The fit kernels
// are persistent: waves pull chunks of consecutive voxels from a global atomic counter and every
// lane that finishes a voxel takes the next one (fit_persistent_kernel below); the streaming
// kernels (closed-form log-linear fit, residual map) use grid = ceil(N / tile) >> 256 CUs.
// HBM layout: echoes (nTE, N) float32, TE-major; every sample of a fitted voxel is read once and
// parked in LDS ([nTE][257] floats per workgroup, one column per lane, padded so the voxel-major
// staging transpose is conflict-free).  The solver re-reads its column from LDS on every objective
// evaluation instead of holding nTE samples in VGPRs (nTE is a run-time value).  Each map is
// written once.  Algorithmic HBM traffic per voxel: 4*nTE (samples) + 1 (mask) + 16 (t2, k, sigma,
// res) = 49 B at 8 TE.  The fit itself is ALU work (exp/sqrt/div/fma, fp64 or fp32); no MFMA:
// nothing here is a contraction.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <string>

#include "t2fit_config.h"
#include "t2fit_diag.h"
#include "t2fit_dispatch.h"
#include "t2fit_error.h"
#include "t2fit_launch.h"
#include "t2fit_support.h"

using namespace t2fit;

namespace {

constexpr int kLdsStride = kBlock + 1;
#ifndef T2_SAMPLE_LOAD
#define T2_SAMPLE_LOAD(p) (*(p))  // A/B: -DT2_SAMPLE_LOAD(p)=__builtin_nontemporal_load(p), profiles/r02_exp42_nt_loads.txt
#endif
#ifndef T2_WAVE_HINT
#define T2_WAVE_HINT 2
#endif
constexpr int kWaveHint = T2_WAVE_HINT;  // occupancy the register allocator / scheduler is told for the one-wave workgroups

// Process-wide tuning: the T2FIT_* switches of the fit, read from the environment once (by the first call that asks, under
// the function-local static's lock) and only read afterwards.  None of it can change a result: the maps do not depend on
// how many workgroups fit a volume.  (Read per call instead, because tests change them between calls: T2FIT_HOST_SLABS in
// t2fit_host.hip, T2FIT_BOOT_MEM_LIMIT and T2FIT_BOOT_STREAMS in t2fit_boot.hip; T2FIT_COPY_THREADS per t2fit_create.)
struct Tuning {
  bool use_persistent = true;    // T2FIT_ONE_SHOT=1: the LM solver runs the one-voxel-per-lane kernel
  int persistent_blocks = 2048;  // T2FIT_PERSISTENT_BLOCKS: grid of the persistent kernel
  int refill_min = 0;            // T2FIT_REFILL_MIN: > 0 overrides the per-solver refill batch
  bool nte_special = true;       // T2FIT_NTE_SPECIAL=0: always the generic-echo-count lane (A/B switch)
  // T2FIT_TAKE: 64-voxel chunks per counter increment in the one-wave-workgroup kernels (0: the default, 2).  Measured
  // (256^3 x 8 TE and its 1/2, 1/4, 1/8 shares, profiles/r02_exp58_mid_size.txt): 2 is best throughout -- 4 lengthens the
  // drain of a launch (2.55 against 2.32 ms on a 1/8 share), 1 costs a little on whole volumes (13.73 against 13.55 ms)
  int take = 0;
  int64_t small_volume = 1 << 20;  // T2FIT_SMALL_VOLUME (A/B runs): at or below, the generic small-chunk kernels
  int wave_wg = 1;       // T2FIT_WAVE_WG=0: 256-lane workgroups for the large-volume L-BFGS-B kernels, not one-wave ones
  int waves_per_cu = 0;  // T2FIT_WAVES_PER_CU: cap of the one-wave workgroups' occupancy (A/B runs)
};
// The reserve is no part of the record: it can be set at any time from any thread (t2fit_set_reserve_cus) while other
// threads launch.
std::atomic<bool> g_reserve_set{false};  // t2fit_set_reserve_cus() was called: it wins over the environment
std::atomic<int> g_reserve_cus{0};       // T2FIT_RESERVE_CUS: CUs' worth of workgroups the L-BFGS-B kernel is launched short

const Tuning& tuning() {
  static const Tuning tuned = [] {
    Tuning t;
    if (const char* e = std::getenv("T2FIT_ONE_SHOT")) t.use_persistent = std::atoi(e) == 0;
    if (const char* e = std::getenv("T2FIT_PERSISTENT_BLOCKS")) t.persistent_blocks = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("T2FIT_REFILL_MIN")) t.refill_min = std::min(64, std::max(1, std::atoi(e)));
    if (const char* e = std::getenv("T2FIT_RESERVE_CUS"); e && !g_reserve_set.load()) g_reserve_cus.store(std::max(0, std::atoi(e)));
    if (const char* e = std::getenv("T2FIT_NTE_SPECIAL")) t.nte_special = std::atoi(e) != 0;
    if (const char* e = std::getenv("T2FIT_TAKE")) t.take = std::max(0, std::min(64, std::atoi(e)));
    if (const char* e = std::getenv("T2FIT_SMALL_VOLUME")) t.small_volume = std::max<int64_t>(0, std::atoll(e));
    if (const char* e = std::getenv("T2FIT_WAVE_WG")) t.wave_wg = std::max(0, std::atoi(e));
    if (const char* e = std::getenv("T2FIT_WAVES_PER_CU")) t.waves_per_cu = std::max(0, std::atoi(e));
    return t;
  }();
  return tuned;
}

thread_local bool g_timing = false;
// start / stop events of the last kEvRing timed launches (a caller that pipelines launches over several streams reads a
// launch's time a few launches later, when it is long done, instead of stalling on the one just queued)
constexpr int kEvRing = 16;
thread_local hipEvent_t g_ev0[kEvRing] = {}, g_ev1[kEvRing] = {}, g_ev2[kEvRing] = {};  // start, end of the fit kernel, end of the epilogue pass
thread_local long g_ev_count = 0;   // timed launches so far
thread_local int g_ev_slot = 0;     // ring slot of the launch being queued

// milliseconds between two events of the timed launch `launches_ago` launches back, or -1
double event_ms(int launches_ago, const hipEvent_t* from, const hipEvent_t* to) {
  if (launches_ago < 0 || launches_ago >= kEvRing || launches_ago >= g_ev_count) return -1.0;
  const int slot = (int)((g_ev_count - 1 - launches_ago) % kEvRing);
  if (hipEventSynchronize(to[slot]) != hipSuccess) return -1.0;
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, from[slot], to[slot]) != hipSuccess) return -1.0;
  return (double)ms;
}

struct DevMaps {
  float *t2, *k, *sigma, *res, *r2, *fun, *se;
  int32_t* nit;
  uint8_t* status;
  double* xd;    // optional: float64 parameters, 3 per voxel (voxel seam)
  double* fund;  // optional: float64 objective value
  double* trace = nullptr;         // trace kernels only: [n_vox][trace_cap][4] doubles (k, T2, sigma, f)
  int32_t* trace_len = nullptr;    //                     iterations recorded per voxel
  int trace_cap = 0;
};

// Stage this workgroup's samples into LDS.  TE-major: each lane copies its own column (coalesced
// per plane, no exchange needed).  Voxel-major: the (256, nTE) tile is contiguous in HBM, so it is
// read linearly by the whole workgroup and transposed on the way into LDS.
__device__ __forceinline__ void stage_echoes(float* lds, const float* __restrict__ echoes, int layout,
                                             int n_te, int64_t n_vox, int64_t base, bool load_own) {
  const int lane = threadIdx.x;
  if (layout == T2FIT_LAYOUT_TE_MAJOR) {
    if (load_own) {
      const float* src = echoes + base + lane;
      for (int i = 0; i < n_te; ++i) lds[i * kLdsStride + lane] = src[(int64_t)i * n_vox];
    }
  } else {
    const int64_t rows = n_vox - base < kBlock ? n_vox - base : kBlock;
    const int total = (int)rows * n_te;
    const float* src = echoes + base * n_te;
    for (int j = lane; j < total; j += kBlock) {
      const int v = j / n_te;
      const int i = j - v * n_te;
      lds[i * kLdsStride + v] = src[j];
    }
    __syncthreads();
  }
}

// kExtras = false: the caller asked for the reference's four maps only; the optional outputs are not even tested
// for (their pointers would otherwise live in scalar registers across the whole persistent loop)
// kEpilogueFollows: the persistent fits are followed by residuals_kernel, which writes res / r2 / se of every voxel
// (zeros outside the mask): storing those zeros here as well would write the same lines twice
template <bool kExtras = true, bool kEpilogueFollows = false>
__device__ __forceinline__ void store_masked(const DevMaps& m, int64_t v) {
  // zeros outside the mask (run_t2mapping.py:415-418)
  m.t2[v] = 0.0f; m.k[v] = 0.0f; m.sigma[v] = 0.0f;
  if constexpr (!kEpilogueFollows) m.res[v] = 0.0f;
  if constexpr (!kExtras) return;
  if constexpr (!kEpilogueFollows) {
    if (m.r2) m.r2[v] = 0.0f;
    if (m.se) m.se[v] = 0.0f;
  }
  if (m.fun) m.fun[v] = 0.0f;
  if (m.nit) m.nit[v] = 0;
  if (m.status) m.status[v] = T2FIT_ST_MASKED;
  if (m.xd) { m.xd[3 * v] = 0.0; m.xd[3 * v + 1] = 0.0; m.xd[3 * v + 2] = 0.0; }
  if (m.fund) m.fund[v] = 0.0;
}

__device__ __forceinline__ void store_result(const DevMaps& m, int64_t v, const LaneOutputs& o, const LaneResult& r) {
  m.t2[v] = o.t2; m.k[v] = o.k; m.sigma[v] = o.sigma; m.res[v] = o.res;
  if (m.r2) m.r2[v] = o.r2;
  if (m.se) m.se[v] = o.se;
  if (m.fun) m.fun[v] = o.fun;
  if (m.nit) m.nit[v] = o.nit;
  if (m.status) m.status[v] = o.status;
  if (m.xd) { m.xd[3 * v] = r.x[0]; m.xd[3 * v + 1] = r.x[1]; m.xd[3 * v + 2] = r.x[2]; }
  if (m.fund) m.fund[v] = r.fun;
}

// parameters and per-voxel extras only; res / r2 come from the epilogue pass
template <bool kExtras = true>
__device__ __forceinline__ void store_fit(const DevMaps& m, int64_t v, const LaneResult& r) {
  m.k[v] = (float)r.x[0]; m.t2[v] = (float)r.x[1]; m.sigma[v] = (float)r.x[2];
  if constexpr (!kExtras) return;
  if (m.fun) m.fun[v] = (float)r.fun;
  if (m.nit) m.nit[v] = r.nit;
  if (m.status) m.status[v] = r.status;
  if (m.xd) { m.xd[3 * v] = r.x[0]; m.xd[3 * v + 1] = r.x[1]; m.xd[3 * v + 2] = r.x[2]; }
  if (m.fund) m.fund[v] = r.fun;
}

// One lane per voxel, one voxel per lane: used for the LM solver and as the fallback of the
// persistent kernel below.
template <int SOLVER, int PREC, int MODEL>
__global__ __launch_bounds__(kBlock) void fit_volume_kernel(const LaneParams P, const float* __restrict__ echoes,
                                                            int layout, const uint8_t* __restrict__ mask,
                                                            int64_t n_vox, DevMaps m) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kBlock;
  const int64_t v = base + lane;
  const bool in_range = v < n_vox;
  const bool active = in_range && (mask == nullptr || mask[v] != 0);
  stage_echoes(lds, echoes, layout, P.n_te, n_vox, base, active);
  if (!in_range) return;
  if (!active) {
    store_masked(m, v);
    return;
  }
  bool finite;
  float y0_raw;
  const ObjCtx c = prepare_samples(P, lds + lane, kLdsStride, finite, y0_raw);
  LaneResult r;
  fit_lane_t<SOLVER, PREC, MODEL>(P, c, finite, y0_raw, r);
  LaneOutputs o;
  lane_epilogue(c, r, o, m.r2 != nullptr, m.se != nullptr);
  store_result(m, v, o, r);
}

// Closed-form log-linear fit (T2FIT_SOLVER_LOGLIN), TE-major stacks: one streaming pass, four
// consecutive voxels per lane so that every echo plane is read with 16-byte loads and every map is
// written with 16-byte stores (1 KiB per wave instruction).  Fit, bounds, float32 casts, residual map
// and the optional extras all happen in this pass: algorithmic HBM bytes = 4*nTE + 1 + 16 per voxel,
// and nothing but HBM bounds it.  A lane whose four voxels are all outside the mask issues no echo
// loads.  Samples are parked in LDS as [nTE][4][256] (lane-contiguous: conflict-free) so that the lane
// math shared with the other solvers can address them by a run-time echo index.
constexpr int kLoglinVec = 4;
constexpr int kLoglinTile = kBlock * kLoglinVec;

// kExtras = false is the four-map form (no r2 / se / fun / nit / status / float64 outputs): its code holds none
// of those evaluations, which keeps the four unrolled voxel bodies inside the instruction cache.
template <bool kExtras>
__global__ __launch_bounds__(kBlock) void loglin_volume_kernel(const LaneParams P, const float* __restrict__ echoes,
                                                               const uint8_t* __restrict__ mask, int64_t n_vox,
                                                               DevMaps m) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x;
  const int64_t v0 = (int64_t)blockIdx.x * kLoglinTile + (int64_t)lane * kLoglinVec;
  if (v0 >= n_vox) return;  // n_vox is a multiple of 4 on this path: a lane is all in or all out
  const int n_te = P.n_te;
  bool act[kLoglinVec] = {true, true, true, true};
  if (mask) {
    const uchar4 mk = *reinterpret_cast<const uchar4*>(mask + v0);
    act[0] = mk.x != 0; act[1] = mk.y != 0; act[2] = mk.z != 0; act[3] = mk.w != 0;
  }
  const bool any = act[0] || act[1] || act[2] || act[3];
  // finite check, first sample and row maximum are taken while the samples are still in registers
  bool fin[kLoglinVec] = {true, true, true, true};
  float ymax[kLoglinVec] = {0.0f, 0.0f, 0.0f, 0.0f}, y0[kLoglinVec] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (any) {
    const float* src = echoes + v0;
    for (int i0 = 0; i0 < n_te; i0 += 8) {  // up to eight 16-byte loads in flight per lane
      float4 tmp[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (i0 + j < n_te) tmp[j] = *reinterpret_cast<const float4*>(src + (int64_t)(i0 + j) * n_vox);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (i0 + j < n_te) {
          float* dst = lds + (i0 + j) * kLoglinTile + lane;
          const float sv[kLoglinVec] = {tmp[j].x, tmp[j].y, tmp[j].z, tmp[j].w};
#pragma unroll
          for (int q = 0; q < kLoglinVec; ++q) {
            dst[q * kBlock] = sv[q];
            fin[q] = fin[q] && t2_finite(sv[q]);
            if (i0 + j == 0) { y0[q] = sv[q]; ymax[q] = sv[q]; }
            ymax[q] = sv[q] > ymax[q] ? sv[q] : ymax[q];
          }
        }
    }
  }
  float o_t2[kLoglinVec], o_k[kLoglinVec], o_res[kLoglinVec];
  const bool want_fun = kExtras && (m.fun != nullptr || m.fund != nullptr);
#pragma unroll
  for (int q = 0; q < kLoglinVec; ++q) {
    o_t2[q] = 0.0f; o_k[q] = 0.0f; o_res[q] = 0.0f;
    const int64_t v = v0 + q;
    if (!act[q]) {
      if constexpr (kExtras) {
        if (m.r2) m.r2[v] = 0.0f;
        if (m.se) m.se[v] = 0.0f;
        if (m.fun) m.fun[v] = 0.0f;
        if (m.nit) m.nit[v] = 0;
        if (m.status) m.status[v] = T2FIT_ST_MASKED;
        if (m.xd) { m.xd[3 * v] = 0.0; m.xd[3 * v + 1] = 0.0; m.xd[3 * v + 2] = 0.0; }
        if (m.fund) m.fund[v] = 0.0;
      }
      continue;
    }
    float* col = lds + q * kBlock + lane;
    bool finite = fin[q];
    if (P.norm) {  // run_t2mapping.py:237-238: float32 / float32, as prepare_samples() does it
      for (int i = 0; i < n_te; ++i) {
        const float sv = col[i * kLoglinTile] / ymax[q];
        col[i * kLoglinTile] = sv;
        finite = finite && t2_finite(sv);
      }
    }
    ObjCtx c;
    c.P = &P;
    c.y = EchoView{col, kLoglinTile};
    double lb[3], ub[3];
    const bool feasible = lane_bounds(P, y0[q], lb, ub);
    LaneResult r;
    r.nit = 0; r.nfev = 0; r.fun = NAN;
    if (!feasible) {
      r.x[0] = NAN; r.x[1] = NAN; r.x[2] = 0.0;
      r.status = T2FIT_ST_INFEASIBLE;
    } else if (!finite) {
      r.x[0] = t2_clip(P.x0[0], lb[0], ub[0]); r.x[1] = t2_clip(P.x0[1], lb[1], ub[1]); r.x[2] = 0.0;
      r.status = T2FIT_ST_NONFINITE;
    } else {
      loglin_solve(c, lb, ub, want_fun, r);
    }
    LaneOutputs o;
    lane_epilogue(c, r, o, kExtras && m.r2 != nullptr, kExtras && m.se != nullptr);
    o_t2[q] = o.t2; o_k[q] = o.k; o_res[q] = o.res;
    if constexpr (kExtras) {
      if (m.r2) m.r2[v] = o.r2;
      if (m.se) m.se[v] = o.se;
      if (m.fun) m.fun[v] = o.fun;
      if (m.nit) m.nit[v] = o.nit;
      if (m.status) m.status[v] = o.status;
      if (m.xd) { m.xd[3 * v] = r.x[0]; m.xd[3 * v + 1] = r.x[1]; m.xd[3 * v + 2] = r.x[2]; }
      if (m.fund) m.fund[v] = r.fun;
    }
  }
  *reinterpret_cast<float4*>(m.t2 + v0) = make_float4(o_t2[0], o_t2[1], o_t2[2], o_t2[3]);
  *reinterpret_cast<float4*>(m.k + v0) = make_float4(o_k[0], o_k[1], o_k[2], o_k[3]);
  *reinterpret_cast<float4*>(m.sigma + v0) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  *reinterpret_cast<float4*>(m.res + v0) = make_float4(o_res[0], o_res[1], o_res[2], o_res[3]);
}

// Persistent form of the reference-trajectory fit.  The number of objective evaluations per voxel
// varies 4..200 (line searches), so with one voxel per lane a wave waits for its slowest voxel
// (measured lane efficiency 0.53).  Here a wave keeps all 64 lanes busy instead: waves pull chunks
// of kChunk (256, or 64 for small volumes) consecutive voxels from a global atomic counter, zero-fill the masked-out ones, queue
// the active ones in LDS, and every lane that finishes a voxel pops the next one.  The loop body is
// one objective+gradient evaluation (uniform, expensive) followed by the lane's solver advance
// (divergent, cheap); the wave leaves when a __ballot shows no lane has work and the queue is dry.
constexpr int kChunkLarge = 256;  // voxels a wave takes from the global queue at a time
constexpr int kChunkSmall = 64;   // small volumes (phantoms): more, smaller chunks so that every wave gets work
constexpr int kQueueCap = 64 + kChunkLarge;

// what the persistent kernel needs to know about a resumable lane solver
template <int MODEL, int NTE = 0, int HOME = PAIRS_LDS> struct LbfgsbLane {
  using Solver = Lbfgsb<MODEL, NTE, HOME>;
  // the one-wave-workgroup kernels keep one number of each pair outside LDS (three parameters: eight waves per CU): in
  // the lane's registers where it has 20 to spare (least squares: 221 -> 241 of 256), in global memory where it has
  // not (the Rician likelihood fills all 256 as it is)
  using WaveWg = LbfgsbLane<MODEL, NTE, MODEL == T2FIT_MODEL_GAUSSIAN ? PAIRS_LDS
                                         : MODEL == T2FIT_MODEL_RICIAN ? PAIRS_GLOBAL : PAIRS_REG>;
  static constexpr bool kGlobalPart = Solver::kPairGlobal;
  static constexpr int NP = Solver::N;
  static constexpr int kNte = NTE;  // > 0: the echo count is a compile-time constant (the refill loops flatten too)
  static constexpr int kHistDoubles = Solver::M * Solver::PAIR_L;  // correction pairs, per lane, in LDS
  static constexpr int kWavesPerSimd = 1;
  // one-wave workgroups, two waves on a SIMD (256 registers): every model.  (The Rician-likelihood lane needed 370
  // registers while its evaluation was unrolled over echoes and i0e coefficients; as loops -- t2fit_lbfgsb.h eval(),
  // t2fit_lane.h t2_log_i0e4 -- it fits.)
  static constexpr bool kWaveWgOk = true;
#ifndef T2_WAVE_HINT_2PAR
#define T2_WAVE_HINT_2PAR 3
#endif
  // (two parameters: 240 B of pairs per lane let ten waves share a CU, three on two of its SIMDs: 168 registers.  In
  // round 2 the lane spilled 29-45 registers at that limit and 7.28 ms became 7.75 -- profiles/r02_exp50_2par_three_waves.txt;
  // since the main loop has one way into the round the lane needs 155-168 and nothing spills: 6.37 -> 5.96 ms at
  // 256 x 256 x 180 x 6 TE, profiles/r03_exp23_2par_ten_waves.txt.  -DT2_WAVE_HINT_2PAR=2: eight waves.)
  static constexpr int kWaveWgHint = MODEL == T2FIT_MODEL_GAUSSIAN ? T2_WAVE_HINT_2PAR : kWaveHint;
  // lanes that must be idle before a wave refills.  Measured on MI355X at eight waves per CU (profiles/
  // r03_exp6_refill_take.txt), 256^3 x 8 TE: 1 -> 12.48 ms, 4 -> 12.13, 8 -> 12.03, 12 -> 12.20, 16 -> 12.42; the Rician
  // likelihood, whose evaluation is four times as long (an idle lane costs more): 4 -> 19.77, 8 -> 20.01, 16 -> 20.76
  static constexpr int kRefillMin = MODEL == T2FIT_MODEL_RICIAN ? 4 : 8;
  static constexpr bool kSplit = true;   // advance() = digest() + begin_pass(): the kernel calls the two halves itself
  __device__ static void init(Solver& s, const ObjCtx&, const double* x0, const double* lb, const double* ub,
                              double* hist, int hstride, double* ghist) { s.init(x0, lb, ub, hist, hstride, ghist, 64); }
  __device__ static void result(const Solver& s, const ObjCtx&, LaneResult& r) { s.result(r); }
  template <int J> __device__ static void take_sample(Solver& s, float y) {
    if constexpr (NTE > 0 && J < NTE) s.ys[J] = y;
  }
};
template <typename T, int NPAR, int NTE = 0> struct LmLaneAdaptor {
  using Solver = LmLane<T, NPAR, NTE>;
  using WaveWg = LmLaneAdaptor<T, NPAR, NTE>;
  static constexpr bool kGlobalPart = false;
  static constexpr int NP = NPAR;
  static constexpr int kNte = NTE;
  static constexpr int kHistDoubles = 0;
  static constexpr bool kWaveWgOk = false;
  static constexpr int kWaveWgHint = 1;
  // float32: four waves per SIMD (128 registers); float64: what the 229 registers of the lane allow (two, LDS permitting)
  static constexpr int kWavesPerSimd = sizeof(T) == 4 ? 4 : 1;
  static constexpr int kRefillMin = 24;  // measured (f32, 3 parameters, MI355X): 8 -> 1.62 ms, 16 -> 1.42 ms, 24 -> 1.35 ms, 32 -> 1.35 ms
  static constexpr bool kSplit = false;
  __device__ static void init(Solver& s, const ObjCtx& c, const double* x0, const double* lb, const double* ub,
                              double*, int, double*) { s.init(c, x0, lb, ub); }
  __device__ static void result(const Solver& s, const ObjCtx& c, LaneResult& r) { s.result(c, r); }
  template <int J> __device__ static void take_sample(Solver&, float) {}
};

// `P` as it lies in a kernel's argument segment (constant address space: read by scalar loads)
using KernargParams = const __attribute__((address_space(4))) LaneParams*;

template <class A, int kChunk, bool kTrace, bool kExtras, int kWg = kBlock, bool kRegs = false>
__device__ __forceinline__ void persistent_fit(const LaneParams& P, const float* __restrict__ echoes, int layout,
                                               const uint8_t* __restrict__ mask, int64_t n_vox, const DevMaps& m,
                                               unsigned long long* next_chunk, int refill_min, int take, double* ghist_all, KernargParams Pk) {
  extern __shared__ float lds[];
  constexpr int NP = A::NP;
  // kRegs: samples and voxel queue in registers, LDS for the correction pairs only -- the form launched as one-wave
  // workgroups (kWg == 64; see launch_persistent: six or eight waves per CU instead of four)
  constexpr bool kWaveWg = kRegs;
  static_assert(kRegs ? (kChunk == 64 && A::kNte > 0 && A::kNte <= 8) : kWg == kBlock,
                "workgroup of 256 lanes, or waves taking 64-voxel chunks with the samples in registers");
  constexpr int kStride = kWaveWg ? 64 : kLdsStride;  // sample columns: the +1 pad is for the 256-wide transposes only
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* col = lds + threadIdx.x;
  // LDS, kWg == 256: [n_te][257] float sample columns | [kHistDoubles][256] double solver history | 4 queues
  //      kRegs:      [kHistDoubles][kWg] double solver history, nothing else (samples and queue are in registers)
  double* hist = reinterpret_cast<double*>(lds + (kWaveWg ? 0 : ((P.n_te * kStride + 1) & ~1))) + threadIdx.x;
  uint32_t* queue = reinterpret_cast<uint32_t*>(hist - threadIdx.x + A::kHistDoubles * kWg) + wave * kQueueCap;
  // A::kGlobalPart: this wave's M x 64 doubles of the pairs' global part ([ring slot][lane], 5 KiB, L2-resident)
  double* ghist = nullptr;
  if constexpr (A::kGlobalPart)
    ghist = ghist_all + ((size_t)blockIdx.x * (kWg / 64) + wave) * (A::Solver::M * 64) + lane;
  uint32_t qv = 0;  // kWaveWg: lane r holds the r-th waiting voxel of the chunk last taken
  const unsigned long long lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const EchoView y{col, kStride};
  int q_head = 0, q_count = 0;
  bool chunks_left = true;
  bool busy = false, done = false;
  int64_t v = 0;
  typename A::Solver s;
  ObjCtx c;
  c.P = &P;
  c.y = y;
  // The uniform inputs that only the refill path reads -- the table start point and box, the no-prior bounds, `norm` and
  // `no_prior` -- are not held in scalar registers for the life of the wave (18 of them for the box alone, spilled to
  // lanes of a vector register and read back beside the solver round): the refill path reads them each time through
  // `Pk`, the kernel's own pointer to `P` in its argument segment, behind a barrier the optimiser cannot see through, so
  // the loads stay where they are written.
  auto refill_params = [Pk] {
    auto kp = Pk;
    asm volatile("" : "+s"(kp));
    return kp;
  };
  // diagnostic builds (t2fit_diag.h): nothing in the product
  T2_STAMPS_BEGIN(queue - wave * kQueueCap + (kBlock / 64) * kQueueCap, wave, lane, c)
  T2_RECORD_PLACEMENT(next_chunk, blockIdx.x * (kWg / 64) + wave, lane)
  bool parked = false;  // split solvers: digest() done, begin_pass() asked to be run again (see the round below)
  int pend = 0;
  // kWaveWg: the chunk queue is read two steps ahead, so that taking a chunk never waits for memory -- chunk A has
  // its base and its mask bytes (loaded when the chunk before it was taken), chunk B its counter value (lane 0)
  // one counter increment hands a wave `take` 64-voxel chunks in a row (launch_persistent: 2)
  const int kTake = take;
  int64_t base_a = 0;
  int sub_a = 0;
  uint32_t idx_b = 0;
  uint8_t mask_a = 0;
  auto load_mask = [&](int64_t base) -> uint8_t {
    const int64_t vv = base + lane;
    return vv < n_vox ? (mask ? mask[vv] : (uint8_t)1) : (uint8_t)0;
  };
  if constexpr (kWaveWg) {
    uint32_t c0 = 0;
    if (lane == 0) c0 = (uint32_t)atomicAdd(next_chunk, 1ull);
    base_a = (int64_t)__shfl(c0, 0, 64) * (64 * kTake);
    mask_a = load_mask(base_a);
    if (lane == 0) idx_b = (uint32_t)atomicAdd(next_chunk, 1ull);
  }
  for (;;) {
    // Refill in batches: the refill path (sample loads, seed / set-up) runs with only the idle lanes
    // active, so it is entered when at least refill_min lanes are idle (or nothing is running).
    unsigned long long need = __ballot(!busy);
    if (__popcll(need) >= refill_min || need == ~0ull) {
      // (a loop of its own for the rare wave whose new voxels all ended at once -- samples that cannot be fitted -- so
      // that the round below has ONE way in and the solver state one version per trip of the main loop: with a
      // `continue` around the round the compiler kept the state in two register sets and copied it across, ~100 moves
      // per round)
      do {
      T2_BLK_T0(t_rf)
      // lanes that finished since the last refill hand in their results here, together, rather than one
      // or two at a time in the round they finished (the conversion and the stores are divergent code)
      if (done) {
        LaneResult r;
        A::result(s, c, r);
        store_fit<kExtras>(m, v, r);
        done = false;
      }
      bool fresh = false;
      if constexpr (kWaveWg) {
        // The queue is one register: a chunk's active voxels are compacted into lanes 0.. (ds_permute: lane j sends its
        // voxel to the lane of its rank among the active ones) and idle lane number r reads entry q_head + r back
        // (ds_bpermute).  Serve from what is left of the last chunk, then take chunks until every idle lane has a voxel.
        unsigned long long want = need;
        for (;;) {
          if (q_count == 0) {
            if (!chunks_left) break;
            const int64_t base = base_a;
            if (base >= n_vox) { chunks_left = false; break; }
            const int64_t vv = base + lane;
            const bool act = mask_a != 0;
            // step the read-ahead: B's counter value has been back for a while; its mask bytes and the next counter
            // value are needed when the next chunk is taken, many rounds from now
            if (++sub_a < kTake) {
              base_a += 64;
              mask_a = load_mask(base_a);
            } else {
              sub_a = 0;
              base_a = (int64_t)__shfl(idx_b, 0, 64) * (64 * kTake);
              mask_a = load_mask(base_a);
              if (lane == 0) idx_b = (uint32_t)atomicAdd(next_chunk, 1ull);
            }
            const unsigned long long b = __ballot(act);
            q_count = __popcll(b);
            q_head = 0;
            // a full permutation: active lanes to the front in order, the others behind them
            const int dst = act ? __popcll(b & lt_mask) : q_count + __popcll(~b & lt_mask);
            qv = (uint32_t)__builtin_amdgcn_ds_permute(dst << 2, (int)(uint32_t)vv);
            if (vv < n_vox && !act) store_masked<kExtras, true>(m, vv);
            if (q_count == 0) continue;
          }
          const int rank = __popcll(want & lt_mask);
          const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute(((q_head + rank) & 63) << 2, (int)qv);
          if (!busy && rank < q_count) {
            v = (int64_t)got;
            busy = true;
            fresh = true;
          }
          const int n_want = __popcll(want);
          const int taken = n_want < q_count ? n_want : q_count;
          q_head += taken;
          q_count -= taken;
          want = __ballot(!busy);
          if (want == 0ull) break;
        }
      } else {
      const int n_need = __popcll(need);
      while (q_count < n_need && chunks_left) {
        unsigned long long cidx = 0;
        if (lane == 0) cidx = atomicAdd(next_chunk, 1ull);
        cidx = __shfl(cidx, 0, 64);
        const int64_t base = (int64_t)cidx * kChunk;
        if (base >= n_vox) { chunks_left = false; break; }
        if (q_head != 0) {  // fewer than 64 entries are left: move them to the front
          uint32_t tmp = 0;
          if (lane < q_count) tmp = queue[q_head + lane];
          if (lane < q_count) queue[lane] = tmp;
          q_head = 0;
        }
        // all mask bytes of the chunk first (independent loads, one latency), then the queue
        // pushes, then the zero stores of the masked-out voxels
        bool act[kChunk / 64];
#pragma unroll
        for (int q = 0; q < kChunk / 64; ++q) {
          const int64_t vv = base + q * 64 + lane;
          act[q] = vv < n_vox && (mask == nullptr || mask[vv] != 0);
        }
#pragma unroll
        for (int q = 0; q < kChunk / 64; ++q) {
          const unsigned long long b = __ballot(act[q]);
          if (act[q]) queue[q_count + __popcll(b & lt_mask)] = (uint32_t)(base + q * 64 + lane);
          q_count += __popcll(b);
        }
#pragma unroll
        for (int q = 0; q < kChunk / 64; ++q) {
          const int64_t vv = base + q * 64 + lane;
          if (vv < n_vox && !act[q]) store_masked<kExtras, true>(m, vv);
        }
      }
      if (!busy) {
        const int rank = __popcll(need & lt_mask);
        if (rank < q_count) {
          v = (int64_t)queue[q_head + rank];
          busy = true;
          fresh = true;
        }
      }
      const int taken = n_need < q_count ? n_need : q_count;
      q_head += taken;
      q_count -= taken;
      }
      if (fresh) {
        // this lane's samples: up to 8 loads in flight, checked in registers, parked in its LDS
        // column (already divided by the row maximum when cfg.norm, run_t2mapping.py:237-238)
        bool finite = true;
        float ymax = 0.0f, y0 = 0.0f;
        const int n_te = A::kNte > 0 ? A::kNte : P.n_te;
        float first8[8] = {};  // echo-count specialisations: the samples stay in registers (A::take_sample)
        for (int i0 = 0; i0 < n_te; i0 += 8) {
          float tmp[8];
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (i0 + j < n_te)
              // (plain loads.  Non-temporal ones keep more of the half-written map lines of the voxels still being
              // fitted in L2 -- LM float32 writes 313 instead of 425 MB per volume -- but every 128-byte line of samples
              // is then fetched once per refill that touches it: 1.7 x the reads, 4 % slower)
              tmp[j] = T2_SAMPLE_LOAD(layout == T2FIT_LAYOUT_TE_MAJOR ? &echoes[(int64_t)(i0 + j) * n_vox + v]
                                                                      : &echoes[v * n_te + (i0 + j)]);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (i0 + j < n_te) {
              const float sv = tmp[j];
              if constexpr (!kWaveWg) col[(i0 + j) * kStride] = sv;
              if (i0 == 0) first8[j] = sv;
              finite = finite && t2_finite(sv);
              if (i0 + j == 0) { y0 = sv; ymax = sv; }
              ymax = sv > ymax ? sv : ymax;
            }
        }
        const auto* const Pr = refill_params();
        if (Pr->norm) {
          if constexpr (A::kNte > 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (j < n_te) {
                const float sv = first8[j] / ymax;
                first8[j] = sv;
                if constexpr (!kWaveWg) col[j * kStride] = sv;
                finite = finite && t2_finite(sv);
              }
          } else {
            for (int i = 0; i < n_te; ++i) {
              const float sv = col[i * kStride] / ymax;
              col[i * kStride] = sv;
              finite = finite && t2_finite(sv);
            }
          }
        }
        if constexpr (A::kNte > 0)
          static_for<0, 8>([&](auto JC) { A::template take_sample<decltype(JC)::value>(s, first8[decltype(JC)::value]); });
        double box_x0[3], lb[3], ub[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { box_x0[j] = Pr->x0[j]; lb[j] = Pr->lb[j]; ub[j] = Pr->ub[j]; }
        if (Pr->no_prior) {  // run_t2mapping.py:243-245
          lb[0] = (double)y0; ub[0] = Pr->np_k_ub;
          lb[1] = Pr->np_t2_lb; ub[1] = Pr->np_t2_ub;
        }
        bool feasible = true;
#pragma unroll
        for (int j = 0; j < NP; ++j) feasible = feasible && !(lb[j] > ub[j]);
        if (!feasible || !finite) {  // nothing to iterate on (fit_lane_t documents both cases)
          LaneResult r;
          r.nit = 0; r.nfev = 0; r.fun = NAN;
#pragma unroll
          for (int j = 0; j < 3; ++j)
            r.x[j] = !feasible ? (j < NP ? NAN : 0.0) : (j < NP ? t2_clip(box_x0[j], lb[j], ub[j]) : 0.0);
          r.status = !feasible ? T2FIT_ST_INFEASIBLE : T2FIT_ST_NONFINITE;
          store_fit<kExtras>(m, v, r);
          busy = false;
        } else {
          if constexpr (kTrace) {  // per-iteration trace of this voxel (voxel seam only)
            c.trace = m.trace + (size_t)v * 4 * m.trace_cap;
            c.trace_cap = m.trace_cap;
            c.trace_n = m.trace_len + v;
            *c.trace_n = 0;
          }
          A::init(s, c, box_x0, lb, ub, hist, kWg, ghist);
          if constexpr (A::kSplit) { T2_STAMPS_ATTACH(s) }
        }
      }
      T2_BLK_END(c, 8, t_rf)
      need = __ballot(!busy);
      } while (need == ~0ull && (chunks_left || q_count != 0));
    }
    if (__ballot(busy) == 0ull) break;  // nothing running and nothing left to take
    if constexpr (A::kSplit) {
      // One round: every lane with a point to evaluate evaluates it (uniform code) and digests the result; lanes whose
      // line search has ended then run begin_pass() (B, Cauchy point, subspace step, line-search set-up).  `parked`: the
      // pass asked to be run again (memory dropped, line search could not start: rare) -- the lane comes back in the next
      // round and skips the evaluation.  One region under `busy`, so that the solver state has one version per round.
      if (busy) {
        if (!parked) {
          T2_BLK_T0(t_ev)
          s.eval(c);
          T2_BLK_END(c, 7, t_ev)
          pend = s.digest(c);
        }
        if (pend == A::Solver::GO_BEGIN || pend == A::Solver::GO_FAIL) {
          T2_BLK_T0(t_bg)
          pend = s.begin_pass(c, pend);
          T2_BLK_END(c, 9, t_bg)
        }
        parked = pend == A::Solver::GO_BEGIN || pend == A::Solver::GO_FAIL;
        if (pend == A::Solver::GO_DONE) { busy = false; done = true; }
      }
    } else {
      if (busy) s.eval(c);
      if (busy && s.advance(c)) {
        busy = false;
        done = true;
      }
    }
  }
  if (done) {  // (every exit passes through the refill block above; kept for safety)
    LaneResult r;
    A::result(s, c, r);
    store_fit<kExtras>(m, v, r);
  }
  T2_STAMPS_END(next_chunk, lane)
}

// The kernel proper.  kWavesPerSimd is the occupancy the register allocator is asked to keep: 1 for the
// float64 solvers (the L-BFGS-B lane alone holds ~340 registers), 4 for the float32 LM lane, which sits a few
// registers above the 128-register line of four waves per SIMD without the hint.
template <class A, int kChunk, bool kTrace = false, int kWavesPerSimd = 1, bool kExtras = true, int kWg = kBlock,
          bool kRegs = false>
__global__ __launch_bounds__(kWg, kWavesPerSimd) void fit_persistent_kernel(const LaneParams P,
                                                                    const float* __restrict__ echoes, int layout,
                                                                    const uint8_t* __restrict__ mask, int64_t n_vox,
                                                                    DevMaps m, unsigned long long* next_chunk, int refill_min,
                                                                    int take, double* ghist) {
  // (`P` is this kernel's first argument: it lies at the start of the argument segment)
  persistent_fit<A, kChunk, kTrace, kExtras, kWg, kRegs>(P, echoes, layout, mask, n_vox, m, next_chunk, refill_min, take, ghist,
                                                         (KernargParams)__builtin_amdgcn_kernarg_segment_ptr());
}

// Residual map (utils/t2map_utils.py:62-89) and optional R^2 from float32 maps already on the device.
// Also the second, fully uniform pass of the reference-trajectory fit: the persistent kernel stores
// t2/k/sigma only, because a lane that evaluated 8 float64 exp() for one finished voxel would hold
// up the other 63 lanes of its wave.
__global__ __launch_bounds__(kBlock) void residuals_kernel(const LaneParams P, const float* __restrict__ echoes,
                                                           int layout, const uint8_t* __restrict__ mask,
                                                           int64_t n_vox, const float* __restrict__ t2,
                                                           const float* __restrict__ k,
                                                           const float* __restrict__ sigma, float* res, float* r2,
                                                           float* se) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kBlock;
  const int64_t v = base + lane;
  const bool in_range = v < n_vox;
  const bool active = in_range && (mask == nullptr || mask[v] != 0);
  stage_echoes(lds, echoes, layout, P.n_te, n_vox, base, active);
  if (!in_range) return;
  float out = 0.0f, out2 = 0.0f, out3 = 0.0f;
  if (active) {
    bool finite;
    float y0_raw;
    const ObjCtx c = prepare_samples(P, lds + lane, kLdsStride, finite, y0_raw);
    const float kv = k[v], tv = t2[v], sv = sigma ? sigma[v] : 0.0f;
    out = residual_mean(c, kv, tv, sv);
    if (r2) out2 = r_squared(c, (double)kv, (double)tv, (double)sv);
    if (se) out3 = t2_std_error(c, (double)kv, (double)tv, (double)sv);
  }
  res[v] = out;
  if (r2) r2[v] = out2;
  if (se) se[v] = out3;
}

// ---- launch helpers -----------------------------------------------------------------------------
using FitKernel = void (*)(const LaneParams, const float*, int, const uint8_t*, int64_t, DevMaps);

FitKernel pick_kernel(const t2fit_config& c) {
  if (c.solver == T2FIT_SOLVER_LM) {
    if (c.precision == T2FIT_PREC_F32)
      return c.model == T2FIT_MODEL_GAUSSIAN
                 ? fit_volume_kernel<T2FIT_SOLVER_LM, T2FIT_PREC_F32, T2FIT_MODEL_GAUSSIAN>
                 : fit_volume_kernel<T2FIT_SOLVER_LM, T2FIT_PREC_F32, T2FIT_MODEL_GAUSSIAN_RICIAN>;
    return c.model == T2FIT_MODEL_GAUSSIAN
               ? fit_volume_kernel<T2FIT_SOLVER_LM, T2FIT_PREC_F64, T2FIT_MODEL_GAUSSIAN>
               : fit_volume_kernel<T2FIT_SOLVER_LM, T2FIT_PREC_F64, T2FIT_MODEL_GAUSSIAN_RICIAN>;
  }
  if (c.solver == T2FIT_SOLVER_LOGLIN)  // voxel-major stacks, ragged sizes, unaligned views: one voxel per lane
    return fit_volume_kernel<T2FIT_SOLVER_LOGLIN, T2FIT_PREC_F64, T2FIT_MODEL_GAUSSIAN>;
  return nullptr;  // the L-BFGS-B solver runs in the persistent kernel
}

// more than the reference's four maps is wanted: the kernels' kExtras forms
bool wants_extras(const DevMaps& dm) { return dm.r2 || dm.se || dm.fun || dm.nit || dm.status || dm.xd || dm.fund; }

// what every launch_persistent<...> call of one fit repeats
struct LaunchArgs {
  unsigned grid; size_t lds_samples; hipStream_t st;
  const LaneParams& P; const float* echoes; int layout; const uint8_t* mask; int64_t n_vox; const DevMaps& dm;
  unsigned long long* counter;
  bool big;  // large-volume kernels (kLargeOnly instantiations are only reached with it set)
};

// kLargeOnly: instantiate the two large-volume kernels only (the echo-count specialisations; small volumes and
// traced voxel batches use the generic lane, where compile time buys nothing)
// kWaveOnly: instantiate the one-wave-workgroup kernels of A only (the less common echo counts: compile time); where
// they do not apply (T2FIT_WAVE_WG=0, diagnostic builds) hipErrorNotSupported tells the caller to use the generic lane
template <class A, bool kLargeOnly = false, bool kWaveOnly = false>
hipError_t launch_persistent(const LaunchArgs& a) {
  constexpr int W = A::kWavesPerSimd;
  const Tuning& tune = tuning();
  const DevMaps& dm = a.dm;
  const bool extras = wants_extras(dm);
  const int refill_min = tune.refill_min > 0 ? tune.refill_min : A::kRefillMin;  // (A::WaveWg has A's)
  if constexpr (!kPhaseStamps && kLargeOnly && A::kHistDoubles > 0 && A::kWaveWgOk) {
    // One-wave workgroups.  The lane's correction pairs (400 B with three parameters, 240 B with two: s is kept as a
    // direction, t2fit_lbfgsb.h load_s) cap a CU's 160 KiB of LDS at 409 lanes: four waves as one 256-lane workgroup,
    // six as one-wave workgroups (round 2), and EIGHT -- two on every SIMD, what the lane's 256 registers allow -- once
    // one of a pair's five numbers lives elsewhere (A::WaveWg: 320 B per lane, 16 of a CU's 128 LDS pieces per wave).
    // Elsewhere is the lane's own registers for the least-squares lanes (Lbfgsb<.., PAIRS_REG>: ten doubles, 221 -> 241
    // registers at 8 echoes, nothing spilled to memory; no allocation, no traffic), and global memory for the Rician
    // likelihood, which fills its 256 registers as it is (PAIRS_GLOBAL: M x 64 doubles per wave, 10 MiB for the whole
    // chip, read back from L2).  Measured on one box with the global part, maps identical bit for bit: 256^3 x 8 TE
    // 13.62 -> 12.02 ms; with the split ring but capped at six waves 14.05 (the global accesses cost 3 %), at seven
    // 12.96 (profiles/r03_exp3_eight_waves.txt); global part against registers: profiles/r10_pair_registers_ab.txt.
    // Nothing but the pairs is in LDS: the samples are in registers (echo-count specialisation), the voxel queue too.
    if (tune.wave_wg) {
      using AW = typename A::WaveWg;  // three parameters: one number of every pair outside LDS, 320 B of LDS per lane
      constexpr int kHint = AW::kWaveWgHint;  // waves per SIMD the register allocator is held to
      auto k64 = extras ? fit_persistent_kernel<AW, kChunkSmall, false, kHint, true, 64, true>
                        : fit_persistent_kernel<AW, kChunkSmall, false, kHint, false, 64, true>;
      unsigned wg = 64;
      if constexpr (kWgShapeDiag) {  // T2FIT_WAVE_WG=2 / 3: the same register-queue code in workgroups of 256 / 128 lanes
        if (tune.wave_wg == 2) { k64 = fit_persistent_kernel<AW, kChunkSmall, false, 1, false, 256, true>; wg = 256; }
        if (tune.wave_wg == 3) { k64 = fit_persistent_kernel<AW, kChunkSmall, false, 1, false, 128, true>; wg = 128; }
      }
      size_t lds64 = (size_t)AW::kHistDoubles * wg * sizeof(double);
      // (LDS is handed out in 1280-byte pieces, 128 to a CU: measured with tools/diag/wave_placement_probe.hip, five
      // workgroups of 32000 bytes are resident together, of 32768 four)
      unsigned per_cu = (unsigned)std::min<size_t>(wg == 64 ? 4 * kHint : 512 / wg, 128 / ceil_div<size_t>(lds64, 1280));
      if (tune.waves_per_cu > 0 && (unsigned)tune.waves_per_cu < per_cu) {  // A/B switch: pad the allocation so that no more fit
        per_cu = (unsigned)tune.waves_per_cu;
        lds64 = (size_t)(128 / per_cu) * 1280;
      }
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k64), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)lds64);
      if (e != hipSuccess) return e;
      int dev = 0, cus = 0;
      if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
      if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
      // every wave that fits is resident; more would only start to leave
      const unsigned n_wg = std::min<unsigned>(a.grid, (unsigned)cus) * per_cu;
      double* ghist = nullptr;
      if constexpr (AW::kGlobalPart) {  // Rician likelihood only: M x 64 doubles per wave (5 KiB; 10 MiB for the whole chip),
        // kept between launches (t2fit_support.h): the kernel keeps live solver state in it
        e = scratch_get(a.st, kScratchRing, (size_t)n_wg * (wg / 64) * AW::Solver::M * 64 * sizeof(double), &ghist);
        if (e != hipSuccess) return e;
      }
      hipLaunchKernelGGL(k64, dim3(n_wg), dim3(wg), lds64, a.st, a.P, a.echoes, a.layout, a.mask, a.n_vox, dm, a.counter,
                         refill_min, tune.take > 0 ? tune.take : 2, ghist);
      return hipGetLastError();
    }
  }
  if constexpr (kWaveOnly) {
    return hipErrorNotSupported;
  } else {
    auto kern = extras ? fit_persistent_kernel<A, kChunkLarge, false, W, true>
                       : fit_persistent_kernel<A, kChunkLarge, false, W, false>;
    if constexpr (!kLargeOnly) {
      if (dm.trace) kern = fit_persistent_kernel<A, kChunkSmall, true, W>;
      else if (!a.big) kern = fit_persistent_kernel<A, kChunkSmall, false, W>;
    }
    const size_t lds = ((a.lds_samples / sizeof(float) + 1) & ~(size_t)1) * sizeof(float) +
                       (size_t)A::kHistDoubles * kBlock * sizeof(double) +
                       (size_t)(kBlock / 64) * (kQueueCap * sizeof(uint32_t) + kStampLdsBytesPerWave);
    // > 64 KiB of dynamic LDS (the correction pairs of 256 lanes) has to be opted into
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(kBlock), lds, a.st, a.P, a.echoes, a.layout, a.mask, a.n_vox, dm, a.counter,
                       refill_min, 1, (double*)nullptr);
    return hipGetLastError();
  }
}

// reference-trajectory lane for `model`, specialised for the common echo-train lengths on large volumes
template <int MODEL>
hipError_t launch_lbfgsb(int n_te, const LaunchArgs& a) {
  if (a.big && tuning().nte_special) {
    if (n_te == 8) return launch_persistent<LbfgsbLane<MODEL, 8>, true>(a);
    if (n_te == 6) return launch_persistent<LbfgsbLane<MODEL, 6>, true>(a);
    if (n_te == 3) return launch_persistent<LbfgsbLane<MODEL, 3>, true>(a);
    // 7 / 5 / 4 echoes: the one-wave-workgroup kernels only (16.2 -> 12.6 ms at 5 echoes against the generic lane)
    hipError_t e = hipErrorNotSupported;
    if (tuning().wave_wg == 1) {
      if (n_te == 7) e = launch_persistent<LbfgsbLane<MODEL, 7>, true, true>(a);
      if (n_te == 5) e = launch_persistent<LbfgsbLane<MODEL, 5>, true, true>(a);
      if (n_te == 4) e = launch_persistent<LbfgsbLane<MODEL, 4>, true, true>(a);
    }
    if (e != hipErrorNotSupported) return e;
  }
  return launch_persistent<LbfgsbLane<MODEL>>(a);
}

// converged LM lane in float64; on large volumes with a common echo-train length the echo-count specialisation
template <int NPAR>
hipError_t launch_lm_f64(int n_te, const LaunchArgs& a) {
  if (a.big && tuning().nte_special) {
    if (n_te == 8) return launch_persistent<LmLaneAdaptor<double, NPAR, 8>, true>(a);
    if (n_te == 6) return launch_persistent<LmLaneAdaptor<double, NPAR, 6>, true>(a);
    if (n_te == 3) return launch_persistent<LmLaneAdaptor<double, NPAR, 3>, true>(a);
  }
  return launch_persistent<LmLaneAdaptor<double, NPAR>>(a);
}

// the 4-voxels-per-lane form needs 16-byte aligned planes and maps, a 4-byte aligned mask and <= 64 KiB of LDS
bool loglin_vec_ok(const float* echoes, int layout, const uint8_t* mask, int64_t n_vox, const DevMaps& dm, int n_te) {
  return layout == T2FIT_LAYOUT_TE_MAJOR && n_vox % kLoglinVec == 0 && aligned16(echoes) &&
         (reinterpret_cast<uintptr_t>(mask) & 3u) == 0 && aligned16(dm.t2) && aligned16(dm.k) && aligned16(dm.sigma) &&
         aligned16(dm.res) && (size_t)n_te * kLoglinTile * sizeof(float) <= 65536;
}

}  // namespace

// ---- t2fit_launch.h -------------------------------------------------------------------------------------------------
int t2fit::check_common(const t2fit_config* cfg, const void* echoes, int layout, int64_t n_vox) {
  const char* why;
  const int rc = config_check(cfg, &why);
  if (rc != T2FIT_OK) return fail(rc, why);
  if (!echoes) return fail(T2FIT_E_INVALID, "echoes is NULL");
  if (layout != T2FIT_LAYOUT_TE_MAJOR && layout != T2FIT_LAYOUT_VOXEL_MAJOR) return fail(T2FIT_E_INVALID, "unknown layout");
  if (n_vox < 0) return fail(T2FIT_E_INVALID, "n_vox is negative");
  if (ceil_div<int64_t>(n_vox, kBlock) > 0x7fffffffLL) return fail(T2FIT_E_INVALID, "n_vox too large for one launch");
  return T2FIT_OK;
}

bool t2fit::is_large_volume(int64_t n_vox) { return n_vox > tuning().small_volume; }

int t2fit::launch_fit(const t2fit_config* cfg, const float* echoes, int layout, const uint8_t* mask, int64_t n_vox,
                      const t2fit_maps& maps, hipStream_t st, bool part_of_large, const VoxelOutputs& vox) {
  if (n_vox == 0) return T2FIT_OK;
  const DevMaps dm{maps.t2, maps.k, maps.sigma, maps.res, maps.r2, maps.fun, maps.t2_se, maps.nit, maps.status,
                   vox.xd, vox.fund, vox.trace, vox.trace_len, vox.trace_cap};
  const Tuning& tune = tuning();
  const LaneParams P = make_lane_params(*cfg);
  const unsigned grid = (unsigned)ceil_div<int64_t>(n_vox, kBlock);
  const size_t lds = (size_t)cfg->n_te * kLdsStride * sizeof(float);
  FitKernel kern = pick_kernel(*cfg);
  const bool loglin = cfg->solver == T2FIT_SOLVER_LOGLIN;
  const bool persistent = !loglin && (tune.use_persistent || cfg->solver == T2FIT_SOLVER_LBFGSB);
  if (persistent && n_vox >= 0xffffffffLL) return fail(T2FIT_E_INVALID, "n_vox must be below 2^32 per call");
  unsigned long long* counter = nullptr;
  if (persistent) {
    T2_HIP(hipMallocAsync((void**)&counter, kCounterWords * sizeof(unsigned long long), st));
    T2_HIP(hipMemsetAsync(counter, 0, kCounterWords * sizeof(unsigned long long), st));
  }
  if (g_timing) {
    g_ev_slot = (int)(g_ev_count % kEvRing);
    if (!g_ev0[g_ev_slot]) {
      T2_HIP(hipEventCreate(&g_ev0[g_ev_slot]));
      T2_HIP(hipEventCreate(&g_ev1[g_ev_slot]));
      T2_HIP(hipEventCreate(&g_ev2[g_ev_slot]));
    }
    T2_HIP(hipEventRecord(g_ev0[g_ev_slot], st));
  }
  if (persistent) {
    // one workgroup per CU slot; not required to be co-resident (work comes from an atomic queue)
    const bool big = !dm.trace && (part_of_large || is_large_volume(n_vox));
    const int64_t chunks = ceil_div<int64_t>(n_vox, big ? kChunkLarge : kChunkSmall);
    unsigned pgrid = (unsigned)std::min<int64_t>((chunks + 3) / 4, tune.persistent_blocks);
    const int reserve = g_reserve_cus.load(std::memory_order_relaxed);
    if (reserve > 0 && cfg->solver == T2FIT_SOLVER_LBFGSB) {
      // The resident workgroups of this kernel hold all of a CU's LDS.  Launched `reserve` CUs' worth of workgroups
      // short, the chip keeps that many workgroup slots (LDS and wave slots) free for kernels of other streams (RCCL's
      // all-gather beside the next fit), which otherwise could not become resident before this one drains.  With
      // one-wave workgroups the dispatcher spreads the shortfall over the CUs it likes: free slots, not whole CUs.
      int dev = 0, cus = 0;
      T2_HIP(hipGetDevice(&dev));
      T2_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
      pgrid = std::min<unsigned>(pgrid, (unsigned)std::max(1, cus - reserve));
    }
    const LaunchArgs a{pgrid, lds, st, P, echoes, layout, mask, n_vox, dm, counter, big};
    const bool two = cfg->model == T2FIT_MODEL_GAUSSIAN;
    hipError_t pe;
    if (cfg->solver == T2FIT_SOLVER_LBFGSB) {
      if (two) pe = launch_lbfgsb<T2FIT_MODEL_GAUSSIAN>(cfg->n_te, a);
      else if (cfg->model == T2FIT_MODEL_GAUSSIAN_RICIAN) pe = launch_lbfgsb<T2FIT_MODEL_GAUSSIAN_RICIAN>(cfg->n_te, a);
      else pe = launch_lbfgsb<T2FIT_MODEL_RICIAN>(cfg->n_te, a);
    } else if (cfg->precision == T2FIT_PREC_F32) {
      // (float32 stays on the generic lane: the specialised evaluation keeps eight echoes in flight, which does not fit
      // the 128 registers of four waves per SIMD -- 204 B/lane of scratch, 2.0 ms -- and loses at three waves: 1.27 vs
      // 1.20 ms; float64: 2.73 vs 2.96 ms)
      pe = two ? launch_persistent<LmLaneAdaptor<float, 2>>(a) : launch_persistent<LmLaneAdaptor<float, 3>>(a);
    } else {
      pe = two ? launch_lm_f64<2>(cfg->n_te, a) : launch_lm_f64<3>(cfg->n_te, a);
    }
    if (pe != hipSuccess) {
      (void)hipFreeAsync(counter, st);
      return fail(T2FIT_E_HIP, std::string("persistent fit launch: ") + hipGetErrorString(pe));
    }
    if (g_timing) T2_HIP(hipEventRecord(g_ev1[g_ev_slot], st));  // the fit kernel ends here; the epilogue pass is a separate, HBM-bound launch
    hipLaunchKernelGGL(residuals_kernel, dim3(grid), dim3(kBlock), lds, st, P, echoes, layout, mask, n_vox,
                       (const float*)dm.t2, (const float*)dm.k, (const float*)dm.sigma, dm.res, dm.r2, dm.se);
    if (g_timing) {
      T2_HIP(hipEventRecord(g_ev2[g_ev_slot], st));
      ++g_ev_count;
    }
  } else if (loglin && loglin_vec_ok(echoes, layout, mask, n_vox, dm, cfg->n_te)) {
    hipLaunchKernelGGL(wants_extras(dm) ? loglin_volume_kernel<true> : loglin_volume_kernel<false>,
                       dim3((unsigned)ceil_div<int64_t>(n_vox, kLoglinTile)), dim3(kBlock),
                       (size_t)cfg->n_te * kLoglinTile * sizeof(float), st, P, echoes, mask, n_vox, dm);
  } else {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, P, echoes, layout, mask, n_vox, dm);
  }
  T2_HIP(hipGetLastError());
  if (g_timing && !persistent) {  // one-pass kernels: no epilogue (its time reads 0)
    T2_HIP(hipEventRecord(g_ev1[g_ev_slot], st));
    T2_HIP(hipEventRecord(g_ev2[g_ev_slot], st));
    ++g_ev_count;
  }
  if (counter && cfg->solver == T2FIT_SOLVER_LBFGSB) {  // diagnostic builds (t2fit_diag.h): nothing in the product
    if (const int rc = report_stamps(counter, st)) return rc;
    if (const int rc = report_placement(counter, st)) return rc;
  }
  if (counter) T2_HIP(hipFreeAsync(counter, st));
  return T2FIT_OK;
}

extern "C" {

int t2fit_set_reserve_cus(int cus) {
  g_reserve_set.store(true);
  return g_reserve_cus.exchange(std::max(0, cus));
}

int t2fit_set_timing(int enabled) {
  g_timing = enabled != 0;
  g_ev_count = 0;
  return T2FIT_OK;
}

double t2fit_kernel_ms(int launches_ago) { return event_ms(launches_ago, g_ev0, g_ev1); }

double t2fit_last_kernel_ms(void) { return t2fit_kernel_ms(0); }

double t2fit_epilogue_ms(int launches_ago) { return event_ms(launches_ago, g_ev1, g_ev2); }

int t2fit_volume_dev(const t2fit_config* cfg, const float* echoes_dev, int layout, const uint8_t* mask_dev,
                     int64_t n_vox, const t2fit_maps* maps, void* stream) {
  int rc = check_common(cfg, echoes_dev, layout, n_vox);
  if (rc != T2FIT_OK) return rc;
  if (!maps || !maps->t2 || !maps->k || !maps->sigma || !maps->res)
    return fail(T2FIT_E_INVALID, "maps->t2/k/sigma/res must be non-NULL");
  return launch_fit(cfg, echoes_dev, layout, mask_dev, n_vox, *maps, (hipStream_t)stream);
}

int t2fit_residuals_dev(const t2fit_config* cfg, const float* echoes_dev, int layout, const uint8_t* mask_dev,
                        int64_t n_vox, const float* t2, const float* k, const float* sigma, float* res, void* stream) {
  int rc = check_common(cfg, echoes_dev, layout, n_vox);
  if (rc != T2FIT_OK) return rc;
  if (!t2 || !k || !res) return fail(T2FIT_E_INVALID, "t2/k/res must be non-NULL");
  if (n_vox == 0) return T2FIT_OK;
  const LaneParams P = make_lane_params(*cfg);
  const unsigned grid = (unsigned)ceil_div<int64_t>(n_vox, kBlock);
  const size_t lds = (size_t)cfg->n_te * kLdsStride * sizeof(float);
  hipLaunchKernelGGL(residuals_kernel, dim3(grid), dim3(kBlock), lds, (hipStream_t)stream, P, echoes_dev, layout,
                     mask_dev, n_vox, t2, k, sigma, res, (float*)nullptr, (float*)nullptr);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

}  // extern "C"

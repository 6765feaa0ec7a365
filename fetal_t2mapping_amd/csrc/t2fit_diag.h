// t2fit_diag.h -- everything the two diagnostic builds add to the fit, and nothing the product build keeps.
//   -DT2_PHASE_STAMPS   where do a wave's cycles go?  T2_BLK_T0 / T2_BLK_END stamp the blocks of the lane solver and of
//                       the persistent loop: each wave adds (cycles, lanes active, entries) per block to counters in its
//                       own LDS, the kernel adds them up over the grid at exit, launch_fit prints the table.
//   -DT2_WG_SHAPE_DIAG  where did the dispatcher put the waves?  Every wave of the persistent kernel records its HW_ID /
//                       XCC_ID; launch_fit prints waves per SIMD by CU when T2FIT_PLACEMENT is set.  Also lets
//                       T2FIT_WAVE_WG=2 / 3 run the register-queue code in workgroups of 256 / 128 lanes.
// The two macros are tested in this file and nowhere else; the fit calls the hooks below by name and in the product
// build every one of them expands to nothing.  A diagnostic build overwrites the product library: no test or benchmark
// runs against one.
#pragma once

#if defined(__HIPCC__)  // (the lane headers are also compiled by g++ into the host-side lane simulator)
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "t2fit_error.h"
#endif

namespace t2fit {

constexpr int kDiagBlocks = 11, kDiagWords = 3 * kDiagBlocks;  // stamps: (cycles, lanes, entries) per block
#if defined(T2_PHASE_STAMPS)
constexpr bool kPhaseStamps = true;  // (the one-wave-workgroup kernels keep nothing but pairs in LDS: not launched)
#define T2_DIAG_COUNTERS unsigned long long* diag = nullptr;  // member of ObjCtx / Lbfgsb: the wave's block counters
#else
constexpr bool kPhaseStamps = false;
#define T2_DIAG_COUNTERS
#endif
#if defined(T2_WG_SHAPE_DIAG)
constexpr bool kWgShapeDiag = true;
constexpr int kPlaceWords = 4096;  // HW_ID / XCC_ID of every wave of the persistent kernel
#else
constexpr bool kWgShapeDiag = false;
constexpr int kPlaceWords = 0;
#endif
constexpr int kCounterWords = 16 + kDiagWords + kPlaceWords;  // chunk counter + diagnostic totals

}  // namespace t2fit

#if defined(T2_PHASE_STAMPS) && defined(__HIP_DEVICE_COMPILE__)
#define T2_BLK_T0(name) const unsigned long long name = __builtin_amdgcn_s_memtime();
#define T2_BLK_END(c, i, t0) t2_blk_end((c).diag, i, t0);
__device__ __forceinline__ void t2_blk_end(unsigned long long* dg, int i, unsigned long long t0) {
  const unsigned long long dt = __builtin_amdgcn_s_memtime() - t0;
  const unsigned long long ex = __ballot(true);
  if ((int)(threadIdx.x & 63) == __ffsll((long long)ex) - 1) {
    dg[3 * i] += dt;
    dg[3 * i + 1] += (unsigned long long)__popcll(ex);
    dg[3 * i + 2] += 1ull;
  }
}
#else
#define T2_BLK_T0(name)
#define T2_BLK_END(c, i, t0)
#endif

#if defined(__HIPCC__)
namespace t2fit {

// Hooks of the persistent loop.  Macros: a product build must not even evaluate their arguments (dead uses change the
// optimiser's use lists and with them the kernels' register allocation).  Stamps: kDiagWords words of LDS per wave
// behind the voxel queues, zeroed at the start, added to the grid's totals at the end; block 10 is the wave's life.
#if defined(T2_PHASE_STAMPS)
constexpr size_t kStampLdsBytesPerWave = kDiagWords * sizeof(unsigned long long);
#define T2_STAMPS_BEGIN(lds_behind_queues, wave, lane, c)                                                         \
  unsigned long long* diag = reinterpret_cast<unsigned long long*>(lds_behind_queues) + (wave) * kDiagWords;      \
  if ((lane) < kDiagWords) diag[lane] = 0ull;                                                                     \
  (c).diag = diag;                                                                                                \
  const unsigned long long st_all = __builtin_amdgcn_s_memtime();
#define T2_STAMPS_ATTACH(s) (s).diag = diag;
#define T2_STAMPS_END(counter, lane)                                           \
  if ((lane) == 0) diag[3 * 10] += __builtin_amdgcn_s_memtime() - st_all;      \
  if ((lane) < kDiagWords) atomicAdd((counter) + 16 + (lane), diag[lane]);
#else
constexpr size_t kStampLdsBytesPerWave = 0;
#define T2_STAMPS_BEGIN(lds_behind_queues, wave, lane, c)
#define T2_STAMPS_ATTACH(s)
#define T2_STAMPS_END(counter, lane)
#endif
// wave number `w` of the grid notes where the dispatcher put it
#if defined(T2_WG_SHAPE_DIAG)
#define T2_RECORD_PLACEMENT(counter, w, lane) t2_record_placement(counter, w, lane);
__device__ __forceinline__ void t2_record_placement(unsigned long long* counter, unsigned w, int lane) {
  unsigned hw, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  if (lane == 0 && w < (unsigned)kPlaceWords)
    counter[16 + kDiagWords + w] = 0x100000000ull | ((unsigned long long)(xcc & 0xf) << 20) | (hw & 0xfffff);
}
#else
#define T2_RECORD_PLACEMENT(counter, w, lane)
#endif

// host side, after the launches of an L-BFGS-B fit: fetch the counter block and print what the build collected
inline int report_stamps(const unsigned long long* counter, hipStream_t st) {
#if defined(T2_PHASE_STAMPS)
  unsigned long long h[kCounterWords];
  T2_HIP(hipMemcpyAsync(h, counter, sizeof(h), hipMemcpyDeviceToHost, st));
  T2_HIP(hipStreamSynchronize(st));
  static const char* names[kDiagBlocks] = {"eval + digest", "cauchy: breakpoint taken", "subsm: projected", "begin: build_b",
                                           "begin: cauchy", "begin: subsm", "begin: ls set-up", "eval", "refill",
                                           "begin (all)", "wave life"};
  const double life = (double)h[16 + 3 * 10];
  for (int i = 0; i < kDiagBlocks; ++i) {
    const unsigned long long* d = h + 16 + 3 * i;
    fprintf(stderr, "[t2fit blocks] %-22s %6.2f%% of wave cycles, %5.1f lanes active, %10llu entries, %7.0f cycles each\n",
            names[i], 100.0 * (double)d[0] / life, d[2] ? (double)d[1] / (double)d[2] : 0.0, d[2],
            d[2] ? (double)d[0] / (double)d[2] : 0.0);
  }
#endif
  return T2FIT_OK;
}

inline int report_placement(const unsigned long long* counter, hipStream_t st) {
#if defined(T2_WG_SHAPE_DIAG)
  if (!std::getenv("T2FIT_PLACEMENT")) return T2FIT_OK;
  std::vector<unsigned long long> h(kCounterWords);
  T2_HIP(hipMemcpyAsync(h.data(), counter, h.size() * 8, hipMemcpyDeviceToHost, st));
  T2_HIP(hipStreamSynchronize(st));
  std::map<unsigned, std::array<int, 4>> cu;
  for (int i = 0; i < kPlaceWords; ++i) {
    const unsigned long long v = h[16 + kDiagWords + i];
    if (!(v >> 32)) continue;
    const unsigned hw = (unsigned)v & 0xfffff, xcc = ((unsigned)v >> 20) & 0xf;
    cu[(xcc << 16) | ((hw >> 8) & 0xff)][(hw >> 4) & 3]++;
  }
  std::map<std::string, int> pat;
  for (auto& kv : cu) {
    std::array<int, 4> c = kv.second;
    std::sort(c.begin(), c.end());
    char b[64];
    snprintf(b, sizeof b, "%d,%d,%d,%d", c[3], c[2], c[1], c[0]);
    pat[b]++;
  }
  for (auto& kv : pat) fprintf(stderr, "[t2fit placement] %4d CUs with waves per SIMD %s\n", kv.second, kv.first.c_str());
#endif
  return T2FIT_OK;
}

}  // namespace t2fit
#endif  // __HIPCC__

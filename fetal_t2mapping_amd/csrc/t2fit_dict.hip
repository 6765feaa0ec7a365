// t2fit_dict.hip -- dictionary-matching fit (include/t2fit.h: t2fit_dict_pack_host, t2fit_dict_match_dev;
// fetal_t2mapping_amd/_dict.py states the result in numpy and the kernel equals it bit for bit).
//
// The hot path is the product (atoms x n_te) . (n_te x voxels) on v_mfma_f32_32x32x2_f32: atoms are the rows (A operand),
// voxels the columns (B operand), two echoes per instruction in ascending order.  A workgroup is four waves; a wave owns
// G groups of 32 voxels (G accumulators per A operand) and keeps their samples in registers as B operands for the whole
// atom loop.  The normalised atoms stream through LDS in chunks of tiles ([tile][echo][32 rows], so the A operand of a
// k-step is 64 consecutive floats); chunk c holds the tiles c, c + n_chunks, ..: the first chunk already spans the whole
// table, which raises the running best early and keeps the candidate lists short.
//
// The float32 scores only select candidates.  Lane l holds, for the voxel column l & 31, the 16 atom rows
// (r & 3) + 8 (r >> 2) + 4 (l >> 5) of a tile; it keeps a running float32 best over its own rows and re-scores in float64,
// in the statement's order, every atom with s32 >= best - T (T: the error bound of DESIGN.md section 8r, per voxel).  The
// candidates compete on (float64 score, lowest index); lanes l and l + 32 are merged once at the end.  The same kernel then
// computes scale and rmse from the original atom.  The kernel is a template on the k-step count so that every register
// index is a constant: no scratch.  No atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>

#include "t2fit_error.h"
#include "t2fit_support.h"

namespace {

using t2fit::align_up;
using t2fit::ceil_div;
using t2fit::fail;
using t2fit::misaligned;

constexpr uint32_t kMagic = 0x54443254u;
constexpr int kTile = 32;           // atoms of a tile: the rows of one matrix instruction
constexpr int kChunkFloats = 4096;  // LDS floats of one chunk of tiles (16 KiB)
constexpr int kWaves = 4;           // waves of a workgroup (t2fit::kBlock lanes)

struct DictHeader {  // 64 bytes; include/t2fit.h documents the block
  uint32_t magic;
  int32_t n_atoms, n_te, k_pad, n_tiles;
  float dmax;
  uint32_t reserved[2];
  uint64_t off_tiles, off_atoms, off_norm2, bytes;
};
static_assert(sizeof(DictHeader) == 64, "header layout");

bool sizes_ok(int n_atoms, int n_te) { return n_atoms >= 1 && n_atoms <= T2FIT_DICT_MAX_ATOMS && n_te >= 2 && n_te <= T2FIT_MAX_TE; }

DictHeader header_for(int n_atoms, int n_te) {
  DictHeader h;
  std::memset(&h, 0, sizeof(h));
  h.magic = kMagic;
  h.n_atoms = n_atoms;
  h.n_te = n_te;
  h.k_pad = (n_te + 1) / 2 * 2;
  h.n_tiles = ceil_div(n_atoms, kTile);
  h.off_tiles = sizeof(DictHeader);
  h.off_atoms = h.off_tiles + size_t(h.n_tiles) * h.k_pad * kTile * sizeof(float);
  h.off_norm2 = h.off_atoms + align_up(size_t(n_atoms) * n_te * sizeof(float), 16);
  h.bytes = h.off_norm2 + align_up(size_t(n_atoms) * sizeof(double), 16);
  return h;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

#ifdef T2FIT_DICT_NO_RESCORE_BAND
constexpr double kBand = 0.0;  // tools/dict_bench.py only: T = 0 isolates the cost of the float64 re-scores; results are then wrong
#else
constexpr double kBand = 1.0;
#endif

// KS: k-steps (k_pad / 2); G: 32-voxel groups of a wave
template <int KS, int G>
__global__ __launch_bounds__(t2fit::kBlock) void dict_match_kernel(const float* __restrict__ y, int n_te, int64_t n_vox,
                                                                   const uint8_t* __restrict__ mask,
                                                                   const unsigned char* __restrict__ packed,
                                                                   int32_t* __restrict__ index_out, float* __restrict__ scale_out,
                                                                   float* __restrict__ rmse_out) {
  constexpr int KP = 2 * KS;
  constexpr int WV = kTile * G;                       // voxels of a wave
  constexpr int TILE_FLOATS = KP * kTile;
  constexpr int TPC = kChunkFloats / TILE_FLOATS;     // tiles of a chunk (>= 4)
  static_assert(G == 2 || G == 4, "a wave's staging loop covers 64 voxels per step");
  extern __shared__ float lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
  float* dl = lds;                                    // the chunk: [slot][echo][row]
  float* yl = lds + kChunkFloats + wave * (KP * WV);  // this wave's samples: [echo][voxel], padded echoes 0.0

  const DictHeader* hd = reinterpret_cast<const DictHeader*>(packed);
  const int n_atoms = hd->n_atoms, n_tiles = hd->n_tiles;
  const float* tiles = reinterpret_cast<const float*>(packed + hd->off_tiles);
  const float* atoms = reinterpret_cast<const float*>(packed + hd->off_atoms);
  const double* norm2 = reinterpret_cast<const double*>(packed + hd->off_norm2);
  const int64_t v0 = (int64_t(blockIdx.x) * kWaves + wave) * WV;

#pragma unroll
  for (int e = 0; e < KP; ++e)
#pragma unroll
    for (int i = 0; i < WV / 64; ++i) {
      const int64_t v = v0 + i * 64 + lane;
      yl[e * WV + i * 64 + lane] = (e < n_te && v < n_vox) ? y[int64_t(e) * n_vox + v] : 0.0f;
    }
  __syncthreads();

  // per group: is this lane's voxel matched (in the mask, finite, not all zero), is it written as fitted, its band T
  bool matched[G], fitted[G];
  float band[G];
  bool any = false;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int64_t v = v0 + g * kTile + col;
    bool ok = v < n_vox && (mask == nullptr || mask[v] != 0);
    double nn = 0.0;
    for (int e = 0; e < n_te; ++e) {
      const float s = yl[e * WV + g * kTile + col];
      ok = ok && isfinite(s);
      nn += double(s) * double(s);
    }
    fitted[g] = ok;
    matched[g] = ok && nn > 0.0;
    // T = 2 (K + 2) 2^-24 |y| dmax (1 + 2^-20), rounded up to float32 (and never below the smallest normal number)
    const double t = kBand * (2.0 * (KP + 2) * 0x1p-24 * sqrt(matched[g] ? nn : 0.0) * double(hd->dmax) * (1.0 + 0x1p-20) + 0x1p-126);
    float tf = float(t);
    if (double(tf) < t) tf = nextafterf(tf, std::numeric_limits<float>::infinity());
    // where a float32 partial sum could overflow (|y| dmax near the largest float) the scores select nothing: every atom is re-scored
    if (sqrt(nn) * double(hd->dmax) >= 1e38) tf = std::numeric_limits<float>::infinity();
    band[g] = tf;
    any = any || matched[g];
  }
  bool active[G];  // wave-uniform: the group has a voxel to match
#pragma unroll
  for (int g = 0; g < G; ++g) active[g] = __ballot(matched[g]) != 0;

  // B operands: lane l holds y[k = 2 s + (l >> 5)][voxel l & 31]; a voxel that is not matched contributes zeros
  float b[G][KS];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int s = 0; s < KS; ++s) b[g][s] = matched[g] ? yl[(2 * s + half) * WV + g * kTile + col] : 0.0f;

  float best32[G];
  double best64[G];
  int bestj[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    best32[g] = -std::numeric_limits<float>::infinity();
    best64[g] = -std::numeric_limits<double>::infinity();
    bestj[g] = std::numeric_limits<int>::max();
  }

  if (__syncthreads_or(any ? 1 : 0)) {
    const int n_chunks = ceil_div(n_tiles, TPC);
    for (int c = 0; c < n_chunks; ++c) {
      if (c > 0) __syncthreads();  // every wave has finished with the chunk before
      for (int i = threadIdx.x * 4; i < TPC * TILE_FLOATS; i += t2fit::kBlock * 4) {
        const int slot = i / TILE_FLOATS, off = i % TILE_FLOATS, tile = slot * n_chunks + c;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (tile < n_tiles) v = *reinterpret_cast<const float4*>(tiles + size_t(tile) * TILE_FLOATS + off);
        *reinterpret_cast<float4*>(dl + i) = v;
      }
      __syncthreads();
      if (!__ballot(any)) continue;  // (this wave has nothing to match; it still takes part in the barriers)
      for (int slot = 0; slot < TPC; ++slot) {
        const int tile = slot * n_chunks + c;
        if (tile >= n_tiles) break;
        f32x16 acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[g][r] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const float a = dl[slot * TILE_FLOATS + 2 * s * kTile + lane];  // A[row l & 31][k = 2 s + (l >> 5)]
#pragma unroll
          for (int g = 0; g < G; ++g)
            if (active[g]) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[g][s], acc[g], 0, 0, 0);
        }
        // rows of a ragged last tile beyond the table never compete
        const int rows_left = n_atoms - tile * kTile;
        uint64_t cand = 0;
#pragma unroll
        for (int g = 0; g < G; ++g)
          if (matched[g]) {
            float m = best32[g];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
              if (row < rows_left) m = fmaxf(m, acc[g][r]);
            }
            best32[g] = m;
            const float thr = m - band[g];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
              if (row < rows_left && !(acc[g][r] < thr)) cand |= uint64_t(1) << (g * 16 + r);
            }
          }
        while (cand) {
          const int bit = __ffsll(static_cast<unsigned long long>(cand)) - 1;
          cand &= cand - 1;
          const int g = bit >> 4, r = bit & 15;
          const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
          const float* dh = dl + slot * TILE_FLOATS + row;
          const float* ys = yl + g * kTile + col;
          double s = 0.0;
          for (int e = 0; e < n_te; ++e) s += double(dh[e * kTile]) * double(ys[e * WV]);
          const int j = tile * kTile + row;
#pragma unroll
          for (int gg = 0; gg < G; ++gg)
            if (gg == g && (s > best64[gg] || (s == best64[gg] && j < bestj[gg]))) {
              best64[gg] = s;
              bestj[gg] = j;
            }
        }
      }
    }
  }

  // lanes l and l + 32 hold the same voxels: merge, then lane half (g & 1) writes group g
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const double os = __shfl_xor(best64[g], 32);
    const int oj = __shfl_xor(bestj[g], 32);
    if (os > best64[g] || (os == best64[g] && oj < bestj[g])) {
      best64[g] = os;
      bestj[g] = oj;
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int64_t v = v0 + g * kTile + col;
    if (half != (g & 1) || v >= n_vox) continue;
    int j = -1;
    float scale = 0.0f, rmse = 0.0f;
    if (fitted[g]) {
      j = matched[g] ? bestj[g] : 0;  // an all-zero voxel ties on every atom: the lowest index
      if (unsigned(j) >= unsigned(n_atoms)) j = 0;  // (cannot happen: the best float32 score is always re-scored; keeps the reads below in bounds)
      const float* d = atoms + size_t(j) * n_te;
      const float* ys = yl + g * kTile + col;
      double num = 0.0;
      for (int e = 0; e < n_te; ++e) num += double(ys[e * WV]) * double(d[e]);
      const double q = num / norm2[j];
      const double k = q > 0.0 ? q : 0.0;
      double ss = 0.0;
      for (int e = 0; e < n_te; ++e) {
        const double res = double(ys[e * WV]) - k * double(d[e]);
        ss += res * res;
      }
      scale = float(k);
      rmse = float(sqrt(ss / double(n_te)));
    }
    index_out[v] = j;
    scale_out[v] = scale;
    rmse_out[v] = rmse;
  }
}

template <int KS>
hipError_t launch(const float* y, int n_te, int64_t n_vox, const uint8_t* mask, const unsigned char* packed, int32_t* index,
                  float* scale, float* rmse, hipStream_t st) {
  constexpr int G = KS <= 8 ? 4 : 2;  // the samples of a workgroup stay within 32 KiB of LDS
  constexpr int WV = kTile * G;
  const size_t lds_bytes = (size_t(kChunkFloats) + size_t(kWaves) * 2 * KS * WV) * sizeof(float);
  const int64_t blocks = ceil_div<int64_t>(n_vox, int64_t(kWaves) * WV);
  hipLaunchKernelGGL((dict_match_kernel<KS, G>), dim3(static_cast<unsigned>(blocks)), dim3(t2fit::kBlock), lds_bytes, st, y, n_te,
                     n_vox, mask, packed, index, scale, rmse);
  return hipGetLastError();
}

}  // namespace

extern "C" {

int t2fit_dict_pack_bytes(int n_atoms, int n_te, size_t* bytes) {
  if (!bytes) return fail(T2FIT_E_INVALID, "t2fit_dict_pack_bytes: bytes is NULL");
  if (!sizes_ok(n_atoms, n_te))
    return fail(T2FIT_E_INVALID, "t2fit_dict_pack_bytes: n_atoms must be 1 .. " + std::to_string(T2FIT_DICT_MAX_ATOMS) + " and n_te 2 .. " +
                                     std::to_string(T2FIT_MAX_TE) + ", got " + std::to_string(n_atoms) + " and " + std::to_string(n_te));
  *bytes = header_for(n_atoms, n_te).bytes;
  return T2FIT_OK;
}

int t2fit_dict_pack_host(int n_atoms, int n_te, const float* atoms, void* packed_host, size_t bytes) {
  if (!sizes_ok(n_atoms, n_te))
    return fail(T2FIT_E_INVALID, "t2fit_dict_pack_host: n_atoms must be 1 .. " + std::to_string(T2FIT_DICT_MAX_ATOMS) + " and n_te 2 .. " +
                                     std::to_string(T2FIT_MAX_TE) + ", got " + std::to_string(n_atoms) + " and " + std::to_string(n_te));
  if (!atoms || !packed_host) return fail(T2FIT_E_INVALID, "t2fit_dict_pack_host: atoms or packed_host is NULL");
  const DictHeader h = header_for(n_atoms, n_te);
  if (bytes < h.bytes)
    return fail(T2FIT_E_INVALID, "t2fit_dict_pack_host: the buffer has " + std::to_string(bytes) + " bytes, the dictionary needs " +
                                     std::to_string(h.bytes));
  unsigned char* out = static_cast<unsigned char*>(packed_host);
  std::memset(out, 0, h.bytes);
  float* tiles = reinterpret_cast<float*>(out + h.off_tiles);
  double* norm2 = reinterpret_cast<double*>(out + h.off_norm2);
  double dmax = 0.0;
  for (int j = 0; j < n_atoms; ++j) {
    const float* d = atoms + size_t(j) * n_te;
    double n2 = 0.0;
    for (int e = 0; e < n_te; ++e) {
      if (!std::isfinite(d[e])) return fail(T2FIT_E_INVALID, "t2fit_dict_pack_host: atom " + std::to_string(j) + " has a non-finite sample");
      n2 += double(d[e]) * double(d[e]);
    }
    if (!(n2 > 0.0)) return fail(T2FIT_E_INVALID, "t2fit_dict_pack_host: atom " + std::to_string(j) + " has norm 0");
    const double n = std::sqrt(n2);
    float* t = tiles + size_t(j / kTile) * h.k_pad * kTile + j % kTile;
    double h2 = 0.0;
    for (int e = 0; e < n_te; ++e) {
      const float dh = float(double(d[e]) / n);
      t[e * kTile] = dh;
      h2 += double(dh) * double(dh);
    }
    const double hn = std::sqrt(h2);
    if (hn > dmax) dmax = hn;
    norm2[j] = n2;
  }
  std::memcpy(out + h.off_atoms, atoms, size_t(n_atoms) * n_te * sizeof(float));
  DictHeader hw = h;
  hw.dmax = float(dmax);
  std::memcpy(out, &hw, sizeof(hw));
  return T2FIT_OK;
}

int t2fit_dict_match_dev(const float* y_dev, int n_te, int64_t n_vox, const uint8_t* mask_dev, const void* packed_dev, int32_t* index_dev,
                         float* scale_dev, float* rmse_dev, void* stream) {
  if (!y_dev || !packed_dev || !index_dev || !scale_dev || !rmse_dev)
    return fail(T2FIT_E_INVALID, "t2fit_dict_match_dev: y_dev, packed_dev, index_dev, scale_dev or rmse_dev is NULL");
  if (n_te < 2 || n_te > T2FIT_MAX_TE)
    return fail(T2FIT_E_INVALID, "t2fit_dict_match_dev: n_te must be 2 .. " + std::to_string(T2FIT_MAX_TE) + ", got " + std::to_string(n_te));
  if (n_vox < 0) return fail(T2FIT_E_INVALID, "t2fit_dict_match_dev: n_vox is negative");
  if (misaligned(y_dev, 4) || misaligned(index_dev, 4) || misaligned(scale_dev, 4) || misaligned(rmse_dev, 4))
    return fail(T2FIT_E_INVALID, "t2fit_dict_match_dev: y_dev, index_dev, scale_dev and rmse_dev must be aligned to 4 bytes");
  if (misaligned(packed_dev, 16)) return fail(T2FIT_E_INVALID, "t2fit_dict_match_dev: packed_dev must be aligned to 16 bytes");
  if (n_vox == 0) return T2FIT_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  DictHeader h;
  T2_HIP(hipMemcpyAsync(&h, packed_dev, sizeof(h), hipMemcpyDeviceToHost, st));
  T2_HIP(hipStreamSynchronize(st));
  if (h.magic != kMagic) return fail(T2FIT_E_INVALID, "t2fit_dict_match_dev: packed_dev does not hold a packed dictionary (magic)");
  if (h.n_te != n_te)
    return fail(T2FIT_E_INVALID, "t2fit_dict_match_dev: the dictionary was packed for n_te " + std::to_string(h.n_te) + ", the call has " +
                                     std::to_string(n_te));
  if (!sizes_ok(h.n_atoms, h.n_te)) return fail(T2FIT_E_INVALID, "t2fit_dict_match_dev: the dictionary header has sizes out of range");
  const DictHeader want = header_for(h.n_atoms, h.n_te);
  if (h.k_pad != want.k_pad || h.n_tiles != want.n_tiles || h.off_tiles != want.off_tiles || h.off_atoms != want.off_atoms ||
      h.off_norm2 != want.off_norm2 || h.bytes != want.bytes || !(h.dmax > 0.0f) || !std::isfinite(h.dmax))
    return fail(T2FIT_E_INVALID, "t2fit_dict_match_dev: the dictionary header is not what t2fit_dict_pack_host writes");
  const unsigned char* packed = static_cast<const unsigned char*>(packed_dev);
  hipError_t e = hipSuccess;
  switch (h.k_pad / 2) {
#define T2_DICT_CASE(KS) \
  case KS: e = launch<KS>(y_dev, n_te, n_vox, mask_dev, packed, index_dev, scale_dev, rmse_dev, st); break;
    T2_DICT_CASE(1) T2_DICT_CASE(2) T2_DICT_CASE(3) T2_DICT_CASE(4) T2_DICT_CASE(5) T2_DICT_CASE(6) T2_DICT_CASE(7) T2_DICT_CASE(8)
    T2_DICT_CASE(9) T2_DICT_CASE(10) T2_DICT_CASE(11) T2_DICT_CASE(12) T2_DICT_CASE(13) T2_DICT_CASE(14) T2_DICT_CASE(15) T2_DICT_CASE(16)
#undef T2_DICT_CASE
    default: return fail(T2FIT_E_INVALID, "t2fit_dict_match_dev: k_pad out of range");
  }
  T2_HIP(e);
  return T2FIT_OK;
}

}  // extern "C"

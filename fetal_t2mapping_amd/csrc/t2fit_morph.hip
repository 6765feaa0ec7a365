// t2fit_morph.hip -- gfx950 kernels and C ABI of the mask and phantom-label building (include/t2fit.h:
// t2fit_morph_workspace_bytes, t2fit_binary_threshold_dev, t2fit_binary_morph_dev, t2fit_fill_holes_dev,
// t2fit_seed_labels_dev, t2fit_relabel_dev).  Replaces the host morphology of utils/qmri_utils.py: build_mask (:223-252),
// build_phantom_masks (:591-623), build_phantom_labels_v2 (:868-933), build_mask_from_labels (:935-951) and the lookup
// of convert_synthseg_to_feta (:976-1009).
//
// A binary volume is worked on bit-packed: a word holds 64 consecutive x voxels (bit i = voxel 64 w + i), a row is
// W = ceil(nx / 64) words, rows follow in (z, y) order.  The bits of the last word beyond nx (the tail) hold the border
// value of the running operation; every read of a last word puts them there again, so they never reach a result.
//
//   dilation   out[v] = OR over the element's offsets s of in[v - s], outside = border.  One thread makes one output
//              word.  For a run (dz, dy, x0, x1) it reads the words w - 1, w, w + 1 of row (z - dz, y - dy) as a 192-bit
//              window, ORs the window with itself shifted by 1, 2, 4, .. (log2 of the run length steps) and takes the 64
//              bits that start x0 below the word: exactly the OR over the run, whatever the element.
//   erosion    the exact dual: the same kernel reads complemented words, walks the reflected run list with the
//              complemented border and stores the complement.
//   fill holes the background reached from the border (face connectivity) is grown to its fixed point; see below.
// Nothing here shares a header with the fit kernels except the error plumbing and the size helpers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "t2fit_error.h"
#include "t2fit_support.h"

namespace {

using t2fit::kBlock;
using word_t = unsigned long long;

constexpr int kMaxRadius = 32;
constexpr int kMaxSize = 2 * kMaxRadius + 1;          // 65
constexpr int kMaxRuns = kMaxSize * kMaxSize * 4;     // 16900
constexpr int kMaxSeeds = 4096;
constexpr int kSweepBatch = 4;  // fill holes: sweeps queued between two reads of the flags

// the packed grid of an operation: the volume, or the volume padded by (pz, py, px) zeros on every side
struct Grid {
  int nz, ny, nx;  // of the packed grid
  int w;           // words per row
  word_t valid;    // the bits of a row's last word that are voxels
};

__host__ __device__ inline word_t valid_bits(int nx) { return (nx & 63) ? ((1ull << (nx & 63)) - 1ull) : ~0ull; }

// ---- pack / unpack ------------------------------------------------------------------------------------------------
// A wave makes one word: lane i tests voxel 64 w + i and the ballot is the word.  (pz, py, px): where voxel 0 of the
// source lies in the packed grid; packed voxels outside the source are 0, the tail is `tail`.
__global__ __launch_bounds__(kBlock) void morph_pack_kernel(const uint8_t* __restrict__ src, int sz, int sy, int sx, Grid g, int pz,
                                                            int py, int px, int tail, int64_t n_words,
                                                            word_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);  // wave-uniform
  if (wid >= n_words) return;
  const int wx = (int)(wid % g.w);
  const int64_t row = wid / g.w;
  const int y = (int)(row % g.ny), z = (int)(row / g.ny);
  const int x = wx * 64 + lane;
  const int qz = z - pz, qy = y - py, qx = x - px;
  bool on = tail != 0;
  if (x < g.nx) {
    on = false;
    if (qz >= 0 && qz < sz && qy >= 0 && qy < sy && qx >= 0 && qx < sx) on = src[((int64_t)qz * sy + qy) * sx + qx] != 0;
  }
  const word_t bits = __ballot(on);
  if (lane == 0) out[wid] = bits;
}

// out[v] = bit of packed voxel v + (pz, py, px), complemented when inv
__global__ __launch_bounds__(kBlock) void morph_unpack_kernel(const word_t* __restrict__ bits, Grid g, int pz, int py, int px, int sz,
                                                              int sy, int sx, int inv, uint8_t* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= (int64_t)sz * sy * sx) return;
  const int x = (int)(v % sx);
  const int64_t r = v / sx;
  const int y = (int)(r % sy), z = (int)(r / sy);
  const int X = x + px;
  const word_t wv = bits[((int64_t)(z + pz) * g.ny + (y + py)) * g.w + (X >> 6)];
  out[v] = (uint8_t)(((wv >> (X & 63)) & 1ull) ^ (word_t)(inv & 1));
}

template <class T>
__global__ __launch_bounds__(kBlock) void morph_threshold_kernel(const T* __restrict__ src, int64_t n, double lo, double hi,
                                                                 uint8_t* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n) return;
  const double s = (double)src[v];  // exact for float32 and int32; a NaN fails both comparisons
  out[v] = (s >= lo && s <= hi) ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void morph_relabel_kernel(const int32_t* in, int64_t n, const int32_t* __restrict__ lut, int n_lut,
                                                               int32_t* out) {  // out may be in
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n) return;
  const int32_t l = in[v];
  out[v] = (l >= 0 && l < n_lut) ? lut[l] : 0;
}

// ---- dilation by a run list -------------------------------------------------------------------------------------------
struct DilateArgs {
  const word_t* in;
  word_t* out;
  const int4* runs;  // (dz, dy, x0, x1)
  int n_runs;
  int reflect;      // walk the element reflected through its origin
  Grid g;
  word_t inv;       // all ones: the erosion (words are complemented on the way in and on the way out)
  word_t fill;      // a word outside the grid, in the dilation's polarity
  word_t tail_out;  // the tail of a stored word: the operation's own border value
  int64_t n_words;
};

// word w of row (z, y) in the dilation's polarity; outside the grid: the border
__device__ inline word_t morph_word(const DilateArgs& a, bool row_in, int64_t row_base, int w) {
  if (!row_in || w < 0 || w >= a.g.w) return a.fill;
  word_t v = a.in[row_base + w] ^ a.inv;
  if (w == a.g.w - 1) v = (v & a.g.valid) | (a.fill & ~a.g.valid);
  return v;
}

__global__ __launch_bounds__(kBlock) void morph_dilate_kernel(const DilateArgs a) {
  const int64_t wid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (wid >= a.n_words) return;
  const int wx = (int)(wid % a.g.w);
  const int64_t row = wid / a.g.w;
  const int y = (int)(row % a.g.ny), z = (int)(row / a.g.ny);
  word_t acc = 0ull;
  for (int r = 0; r < a.n_runs; ++r) {  // the run is the same for every lane: the loop below is wave-uniform
    const int4 run = a.runs[r];
    const int x0 = a.reflect ? -run.w : run.z, x1 = a.reflect ? -run.z : run.w;
    const int sz = a.reflect ? z + run.x : z - run.x, sy = a.reflect ? y + run.y : y - run.y;
    const bool row_in = sz >= 0 && sz < a.g.nz && sy >= 0 && sy < a.g.ny;
    const int64_t base = row_in ? ((int64_t)sz * a.g.ny + sy) * a.g.w : 0;
    // window bit 64 + i is voxel i of this word; out bit i = OR of window bits 64 + i - x1 .. 64 + i - x0
    word_t lo = x1 > 0 ? morph_word(a, row_in, base, wx - 1) : 0ull;
    word_t mid = morph_word(a, row_in, base, wx);
    word_t hi = x0 < 0 ? morph_word(a, row_in, base, wx + 1) : 0ull;
    const int len = x1 - x0 + 1;
    for (int c = 1; c < len;) {  // D |= D << s doubles the span covered below each bit
      const int s = c < len - c ? c : len - c;  // 1..32
      hi |= (hi << s) | (mid >> (64 - s));
      mid |= (mid << s) | (lo >> (64 - s));
      lo |= lo << s;
      c += s;
    }
    const int p = 64 - x0;  // 32..96: the 64 bits from window bit p
    word_t got;
    if (p == 64) got = mid;
    else if (p < 64) got = (lo >> p) | (mid << (64 - p));
    else got = (mid >> (p - 64)) | (hi << (128 - p));
    acc |= got;
  }
  acc ^= a.inv;
  if (wx == a.g.w - 1) acc = (acc & a.g.valid) | (a.tail_out & ~a.g.valid);
  a.out[wid] = acc;
}

// ---- fill holes ---------------------------------------------------------------------------------------------------------
// free = background, reached = the part of it connected to the border.  A workgroup owns a tile of 8 x 8 rows by 4 words
// (256 voxels of x), stages the reached words of tile + halo in LDS and grows them to the tile's fixed point: a word takes
// its (z, y) neighbours' bits and the edge bits of its x neighbours, masked by free, and floods them along x inside the
// word with one add per direction (adding a seed bit to a run of ones carries through the run).  A sweep reads one
// buffer and writes the other (the result of a sweep does not depend on the order the tiles ran in); a tile whose words
// changed raises the sweep's flag.  The reached set only grows and its fixed point is unique, so the loop over sweeps
// ends, and the result and the number of sweeps are functions of the input alone.
constexpr int kFZ = 8, kFY = 8, kFW = 4;
constexpr int kHZ = kFZ + 2, kHY = kFY + 2, kHW = kFW + 2;
static_assert(kFZ * kFY * kFW == kBlock, "one thread per word of the tile");

constexpr int kPropZ = 1, kPropY = 2, kPropX = 4;  // the axes the flood crosses

// free and the border seeds from the packed mask (in place: mask -> free)
__global__ __launch_bounds__(kBlock) void morph_fill_init_kernel(word_t* __restrict__ mask_free, word_t* __restrict__ reached, Grid g,
                                                                 int prop, int64_t n_words) {
  const int64_t wid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (wid >= n_words) return;
  const int wx = (int)(wid % g.w);
  const int64_t row = wid / g.w;
  const int y = (int)(row % g.ny), z = (int)(row / g.ny);
  const word_t valid = wx == g.w - 1 ? g.valid : ~0ull;
  const word_t fr = ~mask_free[wid] & valid;
  word_t seed = 0ull;
  if ((prop & kPropZ) && (z == 0 || z == g.nz - 1)) seed = ~0ull;
  if ((prop & kPropY) && (y == 0 || y == g.ny - 1)) seed = ~0ull;
  if (prop & kPropX) {
    if (wx == 0) seed |= 1ull;
    if (wx == g.w - 1) seed |= 1ull << ((g.nx - 1) & 63);
  }
  mask_free[wid] = fr;
  reached[wid] = fr & seed;
}

// the bits of `fr` connected to a bit of `seed` (a subset of fr) through ones of fr towards higher bits, seeds included
__device__ inline word_t morph_flood_up(word_t seed, word_t fr) { return (fr & ~(fr + seed)) | seed; }

__global__ __launch_bounds__(kBlock) void morph_fill_sweep_kernel(const word_t* __restrict__ fr_all, const word_t* __restrict__ src,
                                                                  word_t* __restrict__ dst, Grid g, int prop, int tiles_w, int tiles_y,
                                                                  const int* __restrict__ prev_flag, int* __restrict__ flag) {
  __shared__ word_t R[kHZ * kHY * kHW];
  if (prev_flag && *prev_flag == 0) return;  // the sweep before changed nothing: both buffers hold the fixed point
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int bw = b % tiles_w;
  b /= tiles_w;
  const int by = b % tiles_y, bz = b / tiles_y;
  const int w0 = bw * kFW, y0 = by * kFY, z0 = bz * kFZ;
  for (int i = tid; i < kHZ * kHY * kHW; i += kBlock) {
    const int lw = i % kHW, ly = (i / kHW) % kHY, lz = i / (kHW * kHY);
    const int w = w0 + lw - 1, y = y0 + ly - 1, z = z0 + lz - 1;
    const bool in = w >= 0 && w < g.w && y >= 0 && y < g.ny && z >= 0 && z < g.nz;
    R[i] = in ? src[((int64_t)z * g.ny + y) * g.w + w] : 0ull;
  }
  const int tw = tid % kFW, ty = (tid / kFW) % kFY, tz = tid / (kFW * kFY);
  const int w = w0 + tw, y = y0 + ty, z = z0 + tz;
  const bool in = w < g.w && y < g.ny && z < g.nz;
  const int64_t at = in ? ((int64_t)z * g.ny + y) * g.w + w : 0;
  const word_t fr = in ? fr_all[at] : 0ull;
  const int me = ((tz + 1) * kHY + (ty + 1)) * kHW + (tw + 1);
  __syncthreads();
  const word_t r0 = R[me];
  word_t r = r0;
  for (;;) {
    word_t s = r;
    if (prop & kPropZ) s |= R[me - kHY * kHW] | R[me + kHY * kHW];
    if (prop & kPropY) s |= R[me - kHW] | R[me + kHW];
    if (prop & kPropX) s |= (R[me - 1] >> 63) | (R[me + 1] << 63);
    s &= fr;
    if (prop & kPropX) s = morph_flood_up(s, fr) | __brevll(morph_flood_up(__brevll(s), __brevll(fr)));
    const bool grew = s != r;
    if (!__syncthreads_or(grew)) break;  // (also: every read of this round is done)
    if (grew) R[me] = s;
    r = s;
    __syncthreads();
  }
  if (in) {
    dst[at] = r;
    if (r != r0) *flag = 1;
  }
}

// ---- seed labels ----------------------------------------------------------------------------------------------------------
// The element as a bitmap: row (dz + 32) * 65 + (dy + 32) holds two words, bit dx + 32 of the pair.  A thread owns a voxel
// and walks the seeds.
struct Seed { int x, y, z, label; };

template <class T>
__global__ __launch_bounds__(kBlock) void morph_seed_kernel(const Seed* __restrict__ seeds, int n_seeds, const word_t* __restrict__ bitmap,
                                                            int rz, int ry, int rx, int nz, int ny, int nx, T* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= (int64_t)nz * ny * nx) return;
  const int x = (int)(v % nx);
  const int64_t r = v / nx;
  const int y = (int)(r % ny), z = (int)(r / ny);
  int best = 0;
  for (int s = 0; s < n_seeds; ++s) {
    const Seed sd = seeds[s];
    const int dz = z - sd.z, dy = y - sd.y, dx = x - sd.x;
    if (dz < -rz || dz > rz || dy < -ry || dy > ry || dx < -rx || dx > rx) continue;
    const int bit = dx + kMaxRadius;
    const word_t wv = bitmap[((dz + kMaxRadius) * kMaxSize + (dy + kMaxRadius)) * 2 + (bit >> 6)];
    if (((wv >> (bit & 63)) & 1ull) && sd.label > best) best = sd.label;
  }
  out[v] = (T)best;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
using namespace t2fit;

constexpr size_t up256(size_t v) { return align_up(v, 256); }
constexpr size_t kRunBytes = up256((size_t)kMaxRuns * sizeof(int4));
constexpr size_t kBitmapBytes = up256((size_t)kMaxSize * kMaxSize * 2 * sizeof(word_t));
constexpr size_t kSeedBytes = up256((size_t)kMaxSeeds * sizeof(Seed));
constexpr size_t kFlagBytes = 256;

struct Layout {  // of the workspace
  size_t runs, bitmap, seeds, flags, packed[3], packed_bytes, total;
};

// sizes of the volume and the reach of the padding (0: none) -> the packed grid and the workspace; false: too large
bool morph_layout(int nz, int ny, int nx, int reach, Grid* g, Layout* l) {
  const int64_t pz = (int64_t)nz + 2 * reach, py = (int64_t)ny + 2 * reach, px = (int64_t)nx + 2 * reach;
  const int64_t w = (px + 63) / 64;
  const int64_t words = pz * py * w;
  if (pz * py >= (1LL << 31) || words >= (1LL << 31) || (int64_t)nz * ny * nx >= (1LL << 40)) return false;
  g->nz = (int)pz; g->ny = (int)py; g->nx = (int)px; g->w = (int)w;
  g->valid = valid_bits((int)px);
  l->packed_bytes = up256((size_t)words * sizeof(word_t));
  l->runs = 0;
  l->bitmap = l->runs + kRunBytes;
  l->seeds = l->bitmap + kBitmapBytes;
  l->flags = l->seeds + kSeedBytes;
  l->packed[0] = l->flags + kFlagBytes;
  l->packed[1] = l->packed[0] + l->packed_bytes;
  l->packed[2] = l->packed[1] + l->packed_bytes;
  l->total = l->packed[2] + l->packed_bytes;
  return true;
}

// the checks every entry point with a volume shares; `who` starts the message
int check_volume(const char* who, int nz, int ny, int nx) {
  if (nz < 1 || ny < 1 || nx < 1) return fail(T2FIT_E_INVALID, std::string(who) + ": nz, ny, nx must be positive");
  return T2FIT_OK;
}

int check_workspace(const char* who, const void* ws, size_t have, size_t need) {
  if (!ws) return fail(T2FIT_E_INVALID, std::string(who) + ": workspace_dev is NULL");
  if (reinterpret_cast<uintptr_t>(ws) & 255u) return fail(T2FIT_E_INVALID, std::string(who) + ": workspace_dev is not aligned to 256 bytes");
  if (have < need)
    return fail(T2FIT_E_INVALID, std::string(who) + ": the workspace has " + std::to_string(have) + " bytes, the call needs " +
                                     std::to_string(need) + " (t2fit_morph_workspace_bytes)");
  return T2FIT_OK;
}

// element: size[3] = (sz, sy, sx) of the footprint, odd and <= 65; runs inside it
int check_element(const char* who, const int32_t* size, const int32_t* runs, int n_runs) {
  const std::string w(who);
  if (!size || !runs) return fail(T2FIT_E_INVALID, w + ": size / runs is NULL");
  for (int a = 0; a < 3; ++a) {
    if (size[a] < 1) return fail(T2FIT_E_INVALID, w + ": a footprint size is below 1");
    if (size[a] % 2 == 0) return fail(T2FIT_E_INVALID, w + ": footprint sizes must be odd (the origin is the centre), got an even one");
    if (size[a] > kMaxSize) return fail(T2FIT_E_INVALID, w + ": the footprint's radius exceeds 32");
  }
  if (n_runs < 1 || n_runs > kMaxRuns) return fail(T2FIT_E_INVALID, w + ": n_runs outside 1..16900");
  const int rz = size[0] / 2, ry = size[1] / 2, rx = size[2] / 2;
  for (int r = 0; r < n_runs; ++r) {
    const int32_t* q = runs + 4 * r;
    if (q[0] < -rz || q[0] > rz || q[1] < -ry || q[1] > ry || q[2] < -rx || q[3] > rx || q[2] > q[3])
      return fail(T2FIT_E_INVALID, w + ": run " + std::to_string(r) + " is empty or leaves the footprint");
  }
  return T2FIT_OK;
}

unsigned blocks_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// the flags of the sweeps come back through pinned memory: one small buffer per host thread, kept
int* pinned_flags() {
  thread_local int* p = nullptr;
  if (!p && hipHostMalloc(reinterpret_cast<void**>(&p), kSweepBatch * sizeof(int), hipHostMallocDefault) != hipSuccess) p = nullptr;
  return p;
}

}  // namespace

extern "C" {

int t2fit_morph_workspace_bytes(int nz, int ny, int nx, int reach, size_t* bytes) {
  if (!bytes) return fail(T2FIT_E_INVALID, "t2fit_morph_workspace_bytes: bytes is NULL");
  if (int rc = check_volume("t2fit_morph_workspace_bytes", nz, ny, nx)) return rc;
  if (reach < 0 || reach > 8 * kMaxRadius) return fail(T2FIT_E_INVALID, "t2fit_morph_workspace_bytes: reach outside 0..256");
  Grid g;
  Layout l;
  if (!morph_layout(nz, ny, nx, reach, &g, &l)) return fail(T2FIT_E_INVALID, "t2fit_morph_workspace_bytes: the volume is too large");
  *bytes = l.total;
  return T2FIT_OK;
}

int t2fit_binary_threshold_dev(const void* src_dev, int src_type, int64_t n_vox, double lo, double hi, uint8_t* out_dev, void* stream) {
  if (!src_dev || !out_dev) return fail(T2FIT_E_INVALID, "t2fit_binary_threshold_dev: src_dev / out_dev is NULL");
  if (src_type != T2FIT_MORPH_F32 && src_type != T2FIT_MORPH_I32)
    return fail(T2FIT_E_INVALID, "t2fit_binary_threshold_dev: src_type must be T2FIT_MORPH_F32 or T2FIT_MORPH_I32");
  if (n_vox < 1 || n_vox >= (1LL << 39)) return fail(T2FIT_E_INVALID, "t2fit_binary_threshold_dev: n_vox outside 1..2^39-1");
  if (std::isnan(lo) || std::isnan(hi)) return fail(T2FIT_E_INVALID, "t2fit_binary_threshold_dev: lo / hi is NaN");
  if (reinterpret_cast<uintptr_t>(src_dev) & 3u) return fail(T2FIT_E_INVALID, "t2fit_binary_threshold_dev: src_dev is not aligned to 4 bytes");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(blocks_for(n_vox, kBlock));
  if (src_type == T2FIT_MORPH_F32)
    hipLaunchKernelGGL(morph_threshold_kernel<float>, grid, dim3(kBlock), 0, st, (const float*)src_dev, n_vox, lo, hi, out_dev);
  else
    hipLaunchKernelGGL(morph_threshold_kernel<int32_t>, grid, dim3(kBlock), 0, st, (const int32_t*)src_dev, n_vox, lo, hi, out_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_binary_morph_dev(int op, const uint8_t* in_dev, uint8_t* out_dev, int nz, int ny, int nx, const int32_t* size,
                           const int32_t* runs, int n_runs, int iterations, int border_value, int flags, void* workspace_dev,
                           size_t workspace_bytes, void* stream) {
  const char* who = "t2fit_binary_morph_dev";
  if (!in_dev || !out_dev) return fail(T2FIT_E_INVALID, "t2fit_binary_morph_dev: in_dev / out_dev is NULL");
  if (op != T2FIT_MORPH_DILATE && op != T2FIT_MORPH_ERODE && op != T2FIT_MORPH_CLOSE && op != T2FIT_MORPH_OPEN)
    return fail(T2FIT_E_INVALID, "t2fit_binary_morph_dev: unknown op");
  if (int rc = check_volume(who, nz, ny, nx)) return rc;
  if (int rc = check_element(who, size, runs, n_runs)) return rc;
  if (iterations < 1 || iterations > 8) return fail(T2FIT_E_INVALID, "t2fit_binary_morph_dev: iterations outside 1..8");
  if (border_value != 0 && border_value != 1) return fail(T2FIT_E_INVALID, "t2fit_binary_morph_dev: border_value must be 0 or 1");
  if (flags & ~T2FIT_MORPH_UNBOUNDED) return fail(T2FIT_E_INVALID, "t2fit_binary_morph_dev: undefined flags");
  const bool unbounded = (flags & T2FIT_MORPH_UNBOUNDED) != 0;
  if (unbounded && op != T2FIT_MORPH_CLOSE && op != T2FIT_MORPH_OPEN)
    return fail(T2FIT_E_INVALID, "t2fit_binary_morph_dev: T2FIT_MORPH_UNBOUNDED goes with close / open");
  if (unbounded && border_value != 0)
    return fail(T2FIT_E_INVALID, "t2fit_binary_morph_dev: the unbounded-domain form has zeros outside: border_value must be 0");
  const int radius = std::max(size[0], std::max(size[1], size[2])) / 2;
  const int reach = unbounded ? radius * iterations : 0;
  Grid g;
  Layout l;
  if (!morph_layout(nz, ny, nx, reach, &g, &l)) return fail(T2FIT_E_INVALID, "t2fit_binary_morph_dev: the volume is too large");
  if (int rc = check_workspace(who, workspace_dev, workspace_bytes, l.total)) return rc;

  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace_dev);
  T2_HIP(hipMemcpyAsync(ws + l.runs, runs, (size_t)n_runs * sizeof(int4), hipMemcpyHostToDevice, st));
  T2_HIP(hipStreamSynchronize(st));  // the caller's run list has been read when the call returns

  word_t* buf[2] = {reinterpret_cast<word_t*>(ws + l.packed[0]), reinterpret_cast<word_t*>(ws + l.packed[1])};
  const int64_t n_words = (int64_t)g.nz * g.ny * g.w;
  const int64_t n_vox = (int64_t)nz * ny * nx;
  hipLaunchKernelGGL(morph_pack_kernel, dim3(blocks_for(n_words, kBlock / 64)), dim3(kBlock), 0, st, in_dev, nz, ny, nx, g, reach, reach,
                     reach, border_value, n_words, buf[0]);
  const bool erode_first = op == T2FIT_MORPH_ERODE || op == T2FIT_MORPH_OPEN;
  const int halves = (op == T2FIT_MORPH_CLOSE || op == T2FIT_MORPH_OPEN) ? 2 : 1;
  int cur = 0;
  for (int h = 0; h < halves; ++h) {
    const bool erode = (h == 0) == erode_first;
    DilateArgs a{};
    a.runs = reinterpret_cast<const int4*>(ws + l.runs);
    a.n_runs = n_runs;
    a.reflect = erode ? 1 : 0;
    a.g = g;
    a.inv = erode ? ~0ull : 0ull;
    a.fill = ((border_value != 0) != erode) ? ~0ull : 0ull;
    a.tail_out = border_value ? ~0ull : 0ull;
    a.n_words = n_words;
    for (int it = 0; it < iterations; ++it) {
      a.in = buf[cur];
      a.out = buf[cur ^ 1];
      hipLaunchKernelGGL(morph_dilate_kernel, dim3(blocks_for(n_words, kBlock)), dim3(kBlock), 0, st, a);
      cur ^= 1;
    }
  }
  hipLaunchKernelGGL(morph_unpack_kernel, dim3(blocks_for(n_vox, kBlock)), dim3(kBlock), 0, st, (const word_t*)buf[cur], g, reach, reach,
                     reach, nz, ny, nx, 0, out_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_fill_holes_dev(const uint8_t* in_dev, uint8_t* out_dev, int nz, int ny, int nx, int slice_axis, void* workspace_dev,
                         size_t workspace_bytes, int32_t* n_sweeps_out, void* stream) {
  const char* who = "t2fit_fill_holes_dev";
  if (!in_dev || !out_dev) return fail(T2FIT_E_INVALID, "t2fit_fill_holes_dev: in_dev / out_dev is NULL");
  if (int rc = check_volume(who, nz, ny, nx)) return rc;
  if (slice_axis < -1 || slice_axis > 2) return fail(T2FIT_E_INVALID, "t2fit_fill_holes_dev: slice_axis must be -1 (none), 0, 1 or 2");
  Grid g;
  Layout l;
  if (!morph_layout(nz, ny, nx, 0, &g, &l)) return fail(T2FIT_E_INVALID, "t2fit_fill_holes_dev: the volume is too large");
  if (int rc = check_workspace(who, workspace_dev, workspace_bytes, l.total)) return rc;
  const int tiles_w = ceil_div(g.w, kFW), tiles_y = ceil_div(ny, kFY);
  const int64_t tiles = (int64_t)tiles_w * tiles_y * ceil_div(nz, kFZ);
  if (tiles > 0x7fffffffLL) return fail(T2FIT_E_INVALID, "t2fit_fill_holes_dev: the volume is too large for one launch");

  hipStream_t st = (hipStream_t)stream;
  int* host_flags = pinned_flags();
  if (!host_flags) return fail(T2FIT_E_HIP, "t2fit_fill_holes_dev: no pinned memory for the sweep flags");
  char* ws = static_cast<char*>(workspace_dev);
  word_t* fr = reinterpret_cast<word_t*>(ws + l.packed[0]);
  word_t* reached[2] = {reinterpret_cast<word_t*>(ws + l.packed[1]), reinterpret_cast<word_t*>(ws + l.packed[2])};
  int* flags = reinterpret_cast<int*>(ws + l.flags);
  // axis a of the (z, y, x) array = 0: z; the flood does not cross the planes perpendicular to slice_axis
  const int prop = (slice_axis == 0 ? 0 : kPropZ) | (slice_axis == 1 ? 0 : kPropY) |
                   (slice_axis == 2 ? 0 : kPropX);
  const int64_t n_words = (int64_t)g.nz * g.ny * g.w;
  const int64_t n_vox = (int64_t)nz * ny * nx;
  hipLaunchKernelGGL(morph_pack_kernel, dim3(blocks_for(n_words, kBlock / 64)), dim3(kBlock), 0, st, in_dev, nz, ny, nx, g, 0, 0, 0, 0,
                     n_words, fr);
  hipLaunchKernelGGL(morph_fill_init_kernel, dim3(blocks_for(n_words, kBlock)), dim3(kBlock), 0, st, fr, reached[0], g, prop, n_words);
  T2_HIP(hipGetLastError());
  int cur = 0, sweeps = 0;
  for (bool done = false; !done;) {
    T2_HIP(hipMemsetAsync(flags, 0, kSweepBatch * sizeof(int), st));
    for (int k = 0; k < kSweepBatch; ++k) {
      hipLaunchKernelGGL(morph_fill_sweep_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, st, (const word_t*)fr,
                         (const word_t*)reached[cur], reached[cur ^ 1], g, prop, tiles_w, tiles_y,
                         (const int*)(k ? flags + k - 1 : nullptr), flags + k);
      cur ^= 1;
    }
    T2_HIP(hipGetLastError());
    T2_HIP(hipMemcpyAsync(host_flags, flags, kSweepBatch * sizeof(int), hipMemcpyDeviceToHost, st));
    T2_HIP(hipStreamSynchronize(st));
    int k = 0;
    while (k < kSweepBatch && host_flags[k] != 0) ++k;
    done = k < kSweepBatch;  // sweep k changed nothing; the ones after it returned at once
    sweeps += done ? k + 1 : kSweepBatch;
  }
  // (after a sweep that changed nothing both buffers hold the fixed point)
  hipLaunchKernelGGL(morph_unpack_kernel, dim3(blocks_for(n_vox, kBlock)), dim3(kBlock), 0, st, (const word_t*)reached[cur], g, 0, 0, 0, nz,
                     ny, nx, 1, out_dev);
  T2_HIP(hipGetLastError());
  if (n_sweeps_out) *n_sweeps_out = sweeps;
  return T2FIT_OK;
}

int t2fit_seed_labels_dev(const int32_t* seeds, const int32_t* labels, int n_seeds, const int32_t* size, const int32_t* runs, int n_runs,
                          int nz, int ny, int nx, void* out_dev, int out_type, void* workspace_dev, size_t workspace_bytes,
                          void* stream) {
  const char* who = "t2fit_seed_labels_dev";
  if (!seeds || !labels || !out_dev) return fail(T2FIT_E_INVALID, "t2fit_seed_labels_dev: seeds / labels / out_dev is NULL");
  if (n_seeds < 1 || n_seeds > kMaxSeeds) return fail(T2FIT_E_INVALID, "t2fit_seed_labels_dev: n_seeds outside 1..4096");
  if (int rc = check_volume(who, nz, ny, nx)) return rc;
  if (int rc = check_element(who, size, runs, n_runs)) return rc;
  if (out_type != T2FIT_MORPH_U8 && out_type != T2FIT_MORPH_I32)
    return fail(T2FIT_E_INVALID, "t2fit_seed_labels_dev: out_type must be T2FIT_MORPH_U8 or T2FIT_MORPH_I32");
  if (out_type == T2FIT_MORPH_I32 && (reinterpret_cast<uintptr_t>(out_dev) & 3u))
    return fail(T2FIT_E_INVALID, "t2fit_seed_labels_dev: out_dev is not aligned to 4 bytes");
  for (int s = 0; s < n_seeds; ++s)
    if (labels[s] < 0 || (out_type == T2FIT_MORPH_U8 && labels[s] > 255))
      return fail(T2FIT_E_INVALID, "t2fit_seed_labels_dev: label " + std::to_string(s) + " does not fit the output type");
  Grid g;
  Layout l;
  if (!morph_layout(nz, ny, nx, 0, &g, &l)) return fail(T2FIT_E_INVALID, "t2fit_seed_labels_dev: the volume is too large");
  if (int rc = check_workspace(who, workspace_dev, workspace_bytes, l.total)) return rc;

  std::vector<word_t> bitmap((size_t)kMaxSize * kMaxSize * 2, 0ull);
  for (int r = 0; r < n_runs; ++r) {
    const int32_t* q = runs + 4 * r;
    word_t* row = bitmap.data() + ((size_t)(q[0] + kMaxRadius) * kMaxSize + (q[1] + kMaxRadius)) * 2;
    for (int x = q[2]; x <= q[3]; ++x) row[(x + kMaxRadius) >> 6] |= 1ull << ((x + kMaxRadius) & 63);
  }
  std::vector<Seed> sd((size_t)n_seeds);
  for (int s = 0; s < n_seeds; ++s) sd[s] = Seed{seeds[3 * s], seeds[3 * s + 1], seeds[3 * s + 2], labels[s]};
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace_dev);
  T2_HIP(hipMemcpyAsync(ws + l.bitmap, bitmap.data(), bitmap.size() * sizeof(word_t), hipMemcpyHostToDevice, st));
  T2_HIP(hipMemcpyAsync(ws + l.seeds, sd.data(), sd.size() * sizeof(Seed), hipMemcpyHostToDevice, st));
  T2_HIP(hipStreamSynchronize(st));  // the vectors go out of scope with the call
  const int64_t n_vox = (int64_t)nz * ny * nx;
  const dim3 grid(blocks_for(n_vox, kBlock));
  const Seed* sdev = reinterpret_cast<const Seed*>(ws + l.seeds);
  const word_t* bdev = reinterpret_cast<const word_t*>(ws + l.bitmap);
  if (out_type == T2FIT_MORPH_U8)
    hipLaunchKernelGGL(morph_seed_kernel<uint8_t>, grid, dim3(kBlock), 0, st, sdev, n_seeds, bdev, size[0] / 2, size[1] / 2, size[2] / 2,
                       nz, ny, nx, (uint8_t*)out_dev);
  else
    hipLaunchKernelGGL(morph_seed_kernel<int32_t>, grid, dim3(kBlock), 0, st, sdev, n_seeds, bdev, size[0] / 2, size[1] / 2, size[2] / 2,
                       nz, ny, nx, (int32_t*)out_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_relabel_dev(const int32_t* in_dev, int64_t n_vox, const int32_t* lut_dev, int n_lut, int32_t* out_dev, void* stream) {
  if (!in_dev || !lut_dev || !out_dev) return fail(T2FIT_E_INVALID, "t2fit_relabel_dev: in_dev / lut_dev / out_dev is NULL");
  if (n_vox < 1 || n_vox >= (1LL << 39)) return fail(T2FIT_E_INVALID, "t2fit_relabel_dev: n_vox outside 1..2^39-1");
  if (n_lut < 1) return fail(T2FIT_E_INVALID, "t2fit_relabel_dev: n_lut must be positive");
  hipLaunchKernelGGL(morph_relabel_kernel, dim3(blocks_for(n_vox, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, in_dev, n_vox, lut_dev,
                     n_lut, out_dev);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

}  // extern "C"

// t2fit_components.hip -- gfx950 kernels and C ABI of the connected-component labelling (include/t2fit.h:
// t2fit_components_workspace_bytes, t2fit_components_label_dev, t2fit_components_stats_dev, t2fit_components_lut_dev).
// fetal_t2mapping_amd/_components.py states every result in numpy; everything here is integer arithmetic and the
// device results equal the statement in every element.
//
// Labelling is a union-find over the voxels' linear indices v = (z ny + y) nx + x, with `labels` itself as the parent
// array.  The one invariant: a parent is never larger than its child.  A union finds both roots and hangs the LARGER
// under the smaller with an atomic minimum, so the invariant holds whatever order the unions ran in, every root is the
// smallest index of its set, and every loop below strictly decreases an integer (its bound is written into the loop).
// No wave ever waits for another: there is no spin, no flag, no barrier between workgroups; the phases are kernels.
//   local     a workgroup owns a tile of kTZ x kTY x kTX voxels, stages its values in LDS and runs the union-find on
//             tile-local indices (a tile row is one wave: the x-runs come from one ballot, so only (z, y)
//             neighbours cost a union), then writes the global index of every voxel's tile-local root (background: -1)
//   border    every voxel on a tile face unites with those of its lower neighbours that lie in another tile
//   compress  labels[v] = find(v); the roots (labels[v] == v) are counted per chunk of 1024 voxels
//   number    exclusive scan of the counts, the roots take -(rank + 2), everything else reads its root's rank, the roots
//             are decoded: labels = rank + 1, the components numbered by their first voxel
// "Lower" neighbours are the 3 / 9 / 13 of the 6 / 18 / 26 whose linear index is smaller.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <string>

#include "t2fit_error.h"
#include "t2fit_support.h"

namespace {

using t2fit::kBlock;
using u64 = unsigned long long;

constexpr int kTZ = T2FIT_COMPONENTS_TILE_Z, kTY = T2FIT_COMPONENTS_TILE_Y, kTX = T2FIT_COMPONENTS_TILE_X;
constexpr int kRows = kTZ * kTY;            // 32 rows of 64 voxels
constexpr int kTileVox = kRows * kTX;       // 2048
constexpr int kRowsPerPass = kBlock / kTX;  // 4: a wave takes one row per pass
constexpr int kPasses = kRows / kRowsPerPass;
static_assert(kTX == 64, "a tile row is one wave");
static_assert(kRows % kRowsPerPass == 0, "whole passes");

constexpr int kChunk = 1024;  // voxels (or table entries) per workgroup of the linear kernels
constexpr int kChunkItems = kChunk / kBlock;
constexpr int kStatMinPieces = 16;   // 64-voxel pieces a wave of the statistics walks at the least
constexpr int kStatMaxBlocks = 1024;  // workgroups of the statistics at the most: the atomics on a row grow with the waves

#define CC_RELAXED __ATOMIC_RELAXED
constexpr int kWg = __HIP_MEMORY_SCOPE_WORKGROUP, kAgent = __HIP_MEMORY_SCOPE_AGENT;

// ---- union-find ---------------------------------------------------------------------------------------------------
// p[x] <= x for every x of the foreground; `bound`: the length of p.  The walk visits strictly decreasing indices, so it
// reaches a root in fewer than `bound` hops: the loop cannot run out, and the count is there to make that visible, not as a
// budget (a chain is in practice a few tiles long; were the count ever exhausted, the invariant would already be broken).
template <int Scope>
__device__ inline int uf_find(int* p, int x, int bound) {
  for (int hop = 0; hop < bound; ++hop) {
    const int q = __hip_atomic_load(p + x, CC_RELAXED, Scope);
    if (q == x) break;
    x = q;
  }
  return x;
}

// One set from the sets of a and b.  a + b falls with every turn of the loop.  When the minimum finds that a is no
// longer a root (another wave hung it under `old` first), a may now point at b instead of old: the union goes on with
// (old, b), which puts back whatever link the minimum replaced.  max(a, b) cannot rise and a + b falls by at least one per
// turn, so 2 * bound turns cannot be used up either; the loop leaves through one of its two returns.
template <int Scope>
__device__ inline void uf_unite(int* p, int a, int b, int bound) {
  for (int64_t turn = 0; turn < 2 * (int64_t)bound; ++turn) {
    a = uf_find<Scope>(p, a, bound);
    b = uf_find<Scope>(p, b, bound);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(p + a, b, CC_RELAXED, Scope);
    if (old == a) return;
    a = old;
  }
}

// The links of a foreground voxel of value v towards its lower neighbours other than (0, 0, -1).  get(dz, dy, dx): the
// neighbour's value (0: none); link(dz, dy, dx): unite with it; left_same: (0, 0, -1) holds v and lies in the same tile.
// Per row (dz, dy) of the neighbourhood: when its centre holds v the centre alone is linked (its x neighbours hang on
// it through their run), and not even that when the voxel to the left and the one left of the centre hold v too: the
// left voxel then makes the same link.  The diagonals are linked only past a centre that does not hold v.
template <class Get, class Link>
__device__ inline void lower_links(int conn, int v, bool left_same, Get get, Link link) {
  for (int dz = -1; dz <= 0; ++dz)
    for (int dy = -1; dy <= (dz ? 1 : -1); ++dy) {
      const int d = (dz != 0) + (dy != 0);
      if (d > conn) continue;
      if (get(dz, dy, 0) == v) {
        if (!(left_same && get(dz, dy, -1) == v)) link(dz, dy, 0);
        continue;
      }
      if (d + 1 > conn) continue;
      if (get(dz, dy, -1) == v) link(dz, dy, -1);
      if (get(dz, dy, 1) == v) link(dz, dy, 1);
    }
}

template <class T> __device__ inline int cc_value(T s);
template <> __device__ inline int cc_value<uint8_t>(uint8_t s) { return s != 0; }
template <> __device__ inline int cc_value<int32_t>(int32_t s) { return s; }

struct Tiling { int nz, ny, nx, tiles_x, tiles_y; };

// ---- local ----------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(kBlock) void cc_local_kernel(const T* __restrict__ in, Tiling g, int conn, int32_t* __restrict__ labels) {
  __shared__ int val[kTileVox];
  __shared__ int par[kTileVox];
  const int tid = threadIdx.x, lane = tid & 63;
  int b = blockIdx.x;
  const int bx = b % g.tiles_x;
  b /= g.tiles_x;
  const int by = b % g.tiles_y, bz = b / g.tiles_y;
  const int x0 = bx * kTX, y0 = by * kTY, z0 = bz * kTZ;
  const int x = x0 + lane;
  for (int k = 0; k < kPasses; ++k) {  // (every lane of the wave runs the ballot)
    const int row = (tid >> 6) + kRowsPerPass * k;
    const int y = y0 + row % kTY, z = z0 + row / kTY;
    const bool in_vol = x < g.nx && y < g.ny && z < g.nz;
    const int v = in_vol ? cc_value<T>(in[((int64_t)z * g.ny + y) * g.nx + x]) : 0;
    const int left = __shfl_up(v, 1);
    const bool same = lane > 0 && v != 0 && left == v;
    const u64 starts = ~__ballot(same);  // bit 0 is always set
    const u64 upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const int start = 63 - __clzll((long long)(starts & upto));
    val[row * kTX + lane] = v;
    par[row * kTX + lane] = row * kTX + start;  // the head of the voxel's x-run
  }
  __syncthreads();
  for (int k = 0; k < kPasses; ++k) {
    const int row = (tid >> 6) + kRowsPerPass * k;
    const int ly = row % kTY, lz = row / kTY;
    const int li = row * kTX + lane;
    const int v = val[li];
    if (v == 0) continue;
    const bool left_same = lane > 0 && val[li - 1] == v;
    auto at = [&](int dz, int dy, int dx) { return li + (dz * kTY + dy) * kTX + dx; };
    auto get = [&](int dz, int dy, int dx) {
      const bool in_tile = lz + dz >= 0 && ly + dy >= 0 && ly + dy < kTY && lane + dx >= 0 && lane + dx < kTX;
      return in_tile ? val[at(dz, dy, dx)] : 0;
    };
    auto link = [&](int dz, int dy, int dx) { uf_unite<kWg>(par, li, at(dz, dy, dx), kTileVox); };
    lower_links(conn, v, left_same, get, link);
  }
  __syncthreads();
  for (int k = 0; k < kPasses; ++k) {
    const int row = (tid >> 6) + kRowsPerPass * k;
    const int y = y0 + row % kTY, z = z0 + row / kTY;
    if (!(x < g.nx && y < g.ny && z < g.nz)) continue;
    const int li = row * kTX + lane;
    int32_t out = -1;
    if (val[li] != 0) {
      const int r = uf_find<kWg>(par, li, kTileVox);
      const int rrow = r / kTX;
      out = (int32_t)(((int64_t)(z0 + rrow / kTY) * g.ny + (y0 + rrow % kTY)) * g.nx + (x0 + r % kTX));
    }
    labels[((int64_t)z * g.ny + y) * g.nx + x] = out;
  }
}

// ---- border -----------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(kBlock) void cc_border_kernel(const T* __restrict__ in, Tiling g, int conn, int n_vox, int32_t* labels) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_vox) return;
  const int me = (int)i;
  const int x = me % g.nx, r = me / g.nx;
  const int y = r % g.ny, z = r / g.ny;
  const int lx = x % kTX, ly = y % kTY, lz = z % kTZ;
  if (lx > 0 && lx < kTX - 1 && ly > 0 && ly < kTY - 1 && lz > 0) return;  // every lower neighbour is in the tile
  const int v = cc_value<T>(in[me]);
  if (v == 0) return;
  auto at = [&](int dz, int dy, int dx) { return (int)(me + ((int64_t)dz * g.ny + dy) * g.nx + dx); };
  auto get = [&](int dz, int dy, int dx) {
    const bool in_vol = z + dz >= 0 && y + dy >= 0 && y + dy < g.ny && x + dx >= 0 && x + dx < g.nx;
    return in_vol ? cc_value<T>(in[at(dz, dy, dx)]) : 0;
  };
  auto link = [&](int dz, int dy, int dx) {  // (a link inside the tile was the local phase's)
    const bool other = lz + dz < 0 || ly + dy < 0 || ly + dy >= kTY || lx + dx < 0 || lx + dx >= kTX;
    if (other) uf_unite<kAgent>(labels, me, at(dz, dy, dx), n_vox);
  };
  if (lx == 0 && get(0, 0, -1) == v) link(0, 0, -1);
  const bool left_same = lx > 0 && get(0, 0, -1) == v;
  lower_links(conn, v, left_same, get, link);
}

// ---- compress, number ---------------------------------------------------------------------------------------------------
__device__ inline int block_sum(int c, int* wave_sum) {  // wave_sum: kBlock / 64 ints of LDS
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = c;
  __syncthreads();
  int s = 0;
  for (int w = 0; w < kBlock / 64; ++w) s += wave_sum[w];
  return s;
}

__global__ __launch_bounds__(kBlock) void cc_compress_kernel(int32_t* labels, int n_vox, int32_t* __restrict__ counts) {
  __shared__ int wave_sum[kBlock / 64];
  int c = 0;
  for (int j = 0; j < kChunkItems; ++j) {
    const int64_t i = (int64_t)blockIdx.x * kChunk + j * kBlock + threadIdx.x;
    if (i >= n_vox) continue;
    const int l = labels[i];
    if (l < 0) continue;
    // (a voxel read on the way may be rewritten meanwhile: by its own root or an ancestor, both of its set)
    const int root = uf_find<kAgent>(labels, l, n_vox);
    if (root != l) __hip_atomic_store(labels + i, root, CC_RELAXED, kAgent);
    c += root == (int)i;
  }
  const int s = block_sum(c, wave_sum);
  if (threadIdx.x == 0) counts[blockIdx.x] = s;
}

// counts -> their exclusive prefix sums, in place; the total to total_out[0].  One workgroup, a fixed order.
__global__ __launch_bounds__(1024) void cc_scan_kernel(int32_t* counts, int64_t n_counts, int32_t* total_out) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const int64_t per = (n_counts + 1023) / 1024;
  const int64_t lo = (int64_t)t * per < n_counts ? (int64_t)t * per : n_counts;
  const int64_t hi = lo + per < n_counts ? lo + per : n_counts;
  int s = 0;
  for (int64_t i = lo; i < hi; ++i) s += counts[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int add = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int run = t == 0 ? 0 : part[t - 1];
  for (int64_t i = lo; i < hi; ++i) {
    const int c = counts[i];
    counts[i] = run;
    run += c;
  }
  if (t == 1023) total_out[0] = part[1023];
}

// the rank of item (j, tid) of a chunk among the chunk's flagged items, in ascending index j * kBlock + tid
struct ChunkRanks {
  int before[kChunkItems];
  __device__ ChunkRanks(const bool (&flag)[kChunkItems], int (*wave_sum)[kBlock / 64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = 0; j < kChunkItems; ++j) {
      const u64 bits = __ballot(flag[j]);
      if (lane == 0) wave_sum[j][wave] = __popcll(bits);
      before[j] = __popcll(bits & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    for (int j = 0; j < kChunkItems; ++j)
      for (int q = 0; q < j * (kBlock / 64) + wave; ++q) before[j] += wave_sum[q / (kBlock / 64)][q % (kBlock / 64)];
  }
};

__global__ __launch_bounds__(kBlock) void cc_encode_kernel(int32_t* labels, int n_vox, const int32_t* __restrict__ offsets) {
  __shared__ int wave_sum[kChunkItems][kBlock / 64];
  bool root[kChunkItems];
  for (int j = 0; j < kChunkItems; ++j) {
    const int64_t i = (int64_t)blockIdx.x * kChunk + j * kBlock + threadIdx.x;
    root[j] = i < n_vox && labels[i] == (int)i;
  }
  const ChunkRanks ranks(root, wave_sum);
  const int base = offsets[blockIdx.x];
  for (int j = 0; j < kChunkItems; ++j)
    if (root[j]) labels[(int64_t)blockIdx.x * kChunk + j * kBlock + threadIdx.x] = -(base + ranks.before[j]) - 2;
}

// a voxel that is not a root holds its root's index (>= 0) and nobody reads it; the roots hold -(rank + 2)
__global__ __launch_bounds__(kBlock) void cc_resolve_kernel(int32_t* labels, int n_vox) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_vox) return;
  const int l = labels[i];
  if (l == -1) labels[i] = 0;
  else if (l >= 0) labels[i] = -labels[l] - 1;
}

__global__ __launch_bounds__(kBlock) void cc_decode_kernel(int32_t* labels, int n_vox) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_vox) return;
  const int l = labels[i];
  if (l < -1) labels[i] = -l - 1;
}

// ---- statistics ---------------------------------------------------------------------------------------------------------
struct Tables { int64_t* sizes; int32_t* bbox; int64_t* sums; };

struct Stat {
  int c;
  int64_t sz, sy, sx;
  int z0, y0, x0, z1, y1, x1;
  __device__ void clear() { c = 0; sz = sy = sx = 0; z0 = y0 = x0 = INT_MAX; z1 = y1 = x1 = -1; }
  __device__ void add(int z, int y, int x) {
    c += 1; sz += z; sy += y; sx += x;
    z0 = min(z0, z); y0 = min(y0, y); x0 = min(x0, x);
    z1 = max(z1, z); y1 = max(y1, y); x1 = max(x1, x);
  }
  __device__ void merge(const Stat& o) {
    c += o.c; sz += o.sz; sy += o.sy; sx += o.sx;
    z0 = min(z0, o.z0); y0 = min(y0, o.y0); x0 = min(x0, o.x0);
    z1 = max(z1, o.z1); y1 = max(y1, o.y1); x1 = max(x1, o.x1);
  }
};

__device__ inline int64_t wave_add64(int64_t v) { for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off); return v; }
__device__ inline int wave_add(int v) { for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off); return v; }
__device__ inline int wave_min(int v) { for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off)); return v; }
__device__ inline int wave_max(int v) { for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off)); return v; }

// what the lanes of the wave hold, combined, in every lane (every lane calls this); the parts nobody asked for are skipped
__device__ inline Stat stat_reduce(const Stat& s, const Tables& t) {
  Stat r;
  r.clear();
  r.c = wave_add(s.c);
  if (r.c == 0) return r;  // (the same in every lane)
  if (t.sums) { r.sz = wave_add64(s.sz); r.sy = wave_add64(s.sy); r.sx = wave_add64(s.sx); }
  if (t.bbox) {
    r.z0 = wave_min(s.z0); r.y0 = wave_min(s.y0); r.x0 = wave_min(s.x0);
    r.z1 = wave_max(s.z1); r.y1 = wave_max(s.y1); r.x1 = wave_max(s.x1);
  }
  return r;
}

// one thread adds s to the tables' row `label`.  A side of the box goes to memory only when it would move it: the
// value read may be stale, but then it is farther out than the true one, and the atomic decides.
__device__ inline void stat_commit(int label, const Stat& s, const Tables& t) {
  if (s.c == 0) return;
  if (t.sizes) atomicAdd(reinterpret_cast<u64*>(t.sizes + label), (u64)s.c);
  if (t.sums) {
    atomicAdd(reinterpret_cast<u64*>(t.sums + 3 * (int64_t)label + 0), (u64)s.sz);
    atomicAdd(reinterpret_cast<u64*>(t.sums + 3 * (int64_t)label + 1), (u64)s.sy);
    atomicAdd(reinterpret_cast<u64*>(t.sums + 3 * (int64_t)label + 2), (u64)s.sx);
  }
  if (t.bbox) {
    int32_t* bb = t.bbox + 6 * (int64_t)label;
    const int lo[3] = {s.z0, s.y0, s.x0}, hi[3] = {s.z1, s.y1, s.x1};
    for (int a = 0; a < 3; ++a) {
      if (lo[a] < __hip_atomic_load(bb + a, CC_RELAXED, kAgent)) atomicMin(bb + a, lo[a]);
      if (hi[a] > __hip_atomic_load(bb + 3 + a, CC_RELAXED, kAgent)) atomicMax(bb + 3 + a, hi[a]);
    }
  }
}

__global__ __launch_bounds__(kBlock) void cc_stats_init_kernel(int64_t n_rows, int nz, int ny, int nx, Tables t) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_rows) return;
  if (t.sizes) t.sizes[i] = 0;
  if (t.sums) t.sums[3 * i] = t.sums[3 * i + 1] = t.sums[3 * i + 2] = 0;
  if (t.bbox) {
    t.bbox[6 * i] = nz; t.bbox[6 * i + 1] = ny; t.bbox[6 * i + 2] = nx;
    t.bbox[6 * i + 3] = t.bbox[6 * i + 4] = t.bbox[6 * i + 5] = -1;
  }
}

// A wave walks `per_wave` consecutive pieces of 64 voxels.  In a piece the head of every x-run of one label (a run ends
// with the row) works out the run's sums in closed form, so only heads speak from here on.  The wave keeps two labels
// (the background and the inside of a large component, say) whose runs its lanes gather privately; they go to the tables
// once, at the end, after the waves of the workgroup have combined what they hold for the same label -- or earlier, when
// a label that the piece does not hold gives its place to one it does.  The runs of any other label are combined over
// the lanes of the piece, label by label (a label with a single run needs no combining), and go to the tables at once:
// a label costs a wave one set of atomics per piece at the most.
__global__ __launch_bounds__(kBlock) void cc_stats_kernel(const int32_t* __restrict__ labels, int ny, int nx, int n_vox, int n,
                                                          int64_t per_wave, Tables t) {
  __shared__ Stat held[2 * (kBlock / 64)];
  __shared__ int held_label[2 * (kBlock / 64)];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + wid;
  const int64_t n_pieces = ((int64_t)n_vox + 63) / 64;
  const int64_t p0 = wave * per_wave < n_pieces ? wave * per_wave : n_pieces;
  const int64_t p1 = p0 + per_wave < n_pieces ? p0 + per_wave : n_pieces;
  int cur0 = -1, cur1 = -1;
  Stat own0, own1;
  own0.clear();
  own1.clear();
  for (int64_t p = p0; p < p1; ++p) {
    const int64_t i = p * 64 + lane;
    int l = i < n_vox ? labels[i] : -1;
    if (l > n) l = -1;
    const bool valid = l >= 0;
    const int v = valid ? (int)i : 0;
    const int x = v % nx, r = v / nx;
    const int y = r % ny, z = r / ny;
    const int left = __shfl_up(l, 1);
    const bool head = valid && (lane == 0 || x == 0 || left != l);
    const u64 ends = __ballot(head || !valid) & ~(lane == 63 ? ~0ull : ((2ull << lane) - 1ull));  // above this lane
    const int c = (ends ? __ffsll((long long)ends) - 1 : 64) - lane;  // of a head: the length of its run
    Stat run;
    run.c = c; run.sz = (int64_t)c * z; run.sy = (int64_t)c * y; run.sx = (int64_t)c * x + (int64_t)c * (c - 1) / 2;
    run.z0 = run.z1 = z; run.y0 = run.y1 = y; run.x0 = x; run.x1 = x + c - 1;
    u64 rest = __ballot(head && l != cur0 && l != cur1);
    if (rest != 0) {  // (the same in every lane) a label that is not held: it takes a place this piece does not use
      const bool free0 = __ballot(head && l == cur0) == 0, free1 = __ballot(head && l == cur1) == 0;
      if (free0 || free1) {
        const bool take0 = free0 && !(cur0 >= 0 && free1 && cur1 < 0);  // an empty place before one that holds a label
        const int next = __shfl(l, __ffsll((long long)rest) - 1);
        const Stat out = stat_reduce(take0 ? own0 : own1, t);
        if (lane == 0) stat_commit(take0 ? cur0 : cur1, out, t);  // (an empty place holds nothing)
        if (take0) { cur0 = next; own0.clear(); } else { cur1 = next; own1.clear(); }
      }
    }
    if (head && l == cur0) own0.merge(run);
    else if (head && l == cur1) own1.merge(run);
    rest = __ballot(head && l != cur0 && l != cur1);
    for (int turn = 0; turn < 64 && rest != 0; ++turn) {  // a label of the piece per turn
      const int other = __shfl(l, __ffsll((long long)rest) - 1);
      const bool mine = head && l == other;
      const u64 runs = __ballot(mine);
      if (__popcll(runs) == 1) {
        if (mine) stat_commit(other, run, t);
      } else {
        Stat s;
        s.clear();
        if (mine) s = run;
        const Stat out = stat_reduce(s, t);
        if (lane == 0) stat_commit(other, out, t);
      }
      rest &= ~runs;
    }
  }
  const Stat end0 = stat_reduce(own0, t), end1 = stat_reduce(own1, t);
  if (lane == 0) {
    held[2 * wid] = end0; held_label[2 * wid] = end0.c ? cur0 : -1;
    held[2 * wid + 1] = end1; held_label[2 * wid + 1] = end1.c ? cur1 : -1;
  }
  __syncthreads();
  const int e = threadIdx.x;
  if (e >= 2 * (kBlock / 64) || held_label[e] < 0) return;
  for (int q = 0; q < e; ++q)
    if (held_label[q] == held_label[e]) return;  // the first entry of a label speaks for the others
  Stat sum = held[e];
  for (int q = e + 1; q < 2 * (kBlock / 64); ++q)
    if (held_label[q] == held_label[e]) sum.merge(held[q]);
  stat_commit(held_label[e], sum, t);
}

// ---- selection table ----------------------------------------------------------------------------------------------------
struct LutScratch {  // the head of the scratch buffer; the chunk counts follow at byte 256
  u64 best;          // max over the kept of (size << 32) | (0xffffffff - label); 0: nothing kept
  int32_t n_passing; // components inside the size limits
  int32_t n_kept;
};

__device__ inline bool lut_passes(int64_t size, int64_t min_size, int64_t max_size) {
  return size >= min_size && (max_size == 0 || size <= max_size);
}

__global__ __launch_bounds__(kBlock) void cc_lut_count_kernel(const int64_t* __restrict__ sizes, int64_t n_rows, int64_t min_size,
                                                              int64_t max_size, int largest, LutScratch* head,
                                                              int32_t* __restrict__ counts) {
  __shared__ int wave_sum[kBlock / 64];
  int c = 0;
  u64 best = 0;
  for (int j = 0; j < kChunkItems; ++j) {
    const int64_t i = (int64_t)blockIdx.x * kChunk + j * kBlock + threadIdx.x;
    if (i < 1 || i >= n_rows) continue;
    const int64_t s = sizes[i];
    if (!lut_passes(s, min_size, max_size)) continue;
    c += 1;
    const u64 clamped = s < 0 ? 0ull : s > 0xffffffffLL ? 0xffffffffull : (u64)s;  // (the sizes of a volume are below 2^31)
    const u64 key = (clamped << 32) | (u64)(0xffffffffu - (uint32_t)i);
    best = key > best ? key : best;
  }
  if (largest) {  // the lanes of a wave combine before one of them goes to memory
    for (int off = 32; off > 0; off >>= 1) {
      const u64 o = __shfl_xor(best, off);
      best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0 && best != 0) atomicMax(&head->best, best);
  }
  const int s = block_sum(c, wave_sum);
  if (threadIdx.x == 0) counts[blockIdx.x] = s;
}

__global__ __launch_bounds__(kBlock) void cc_lut_write_kernel(const int64_t* __restrict__ sizes, int64_t n_rows, int64_t min_size,
                                                              int64_t max_size, int largest, int renumber, LutScratch* head,
                                                              const int32_t* __restrict__ offsets, int32_t* __restrict__ lut) {
  __shared__ int wave_sum[kChunkItems][kBlock / 64];
  const int64_t winner = head->best ? (int64_t)(0xffffffffu - (uint32_t)(head->best & 0xffffffffu)) : 0;
  bool keep[kChunkItems];
  for (int j = 0; j < kChunkItems; ++j) {
    const int64_t i = (int64_t)blockIdx.x * kChunk + j * kBlock + threadIdx.x;
    keep[j] = i >= 1 && i < n_rows && lut_passes(sizes[i], min_size, max_size) && (!largest || i == winner);
  }
  const ChunkRanks ranks(keep, wave_sum);
  const int base = largest ? 0 : offsets[blockIdx.x];
  for (int j = 0; j < kChunkItems; ++j) {
    const int64_t i = (int64_t)blockIdx.x * kChunk + j * kBlock + threadIdx.x;
    if (i >= n_rows) continue;
    int32_t out = 0;
    if (keep[j]) out = !renumber ? (int32_t)i : largest ? 1 : base + ranks.before[j] + 1;
    lut[i] = out;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) head->n_kept = largest ? (head->best != 0) : head->n_passing;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
using namespace t2fit;

constexpr size_t kHeadBytes = 256;

unsigned blocks_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// refuses a size < 1 and 2^31 voxels or more
int check_volume(const std::string& who, int nz, int ny, int nx) {
  if (nz < 1 || ny < 1 || nx < 1) return fail(T2FIT_E_INVALID, who + ": nz, ny, nx must be positive");
  if ((int64_t)nz * ny >= (1LL << 31) || (int64_t)nz * ny * nx >= (1LL << 31))
    return fail(T2FIT_E_INVALID, who + ": the volume has 2^31 voxels or more");
  return T2FIT_OK;
}

size_t workspace_need(int64_t n_vox) { return kHeadBytes + align_up((size_t)ceil_div<int64_t>(n_vox, kChunk) * sizeof(int32_t), 256); }

// a count comes back through pinned memory: one small buffer per host thread, kept
int32_t* pinned_word() {
  thread_local int32_t* p = nullptr;
  if (!p && hipHostMalloc(reinterpret_cast<void**>(&p), 64, hipHostMallocDefault) != hipSuccess) p = nullptr;
  return p;
}

template <class T>
void launch_label(const void* in_dev, const Tiling& g, int conn, int n_vox, int32_t* labels, hipStream_t st) {
  const int64_t tiles = (int64_t)g.tiles_x * g.tiles_y * ceil_div(g.nz, kTZ);
  hipLaunchKernelGGL(cc_local_kernel<T>, dim3((unsigned)tiles), dim3(kBlock), 0, st, (const T*)in_dev, g, conn, labels);
  hipLaunchKernelGGL(cc_border_kernel<T>, dim3(blocks_for(n_vox, kBlock)), dim3(kBlock), 0, st, (const T*)in_dev, g, conn, n_vox, labels);
}

}  // namespace

extern "C" {

int t2fit_components_workspace_bytes(int nz, int ny, int nx, size_t* bytes) {
  if (!bytes) return fail(T2FIT_E_INVALID, "t2fit_components_workspace_bytes: bytes is NULL");
  if (int rc = check_volume("t2fit_components_workspace_bytes", nz, ny, nx)) return rc;
  *bytes = workspace_need((int64_t)nz * ny * nx);
  return T2FIT_OK;
}

int t2fit_components_label_dev(const void* in_dev, int in_type, int nz, int ny, int nx, int connectivity, int32_t* labels_dev,
                               int32_t* n_out, void* workspace_dev, size_t workspace_bytes, void* stream) {
  const std::string who = "t2fit_components_label_dev";
  if (!in_dev || !labels_dev) return fail(T2FIT_E_INVALID, who + ": in_dev / labels_dev is NULL");
  if (in_type != T2FIT_MORPH_U8 && in_type != T2FIT_MORPH_I32)
    return fail(T2FIT_E_INVALID, who + ": in_type must be T2FIT_MORPH_U8 or T2FIT_MORPH_I32");
  if (int rc = check_volume(who, nz, ny, nx)) return rc;
  if (connectivity < 1 || connectivity > 3) return fail(T2FIT_E_INVALID, who + ": connectivity must be 1, 2 or 3");
  if ((reinterpret_cast<uintptr_t>(labels_dev) & 3u) || (in_type == T2FIT_MORPH_I32 && (reinterpret_cast<uintptr_t>(in_dev) & 3u)))
    return fail(T2FIT_E_INVALID, who + ": an int32 volume is not aligned to 4 bytes");
  if (in_dev == (const void*)labels_dev) return fail(T2FIT_E_INVALID, who + ": labels_dev must not be in_dev");
  const int n_vox = (int)((int64_t)nz * ny * nx);
  const size_t need = workspace_need(n_vox);
  if (!workspace_dev) return fail(T2FIT_E_INVALID, who + ": workspace_dev is NULL");
  if (reinterpret_cast<uintptr_t>(workspace_dev) & 255u) return fail(T2FIT_E_INVALID, who + ": workspace_dev is not aligned to 256 bytes");
  if (workspace_bytes < need)
    return fail(T2FIT_E_INVALID, who + ": the workspace has " + std::to_string(workspace_bytes) + " bytes, the call needs " +
                                     std::to_string(need) + " (t2fit_components_workspace_bytes)");

  hipStream_t st = (hipStream_t)stream;
  int32_t* pinned = nullptr;
  if (n_out && !(pinned = pinned_word())) return fail(T2FIT_E_HIP, who + ": no pinned memory for the count");
  int32_t* total = static_cast<int32_t*>(workspace_dev);
  int32_t* counts = reinterpret_cast<int32_t*>(static_cast<char*>(workspace_dev) + kHeadBytes);
  const Tiling g{nz, ny, nx, ceil_div(nx, kTX), ceil_div(ny, kTY)};
  const int64_t n_chunks = ceil_div<int64_t>(n_vox, kChunk);
  if (in_type == T2FIT_MORPH_U8) launch_label<uint8_t>(in_dev, g, connectivity, n_vox, labels_dev, st);
  else launch_label<int32_t>(in_dev, g, connectivity, n_vox, labels_dev, st);
  hipLaunchKernelGGL(cc_compress_kernel, dim3((unsigned)n_chunks), dim3(kBlock), 0, st, labels_dev, n_vox, counts);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(1024), 0, st, counts, n_chunks, total);
  hipLaunchKernelGGL(cc_encode_kernel, dim3((unsigned)n_chunks), dim3(kBlock), 0, st, labels_dev, n_vox, (const int32_t*)counts);
  hipLaunchKernelGGL(cc_resolve_kernel, dim3(blocks_for(n_vox, kBlock)), dim3(kBlock), 0, st, labels_dev, n_vox);
  hipLaunchKernelGGL(cc_decode_kernel, dim3(blocks_for(n_vox, kBlock)), dim3(kBlock), 0, st, labels_dev, n_vox);
  T2_HIP(hipGetLastError());
  if (n_out) {
    T2_HIP(hipMemcpyAsync(pinned, total, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    T2_HIP(hipStreamSynchronize(st));
    *n_out = pinned[0];
  }
  return T2FIT_OK;
}

int t2fit_components_stats_dev(const int32_t* labels_dev, int nz, int ny, int nx, int n, int64_t* sizes_dev, int32_t* bbox_dev,
                               int64_t* sums_dev, void* stream) {
  const std::string who = "t2fit_components_stats_dev";
  if (!labels_dev) return fail(T2FIT_E_INVALID, who + ": labels_dev is NULL");
  if (int rc = check_volume(who, nz, ny, nx)) return rc;
  if (n < 0) return fail(T2FIT_E_INVALID, who + ": n is negative");
  if ((reinterpret_cast<uintptr_t>(labels_dev) & 3u) || (reinterpret_cast<uintptr_t>(bbox_dev) & 3u) ||
      (reinterpret_cast<uintptr_t>(sizes_dev) & 7u) || (reinterpret_cast<uintptr_t>(sums_dev) & 7u))
    return fail(T2FIT_E_INVALID, who + ": a table or the volume is not aligned to its element size");
  if (!sizes_dev && !bbox_dev && !sums_dev) return T2FIT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int n_vox = (int)((int64_t)nz * ny * nx);
  const int64_t n_rows = (int64_t)n + 1;
  const Tables t{sizes_dev, bbox_dev, sums_dev};
  const int64_t n_pieces = ceil_div<int64_t>(n_vox, 64);
  const int64_t blocks = std::min<int64_t>(kStatMaxBlocks, ceil_div<int64_t>(n_pieces, kStatMinPieces * (kBlock / 64)));
  const int64_t per_wave = ceil_div<int64_t>(n_pieces, blocks * (kBlock / 64));
  hipLaunchKernelGGL(cc_stats_init_kernel, dim3(blocks_for(n_rows, kBlock)), dim3(kBlock), 0, st, n_rows, nz, ny, nx, t);
  hipLaunchKernelGGL(cc_stats_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, labels_dev, ny, nx, n_vox, n, per_wave, t);
  T2_HIP(hipGetLastError());
  return T2FIT_OK;
}

int t2fit_components_lut_dev(const int64_t* sizes_dev, int n, int64_t min_size, int64_t max_size, int largest, int renumber,
                             int32_t* lut_dev, int32_t* n_kept_out, void* stream) {
  const std::string who = "t2fit_components_lut_dev";
  if (!sizes_dev || !lut_dev) return fail(T2FIT_E_INVALID, who + ": sizes_dev / lut_dev is NULL");
  if (n < 0) return fail(T2FIT_E_INVALID, who + ": n is negative");
  if (min_size < 0 || max_size < 0) return fail(T2FIT_E_INVALID, who + ": min_size / max_size is negative");
  if ((largest != 0 && largest != 1) || (renumber != 0 && renumber != 1))
    return fail(T2FIT_E_INVALID, who + ": largest and renumber must be 0 or 1");
  if ((reinterpret_cast<uintptr_t>(sizes_dev) & 7u) || (reinterpret_cast<uintptr_t>(lut_dev) & 3u))
    return fail(T2FIT_E_INVALID, who + ": sizes_dev / lut_dev is not aligned to its element size");
  hipStream_t st = (hipStream_t)stream;
  int32_t* pinned = nullptr;
  if (n_kept_out && !(pinned = pinned_word())) return fail(T2FIT_E_HIP, who + ": no pinned memory for the count");
  const int64_t n_rows = (int64_t)n + 1;
  const int64_t n_chunks = ceil_div<int64_t>(n_rows, kChunk);
  char* scratch = nullptr;
  T2_HIP(scratch_get(st, kScratchComponents, kHeadBytes + (size_t)n_chunks * sizeof(int32_t), &scratch));
  LutScratch* head = reinterpret_cast<LutScratch*>(scratch);
  int32_t* counts = reinterpret_cast<int32_t*>(scratch + kHeadBytes);
  T2_HIP(hipMemsetAsync(head, 0, sizeof(LutScratch), st));
  hipLaunchKernelGGL(cc_lut_count_kernel, dim3((unsigned)n_chunks), dim3(kBlock), 0, st, sizes_dev, n_rows, min_size, max_size, largest,
                     head, counts);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(1024), 0, st, counts, n_chunks, &head->n_passing);
  hipLaunchKernelGGL(cc_lut_write_kernel, dim3((unsigned)n_chunks), dim3(kBlock), 0, st, sizes_dev, n_rows, min_size, max_size, largest,
                     renumber, head, (const int32_t*)counts, lut_dev);
  T2_HIP(hipGetLastError());
  if (n_kept_out) {
    T2_HIP(hipMemcpyAsync(pinned, &head->n_kept, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    T2_HIP(hipStreamSynchronize(st));
    *n_kept_out = pinned[0];
  }
  return T2FIT_OK;
}

}  // extern "C"

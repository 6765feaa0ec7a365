// t2fit_nnls.hip -- multi-component T2 spectra by regularised non-negative least squares (include/t2fit.h:
// t2fit_nnls_params_default, t2fit_nnls_workgroup, t2fit_nnls_pack_bytes, t2fit_nnls_pack_host, t2fit_nnls_dev, t2fit_nnls_chi2_params_default,
// t2fit_nnls_chi2_dev; fetal_t2mapping_amd/_nnls.py states the result in numpy and the kernel equals it bit for bit).
//
// A wave per voxel.  In the outer step lane j is basis function j (h_j, w_j); in the factor, the two substitutions and the
// partial step lane r is position r of the passive list (P_r, x_r, row r of L).  G is staged once per workgroup in LDS (its
// row P_k is read by consecutive lanes); every wave keeps its packed lower-triangular L in LDS, row r at r (r + 1) / 2.  A
// column of the packed triangle, L[c][k] for the lanes c, lies at c (c + 1) / 2 + k doubles: the triangular numbers are
// distinct modulo 32, so the 32 lanes of a ds_read_b64 group fall on 32 different bank pairs, and a row is consecutive.
//
// Every substitution is column-oriented: step k divides on lane k's value, broadcasts it by a lane read, and every later
// (earlier, for the transposed solve) lane subtracts one product.  Each lane thereby sees exactly the operations of the
// row-oriented statement in its order, so the bits are the statement's.  The factor of G_PP in list order does not depend
// on whether a row is recomputed or kept -- row r reads only rows < r -- so an insertion appends one row and a removal
// recomputes only the rows from the first removed position on, where the statement may refactor from scratch.
//
// The grid is persistent: a wave takes 64 consecutive voxels per increment of a counter, writes the voxels outside the
// mask and the non-finite ones lane-parallel, then fits the rest one after the other.  After the staging barrier no wave
// waits on another.  No floating-point atomics; every register index is a constant (no scratch).
//
// The chi^2 rule (t2fit_nnls_chi2_dev) is the same kernel compiled a second time (nnls_kernel<true>): the wave keeps its
// voxel -- y, h, tol and sum y^2 -- through a short, bounded sequence of such solves whose weight it chooses from the
// misfit of the solve before.  G in LDS is A^T A (the header's mu is 0); the weight enters as the wave-uniform mu * mu added
// to the diagonal element where factor_row reads it, which is the rounding of the packed G of that weight.  Every decision
// of the rule is taken on values read from one lane, so the control flow stays wave-uniform.
#include <hip/hip_runtime.h>

#include <algorithm>
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

constexpr uint32_t kMagic = 0x4C4E3254u;
constexpr int kChunk = T2FIT_NNLS_CHUNK;          // voxels a wave takes per counter increment: one per lane of the pre-pass
constexpr int kMaxWaves = T2FIT_NNLS_MAX_WAVES;   // waves of a workgroup at most
constexpr size_t kLdsBytes = 160 * 1024;          // LDS of a CU
constexpr int kWaveSlots = 32;                    // waves a CU holds at most

struct NnlsHeader {  // 64 bytes; include/t2fit.h documents the block
  uint32_t magic;
  int32_t n_te, n_basis, n_func;
  double mu;
  uint64_t off_a, off_g, off_w, bytes, reserved;
};
static_assert(sizeof(NnlsHeader) == 64, "header layout");

bool sizes_ok(int n_te, int n_basis, int n_func) {
  return n_te >= 2 && n_te <= T2FIT_MAX_TE && n_basis >= 2 && n_basis <= T2FIT_NNLS_MAX_BASIS && n_func >= 0 && n_func <= T2FIT_NNLS_MAX_FUNC;
}

std::string sizes_text(int n_te, int n_basis, int n_func) {
  return "n_te must be 2 .. " + std::to_string(T2FIT_MAX_TE) + ", n_basis 2 .. " + std::to_string(T2FIT_NNLS_MAX_BASIS) + " and n_func 0 .. " +
         std::to_string(T2FIT_NNLS_MAX_FUNC) + ", got " + std::to_string(n_te) + ", " + std::to_string(n_basis) + " and " + std::to_string(n_func);
}

NnlsHeader header_for(int n_te, int n_basis, int n_func) {
  NnlsHeader h;
  std::memset(&h, 0, sizeof(h));
  h.magic = kMagic;
  h.n_te = n_te;
  h.n_basis = n_basis;
  h.n_func = n_func;
  h.off_a = sizeof(NnlsHeader);
  h.off_g = h.off_a + align_up(size_t(n_te) * n_basis * sizeof(double), 16);
  h.off_w = h.off_g + align_up(size_t(n_basis) * n_basis * sizeof(double), 16);
  h.bytes = h.off_w + align_up(size_t(n_func) * n_basis * sizeof(double), 16);
  return h;
}

// doubles of a wave's LDS: the packed triangle, then 64 doubles and 64 ints (as 32 doubles) for the list's compaction
constexpr int tri(int r) { return r * (r + 1) / 2; }
int wave_doubles(int n_basis) { return tri(n_basis) + 64 + 32; }
size_t lds_bytes(int n_basis, int waves) { return (size_t(n_basis) * n_basis + size_t(waves) * wave_doubles(n_basis)) * sizeof(double); }

// workgroups of `waves` waves a CU holds: by LDS and by wave slots
int per_cu(int n_basis, int waves) { return std::min(int(kLdsBytes / lds_bytes(n_basis, waves)), kWaveSlots / waves); }

// waves of a workgroup: the count that puts the most waves on a CU, the larger workgroup on a tie (G is staged once per
// workgroup).  64 basis functions: 7 waves, one workgroup; 40: 8 waves, two workgroups; up to 29: 8 waves, four workgroups
int waves_for(int n_basis) {
  int best = 1;
  for (int w = 2; w <= kMaxWaves; ++w)
    if (w * per_cu(n_basis, w) >= best * per_cu(n_basis, best)) best = w;
  return best;
}

// the value of `lane` (wave-uniform) in every lane
__device__ __forceinline__ double bcast(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// a value every lane holds alike, read from the first lane: it, and what is computed from it, can live in scalar registers
__device__ __forceinline__ double uniform(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// orders this wave's LDS writes before its later LDS reads by other lanes (LDS serves one wave's accesses in order)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = fmax(v, __shfl_xor(v, s, 64));
  return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = fmin(v, __shfl_xor(v, s, 64));
  return v;
}

__device__ __forceinline__ uint64_t below(int p) { return p >= 64 ? ~uint64_t(0) : (uint64_t(1) << p) - 1; }  // bits 0 .. p - 1

// Row r of the factor of G_PP in list order, from the rows before it; j = P_r.  Lane c <= r holds t_c = G[j][P_c]; step k
// turns t_k into L[r][k] and subtracts its product from every later lane (lane r subtracts the square: the pivot).  False,
// with L untouched, unless the pivot passes.  kChi2: G is A^T A and m2 = mu * mu is added to its diagonal element as read (lane
// r's t and the pivot's bound); the lanes before r read G[j][P_c] with P_c != j.
template <bool kChi2>
__device__ __forceinline__ bool factor_row(const double* __restrict__ G, double* __restrict__ L, int nb, int lane, int r, int j, int P,
                                           double piv_rel, double m2) {
  double t = lane <= r ? G[j * nb + P] : 0.0;
  if constexpr (kChi2) {
    if (lane == r) t = t + m2;
  }
  const int row = tri(lane);
  for (int k = 0; k < r; ++k) {
    const double lk = bcast(t, k) / L[tri(k) + k];
    if (lane == k) t = lk;
    else if (lane > k && lane < r) t = t - L[row + k] * lk;
    else if (lane == r) t = t - lk * lk;
  }
  const double d = bcast(t, r);
  double gjj = G[j * nb + j];
  if constexpr (kChi2) gjj = gjj + m2;
  if (!(d > piv_rel * gjj)) return false;
  if (lane < r) L[tri(r) + lane] = t;
  else if (lane == r) L[tri(r) + r] = sqrt(d);
  wave_lds_sync();
  return true;
}

struct Out {
  float* x;
  float* func;
  float* amp;
  float* rmse;
  int32_t* nit;
  int32_t* status;
};

struct Chi2 {  // the rule's numbers and outputs (nnls_kernel<true>; unused, all zero, by nnls_kernel<false>)
  double factor, mu_first, grow, exact_rel, mu_exact;
  int n_grow, n_bisect;
  float* mu;
  float* ratio;
  int32_t* solves;
  int32_t* rule;
};

enum : int { kUnregularised, kExactFit, kBracket, kBisect, kChosen };  // what the solve just run was for

template <bool kChi2>
__global__ __launch_bounds__(64 * kMaxWaves) void nnls_kernel(const float* __restrict__ y, int n_te, int64_t n_vox,
                                                             const uint8_t* __restrict__ mask, const unsigned char* __restrict__ packed,
                                                             double tol_rel, double piv_rel, int max_iter, Out out,
                                                             unsigned long long* __restrict__ counter, Chi2 c2) {
  extern __shared__ double lds[];
  const NnlsHeader* hd = reinterpret_cast<const NnlsHeader*>(packed);
  const int nb = hd->n_basis, n_func = hd->n_func;
  const double* __restrict__ A = reinterpret_cast<const double*>(packed + hd->off_a);
  const double* __restrict__ Gg = reinterpret_cast<const double*>(packed + hd->off_g);
  const double* __restrict__ W = reinterpret_cast<const double*>(packed + hd->off_w);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double* G = lds;
  double* L = lds + nb * nb + wave * (tri(nb) + 64 + 32);
  double* sx = L + tri(nb);                         // the compaction's x by new position
  int* sp = reinterpret_cast<int*>(sx + 64);        // the compaction's P by new position
  for (int i = threadIdx.x; i < nb * nb; i += blockDim.x) G[i] = Gg[i];
  __syncthreads();
  const int limit = max_iter > 0 ? max_iter : 3 * nb;
  const int64_t n_chunks = (n_vox + kChunk - 1) / kChunk;

  for (;;) {
    unsigned long long c = 0;
    if (lane == 0) c = atomicAdd(counter, 1ull);
    const unsigned c_lo = __builtin_amdgcn_readfirstlane(unsigned(c)), c_hi = __builtin_amdgcn_readfirstlane(unsigned(c >> 32));
    c = (static_cast<unsigned long long>(c_hi) << 32) | c_lo;
    if (int64_t(c) >= n_chunks) break;
    const int64_t v0 = int64_t(c) * kChunk;

    // pre-pass, a voxel per lane: outside the mask and non-finite voxels are written here
    uint64_t todo;
    {
      const int64_t v = v0 + lane;
      const bool in = v < n_vox;
      const bool masked = in && mask != nullptr && mask[v] == 0;
      bool finite = true;
      if (in && !masked)
        for (int e = 0; e < n_te; ++e) finite = finite && t2fit::finite_bits(y[int64_t(e) * n_vox + v]);
      if (in && (masked || !finite)) {
        if (out.x)
          for (int j = 0; j < nb; ++j) out.x[int64_t(j) * n_vox + v] = 0.0f;
        for (int m = 0; m < n_func; ++m) out.func[int64_t(m) * n_vox + v] = 0.0f;
        out.amp[v] = 0.0f;
        out.rmse[v] = 0.0f;
        out.nit[v] = 0;
        out.status[v] = masked ? T2FIT_NNLS_MASKED : T2FIT_NNLS_NONFINITE;
        if constexpr (kChi2) {
          c2.mu[v] = 0.0f;
          c2.ratio[v] = 0.0f;
          c2.solves[v] = 0;
          c2.rule[v] = -1;
        }
      }
      todo = __ballot(in && !masked && finite);
    }

    while (todo) {
      const int b = __ffsll(static_cast<unsigned long long>(todo)) - 1;
      todo &= todo - 1;
      const int64_t v = v0 + b;

      // step 1: lane i holds y_i; h_j = sum_i A[i][j] y_i, tol = tol_rel max |h|
      const double yl = lane < n_te ? double(y[int64_t(lane) * n_vox + v]) : 0.0;
      double h = 0.0, yy = 0.0;
      for (int i = 0; i < n_te; ++i) {
        const double yi = bcast(yl, i);
        if (lane < nb) h = h + A[i * nb + lane] * yi;
        if constexpr (kChi2) yy = yy + yi * yi;
      }
      const double tol = tol_rel * wave_max(fabs(h));
      if constexpr (kChi2) yy = uniform(yy);

      int P, p, nit, status;  // lane r of P: the basis function at list position r
      double xl, xj, ss;      // lane r of xl: its coefficient; after a solve x_j on lane j and the misfit
      // the rule (kChi2): the weight of the solve about to run and what it is for, the bracket, the sums over the solves
      double mu = 0.0, ss0 = 0.0, target = 0.0, lo = 0.0, hi = 0.0;
      int stage = kUnregularised, rule = T2FIT_NNLS_RULE_FOUND, g = 0, bisected = 0, solves = 0, nit_sum = 0, status_max = T2FIT_NNLS_OK;

      for (;;) {  // a solve per pass: one for nnls_kernel<false>, at most n_grow + n_bisect + 3 under the rule
        const double m2 = kChi2 ? uniform(mu * mu) : 0.0;
        P = 0;
        xl = 0.0;
        p = 0, nit = 0, status = T2FIT_NNLS_OK;
        uint64_t pmask = 0, banned = 0;  // by basis function: in P, banned

        for (;;) {
          // step 2: w_j = h_j - sum_{k in P} G[j][P_k] x_k, the largest w_j > tol off P and off the ban list, lowest j on a tie
          double w = h;
          for (int k = 0; k < p; ++k) {
            const int pk = __builtin_amdgcn_readlane(P, k);
            const double xk = bcast(xl, k);
            if (lane < nb) w = w - G[pk * nb + lane] * xk;
          }
          const bool cand = lane < nb && !((pmask | banned) >> lane & 1) && w > tol;
          const uint64_t cands = __ballot(cand);
          if (!cands) break;
          const double wmax = wave_max(cand ? w : -std::numeric_limits<double>::infinity());
          const int j = __ffsll(static_cast<unsigned long long>(__ballot(cand && w == wmax))) - 1;
          if (nit == limit) {
            status = T2FIT_NNLS_MAXITER;
            break;
          }
          ++nit;
          // step 3: append j; a failed pivot bans it until the next successful insertion
          if (lane == p) {
            P = j;
            xl = 0.0;
          }
          if (!factor_row<kChi2>(G, L, nb, lane, p, j, P, piv_rel, m2)) {
            banned |= uint64_t(1) << j;
            continue;
          }
          ++p;
          pmask |= uint64_t(1) << j;
          banned = 0;

          bool broke = false;
          for (;;) {
            // step 4: L z = h_P, k ascending; L^T s = z, k descending
            double t = __shfl(h, P, 64);
            const int row = tri(lane);
            for (int k = 0; k < p; ++k) {
              const double zk = bcast(t, k) / L[tri(k) + k];
              if (lane == k) t = zk;
              else if (lane > k && lane < p) t = t - L[row + k] * zk;
            }
            for (int k = p - 1; k >= 0; --k) {
              const double sk = bcast(t, k) / L[tri(k) + k];
              if (lane == k) t = sk;
              else if (lane < k) t = t - L[tri(k) + lane] * sk;
            }
            // step 5
            const bool neg = lane < p && !(t > 0.0);
            if (!__ballot(neg)) {
              if (lane < p) xl = t;
              break;
            }
            // step 6: the partial step; the first position that attains alpha becomes 0 exactly, whatever is not above 0 leaves
            double a = std::numeric_limits<double>::infinity();
            if (neg) {
              a = xl / (xl - t);
              if (a != a) a = 0.0;  // 0 / 0: a new entry whose solution is exactly 0 does not move
            }
            const double alpha = wave_min(a);
            const int q = __ffsll(static_cast<unsigned long long>(__ballot(neg && a == alpha))) - 1;
            double xn = xl + alpha * (t - xl);
            if (lane == q) xn = 0.0;
            const bool keep = lane < p && xn > 0.0;
            const uint64_t keepmask = __ballot(keep);
            uint64_t gone = below(p) & ~keepmask;
            const int first = __ffsll(static_cast<unsigned long long>(gone)) - 1;
            if (!gone) {  // (cannot happen: position q leaves; keeps the loop bounded whatever the arithmetic does)
              broke = true;
              break;
            }
            while (gone) {
              const int r = __ffsll(static_cast<unsigned long long>(gone)) - 1;
              gone &= gone - 1;
              pmask &= ~(uint64_t(1) << __builtin_amdgcn_readlane(P, r));
            }
            if (keep) {
              const int at = __popcll(keepmask & below(lane));
              sx[at] = xn;
              sp[at] = P;
            }
            wave_lds_sync();
            p = __popcll(keepmask);
            xl = lane < p ? sx[lane] : 0.0;
            P = lane < p ? sp[lane] : 0;
            wave_lds_sync();
            if (p == 0) break;
            // the rows before the first removed position are the factor's still: recompute the others in list order
            for (int r = first; r < p && !broke; ++r)
              if (!factor_row<kChi2>(G, L, nb, lane, r, __builtin_amdgcn_readlane(P, r), P, piv_rel, m2)) broke = true;
            if (broke) break;
          }
          if (broke) {
            status = T2FIT_NNLS_BREAKDOWN;
            break;
          }
        }

        // outputs: x_j on lane j, r_i on lane i; the functionals on lanes 0 .. n_func - 1 and amp on lane n_func
        double ri = yl;
        xj = 0.0;
        for (int k = 0; k < p; ++k) {
          const int pk = __builtin_amdgcn_readlane(P, k);
          const double xk = bcast(xl, k);
          if (lane == pk) xj = xk;
          if (lane < n_te) ri = ri - A[lane * nb + pk] * xk;
        }
        ss = 0.0;
        for (int i = 0; i < n_te; ++i) {
          const double r = bcast(ri, i);
          ss = ss + r * r;
        }
        if constexpr (!kChi2) break;

        // the rule: what this solve's misfit decides.  Every lane holds the same ss; lane 0's is read so that the branches
        // below are the wave's, not the lanes'
        ss = uniform(ss);
        ++solves;
        nit_sum += nit;
        status_max = status > status_max ? status : status_max;
        if (stage == kChosen || stage == kExactFit) break;
        if (stage == kUnregularised) {
          ss0 = ss;
          if (!(ss0 > c2.exact_rel * yy)) {  // an exact fit (or a NaN misfit): no target, the fallback weight
            rule = T2FIT_NNLS_RULE_EXACT;
            stage = kExactFit;
            mu = c2.mu_exact;
            continue;
          }
          target = uniform(c2.factor * ss0);
          mu = c2.mu_first;
          stage = kBracket;
          continue;
        }
        if (stage == kBracket) {
          if (!(ss >= target)) {  // (a NaN misfit is no hit)
            lo = mu;
            if (g == c2.n_grow) {
              rule = T2FIT_NNLS_RULE_HIGH;
              break;
            }
            ++g;
            mu = uniform(mu * c2.grow);
            continue;
          }
          if (g == 0) {
            rule = T2FIT_NNLS_RULE_LOW;
            break;
          }
          hi = mu;
          stage = kBisect;
        } else {  // kBisect: the solve was at the bracket's geometric middle
          if (ss < target) lo = mu;
          else hi = mu;
          ++bisected;
        }
        mu = uniform(sqrt(lo * hi));
        if (bisected == c2.n_bisect) stage = kChosen;
      }
      double acc = 0.0;
      for (int jj = 0; jj < nb; ++jj) {
        const double xb = bcast(xj, jj);
        if (lane < n_func) acc = acc + W[lane * nb + jj] * xb;
        else if (lane == n_func) acc = acc + xb;
      }
      if (out.x && lane < nb) out.x[int64_t(lane) * n_vox + v] = float(xj);
      if (lane < n_func) out.func[int64_t(lane) * n_vox + v] = float(acc);
      else if (lane == n_func) out.amp[v] = float(acc);
      if (lane == 0) {
        out.rmse[v] = float(sqrt(ss / double(n_te)));
        if constexpr (kChi2) {
          out.nit[v] = nit_sum;
          out.status[v] = status_max;
          c2.mu[v] = float(mu);
          c2.ratio[v] = rule == T2FIT_NNLS_RULE_EXACT ? 0.0f : float(ss / ss0);
          c2.solves[v] = solves;
          c2.rule[v] = rule;
        } else {
          out.nit[v] = nit;
          out.status[v] = status;
        }
      }
    }
  }
}

// Both entry points: `chi2` NULL is the fixed weight of the packed block (nnls_kernel<false>), else the rule
// (nnls_kernel<true>) with its four outputs.  Same refusals, same launch shape, same counter.
int fit_dev(const std::string& who, const t2fit_nnls_params* params, const t2fit_nnls_chi2_params* chi2, const float* y_dev, int n_te,
            int64_t n_vox, const uint8_t* mask_dev, const void* packed_dev, const Out& out, float* mu_dev, float* ratio_dev, int32_t* solves_dev,
            int32_t* rule_dev, void* stream) {
  if (!params || !y_dev || !packed_dev || !out.amp || !out.rmse || !out.nit || !out.status)
    return fail(T2FIT_E_INVALID, who + ": params, y_dev, packed_dev, amp_dev, rmse_dev, nit_dev or status_dev is NULL");
  if (n_te < 2 || n_te > T2FIT_MAX_TE)
    return fail(T2FIT_E_INVALID, who + ": n_te must be 2 .. " + std::to_string(T2FIT_MAX_TE) + ", got " + std::to_string(n_te));
  if (n_vox < 0) return fail(T2FIT_E_INVALID, who + ": n_vox is negative");
  if (!(params->tol_rel >= 0.0 && std::isfinite(params->tol_rel)) || !(params->piv_rel >= 0.0 && std::isfinite(params->piv_rel)))
    return fail(T2FIT_E_INVALID, who + ": tol_rel and piv_rel must be finite and not negative");
  if (params->max_iter < 0 || params->max_blocks < 0) return fail(T2FIT_E_INVALID, who + ": max_iter and max_blocks must not be negative");
  if (chi2) {
    if (!(std::isfinite(chi2->factor) && chi2->factor > 1.0)) return fail(T2FIT_E_INVALID, who + ": factor must be finite and above 1");
    if (!(std::isfinite(chi2->grow) && chi2->grow > 1.0)) return fail(T2FIT_E_INVALID, who + ": grow must be finite and above 1");
    if (!(std::isfinite(chi2->mu_first) && chi2->mu_first > 0.0)) return fail(T2FIT_E_INVALID, who + ": mu_first must be finite and above 0");
    if (!(std::isfinite(chi2->exact_rel) && chi2->exact_rel >= 0.0) || !(std::isfinite(chi2->mu_exact) && chi2->mu_exact >= 0.0))
      return fail(T2FIT_E_INVALID, who + ": exact_rel and mu_exact must be finite and not negative");
    if (chi2->n_grow < 0 || chi2->n_grow > 64 || chi2->n_bisect < 0 || chi2->n_bisect > 64)
      return fail(T2FIT_E_INVALID, who + ": n_grow and n_bisect must be 0 .. 64");
  }
  if (misaligned(y_dev, 4) || misaligned(out.x, 4) || misaligned(out.func, 4) || misaligned(out.amp, 4) || misaligned(out.rmse, 4) ||
      misaligned(out.nit, 4) || misaligned(out.status, 4) || misaligned(mu_dev, 4) || misaligned(ratio_dev, 4) || misaligned(solves_dev, 4) ||
      misaligned(rule_dev, 4))
    return fail(T2FIT_E_INVALID, who + ": y_dev and the outputs must be aligned to 4 bytes");
  if (misaligned(packed_dev, 16)) return fail(T2FIT_E_INVALID, who + ": packed_dev must be aligned to 16 bytes");
  if (n_vox == 0) return T2FIT_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  NnlsHeader h;
  T2_HIP(hipMemcpyAsync(&h, packed_dev, sizeof(h), hipMemcpyDeviceToHost, st));
  T2_HIP(hipStreamSynchronize(st));
  if (h.magic != kMagic) return fail(T2FIT_E_INVALID, who + ": packed_dev does not hold a packed basis (magic)");
  if (h.n_te != n_te)
    return fail(T2FIT_E_INVALID, who + ": the basis was packed for n_te " + std::to_string(h.n_te) + ", the call has " + std::to_string(n_te));
  if (!sizes_ok(h.n_te, h.n_basis, h.n_func)) return fail(T2FIT_E_INVALID, who + ": the basis header has sizes out of range");
  const NnlsHeader want = header_for(h.n_te, h.n_basis, h.n_func);
  if (h.off_a != want.off_a || h.off_g != want.off_g || h.off_w != want.off_w || h.bytes != want.bytes || !(std::isfinite(h.mu) && h.mu >= 0.0))
    return fail(T2FIT_E_INVALID, who + ": the basis header is not what t2fit_nnls_pack_host writes");
  if (h.n_func > 0 && !out.func) return fail(T2FIT_E_INVALID, who + ": func_dev is NULL and the basis has functionals");
  if (chi2 && h.mu != 0.0)
    return fail(T2FIT_E_INVALID, who + ": the basis was packed with mu " + std::to_string(h.mu) + "; the rule chooses the weight and needs mu 0");

  int dev = 0, cus = 0;
  T2_HIP(hipGetDevice(&dev));
  T2_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int waves = waves_for(h.n_basis);
  const size_t lds = lds_bytes(h.n_basis, waves);
  const int64_t n_chunks = ceil_div<int64_t>(n_vox, kChunk);
  int64_t blocks = std::min<int64_t>(ceil_div<int64_t>(n_chunks, waves), int64_t(cus) * per_cu(h.n_basis, waves));
  if (params->max_blocks > 0) blocks = std::min<int64_t>(blocks, params->max_blocks);
  const auto kernel = chi2 ? &nnls_kernel<true> : &nnls_kernel<false>;
  T2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
  unsigned long long* counter = nullptr;
  T2_HIP(hipMallocAsync(reinterpret_cast<void**>(&counter), sizeof(unsigned long long), st));
  if (const hipError_t zeroed = hipMemsetAsync(counter, 0, sizeof(unsigned long long), st); zeroed != hipSuccess) {
    (void)hipFreeAsync(counter, st);
    T2_HIP(zeroed);
  }
  Chi2 c2;
  std::memset(&c2, 0, sizeof(c2));
  if (chi2) c2 = Chi2{chi2->factor, chi2->mu_first, chi2->grow, chi2->exact_rel, chi2->mu_exact, chi2->n_grow, chi2->n_bisect,
                      mu_dev,       ratio_dev,      solves_dev, rule_dev};
  const dim3 grid(static_cast<unsigned>(blocks)), block(64 * waves);
  const unsigned char* packed = static_cast<const unsigned char*>(packed_dev);
  if (chi2)
    hipLaunchKernelGGL(nnls_kernel<true>, grid, block, lds, st, y_dev, n_te, n_vox, mask_dev, packed, params->tol_rel, params->piv_rel,
                       params->max_iter, out, counter, c2);
  else
    hipLaunchKernelGGL(nnls_kernel<false>, grid, block, lds, st, y_dev, n_te, n_vox, mask_dev, packed, params->tol_rel, params->piv_rel,
                       params->max_iter, out, counter, c2);
  const hipError_t e = hipGetLastError();
  (void)hipFreeAsync(counter, st);
  T2_HIP(e);
  return T2FIT_OK;
}

}  // namespace

extern "C" {

int t2fit_nnls_params_default(t2fit_nnls_params* params) {
  if (!params) return fail(T2FIT_E_INVALID, "t2fit_nnls_params_default: params is NULL");
  params->tol_rel = 1e-10;
  params->piv_rel = 1e-12;
  params->max_iter = 0;
  params->max_blocks = 0;
  return T2FIT_OK;
}

int t2fit_nnls_workgroup(int n_basis, int* waves, size_t* lds_bytes_out, int* workgroups_per_cu) {
  if (!waves || !lds_bytes_out || !workgroups_per_cu)
    return fail(T2FIT_E_INVALID, "t2fit_nnls_workgroup: waves, lds_bytes or workgroups_per_cu is NULL");
  if (n_basis < 2 || n_basis > T2FIT_NNLS_MAX_BASIS)
    return fail(T2FIT_E_INVALID, "t2fit_nnls_workgroup: n_basis must be 2 .. " + std::to_string(T2FIT_NNLS_MAX_BASIS) + ", got " + std::to_string(n_basis));
  *waves = waves_for(n_basis);
  *lds_bytes_out = lds_bytes(n_basis, *waves);
  *workgroups_per_cu = per_cu(n_basis, *waves);
  return T2FIT_OK;
}

int t2fit_nnls_pack_bytes(int n_te, int n_basis, int n_func, size_t* bytes) {
  if (!bytes) return fail(T2FIT_E_INVALID, "t2fit_nnls_pack_bytes: bytes is NULL");
  if (!sizes_ok(n_te, n_basis, n_func)) return fail(T2FIT_E_INVALID, "t2fit_nnls_pack_bytes: " + sizes_text(n_te, n_basis, n_func));
  *bytes = header_for(n_te, n_basis, n_func).bytes;
  return T2FIT_OK;
}

int t2fit_nnls_pack_host(int n_te, int n_basis, int n_func, const double* basis, double mu, const double* functionals, void* packed_host,
                         size_t bytes) {
  if (!sizes_ok(n_te, n_basis, n_func)) return fail(T2FIT_E_INVALID, "t2fit_nnls_pack_host: " + sizes_text(n_te, n_basis, n_func));
  if (!basis || !packed_host || (n_func > 0 && !functionals))
    return fail(T2FIT_E_INVALID, "t2fit_nnls_pack_host: basis, packed_host or (with n_func > 0) functionals is NULL");
  if (!(std::isfinite(mu) && mu >= 0.0)) return fail(T2FIT_E_INVALID, "t2fit_nnls_pack_host: mu must be finite and not negative");
  const NnlsHeader h = header_for(n_te, n_basis, n_func);
  if (bytes < h.bytes)
    return fail(T2FIT_E_INVALID, "t2fit_nnls_pack_host: the buffer has " + std::to_string(bytes) + " bytes, the basis needs " +
                                     std::to_string(h.bytes));
  for (int i = 0; i < n_te * n_basis; ++i)
    if (!std::isfinite(basis[i]))
      return fail(T2FIT_E_INVALID, "t2fit_nnls_pack_host: the basis has a non-finite entry (echo " + std::to_string(i / n_basis) + ", column " +
                                       std::to_string(i % n_basis) + ")");
  for (int i = 0; i < n_func * n_basis; ++i)
    if (!std::isfinite(functionals[i]))
      return fail(T2FIT_E_INVALID, "t2fit_nnls_pack_host: functional " + std::to_string(i / n_basis) + " has a non-finite entry");
  unsigned char* out = static_cast<unsigned char*>(packed_host);
  std::memset(out, 0, h.bytes);
  NnlsHeader hw = h;
  hw.mu = mu;
  std::memcpy(out, &hw, sizeof(hw));
  std::memcpy(out + h.off_a, basis, size_t(n_te) * n_basis * sizeof(double));
  double* G = reinterpret_cast<double*>(out + h.off_g);
  const double m2 = mu * mu;
  for (int j = 0; j < n_basis; ++j)
    for (int k = 0; k < n_basis; ++k) {
      double s = 0.0;
      for (int i = 0; i < n_te; ++i) s = s + basis[i * n_basis + j] * basis[i * n_basis + k];
      G[j * n_basis + k] = j == k ? s + m2 : s;
    }
  if (n_func > 0) std::memcpy(out + h.off_w, functionals, size_t(n_func) * n_basis * sizeof(double));
  return T2FIT_OK;
}

int t2fit_nnls_chi2_params_default(t2fit_nnls_chi2_params* chi2) {
  if (!chi2) return fail(T2FIT_E_INVALID, "t2fit_nnls_chi2_params_default: chi2 is NULL");
  chi2->factor = 1.02;
  chi2->mu_first = 1e-3;
  chi2->grow = 4.0;
  chi2->exact_rel = 1e-12;
  chi2->mu_exact = 0.03;
  chi2->n_grow = 6;
  chi2->n_bisect = 5;
  return T2FIT_OK;
}

int t2fit_nnls_dev(const t2fit_nnls_params* params, const float* y_dev, int n_te, int64_t n_vox, const uint8_t* mask_dev,
                   const void* packed_dev, float* x_dev, float* func_dev, float* amp_dev, float* rmse_dev, int32_t* nit_dev,
                   int32_t* status_dev, void* stream) {
  return fit_dev("t2fit_nnls_dev", params, nullptr, y_dev, n_te, n_vox, mask_dev, packed_dev, Out{x_dev, func_dev, amp_dev, rmse_dev, nit_dev, status_dev},
                 nullptr, nullptr, nullptr, nullptr, stream);
}

int t2fit_nnls_chi2_dev(const t2fit_nnls_params* params, const t2fit_nnls_chi2_params* chi2, const float* y_dev, int n_te, int64_t n_vox,
                        const uint8_t* mask_dev, const void* packed_dev, float* x_dev, float* func_dev, float* amp_dev, float* rmse_dev,
                        int32_t* nit_dev, int32_t* status_dev, float* mu_dev, float* ratio_dev, int32_t* solves_dev, int32_t* rule_dev,
                        void* stream) {
  if (!chi2 || !mu_dev || !ratio_dev || !solves_dev || !rule_dev)
    return fail(T2FIT_E_INVALID, "t2fit_nnls_chi2_dev: chi2, mu_dev, ratio_dev, solves_dev or rule_dev is NULL");
  return fit_dev("t2fit_nnls_chi2_dev", params, chi2, y_dev, n_te, n_vox, mask_dev, packed_dev,
                 Out{x_dev, func_dev, amp_dev, rmse_dev, nit_dev, status_dev}, mu_dev, ratio_dev, solves_dev, rule_dev, stream);
}

}  // extern "C"

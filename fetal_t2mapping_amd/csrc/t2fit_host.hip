// t2fit_host.hip -- the host side of the C ABI of include/t2fit.h: the library's basics (ABI version, the one error string,
// default configuration, device count) and the host seam -- contexts with their streams, pinned staging and slab
// pipeline (t2fit_context.h), and the voxel seam.  No kernels: the fit is reached through t2fit_launch.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "t2fit_config.h"
#include "t2fit_context.h"
#include "t2fit_error.h"
#include "t2fit_launch.h"
#include "t2fit_support.h"

using namespace t2fit;

namespace {
thread_local std::string g_err;
}

// t2fit_error.h: the one error string of the library (the other translation units report through it too)
int t2fit::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

extern "C" {

int t2fit_abi_version(void) { return T2FIT_ABI_VERSION; }

const char* t2fit_last_error(void) { return g_err.c_str(); }

int t2fit_config_default(t2fit_config* cfg, int model, int low_field) {
  const int rc = config_default_impl(cfg, model, low_field);
  return rc == T2FIT_OK ? rc : fail(rc, "t2fit_config_default: cfg is NULL or model unknown");
}

int t2fit_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

// ---- host seam through a context (t2fit_context.h) -------------------------------------------------------------
// (T2FIT_COPY_THREADS is read per t2fit_create, T2FIT_HOST_SLABS per call: tests change the latter between calls)
#define T2_HIP_C(call)                                                          \
  do {                                                                          \
    hipError_t e_ = (call);                                                     \
    if (e_ != hipSuccess) {                                                     \
      cleanup();                                                                \
      return fail(T2FIT_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    }                                                                           \
  } while (0)

int t2fit_create(int device, t2fit_context** out) {
  if (!out) return fail(T2FIT_E_INVALID, "t2fit_create: out is NULL");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
    (void)hipGetLastError();
    return fail(T2FIT_E_HIP, "t2fit_create: no such HIP device");
  }
  T2_HIP(hipSetDevice(device));
  t2fit_context* c = new t2fit_context;
  c->device = device;
  auto cleanup = [&]() {
    if (c->s_in) (void)hipStreamDestroy(c->s_in);
    if (c->s_fit) (void)hipStreamDestroy(c->s_fit);
    if (c->s_out) (void)hipStreamDestroy(c->s_out);
    delete c;
  };
  T2_HIP_C(hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking));
  T2_HIP_C(hipStreamCreateWithFlags(&c->s_fit, hipStreamNonBlocking));
  T2_HIP_C(hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking));
  int threads = 8;
  if (const char* e = std::getenv("T2FIT_COPY_THREADS")) threads = std::max(0, std::min(64, std::atoi(e)));
  c->pool = new t2fit::CopyPool(threads);
  *out = c;
  return T2FIT_OK;
}

int t2fit_destroy(t2fit_context* c) {
  if (!c) return T2FIT_OK;
  {
    std::lock_guard<std::mutex> g(c->busy);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->s_in);
    (void)hipStreamSynchronize(c->s_fit);
    (void)hipStreamSynchronize(c->s_out);
    for (hipStream_t st : {c->s_in, c->s_fit, c->s_out}) scratch_release_stream(c->device, st);
    for (auto ev : c->events) (void)hipEventDestroy(ev);
    for (int j = 0; j < 2; ++j) {
      if (c->pin_in[j]) (void)hipHostFree(c->pin_in[j]);
      if (c->pin_out[j]) (void)hipHostFree(c->pin_out[j]);
    }
    if (c->dev) (void)hipFree(c->dev);
    (void)hipStreamDestroy(c->s_in);
    (void)hipStreamDestroy(c->s_fit);
    (void)hipStreamDestroy(c->s_out);
    delete c->pool;
  }
  delete c;
  return T2FIT_OK;
}

int t2fit_context_volume_host(t2fit_context* c, const t2fit_config* cfg, const float* echoes, int layout,
                              const uint8_t* mask, int64_t n_vox, const t2fit_maps* maps) {
  if (!c) return fail(T2FIT_E_INVALID, "context is NULL");
  int rc = check_common(cfg, echoes, layout, n_vox);
  if (rc != T2FIT_OK) return rc;
  if (!maps || !maps->t2 || !maps->k || !maps->sigma || !maps->res)
    return fail(T2FIT_E_INVALID, "maps->t2/k/sigma/res must be non-NULL");
  if (n_vox == 0) return T2FIT_OK;
  std::lock_guard<std::mutex> guard(c->busy);
  T2_HIP(hipSetDevice(c->device));
  const int n_te = cfg->n_te;
  // Slabs of about 2.4 M voxels (multiples of 4096, so that every slab keeps the alignment the vectorised kernels
  // want; every slab of a large volume runs the large-volume kernels, also the short first and last ones): short enough that filling and draining the pipeline costs little,
  // long enough that a slab's fit covers the host-side copies of its neighbours.  The first slab is a quarter of
  // that: the device starts working after a quarter of the copy time.
  int64_t slab = (int64_t)9 << 18;  // 2,359,296
  bool graded = true;
  if (const char* e = std::getenv("T2FIT_HOST_SLABS")) {  // A/B switch and tests: number of (equal) slabs
    const int64_t want = std::max(1, std::min(4096, std::atoi(e)));
    slab = (n_vox + want - 1) / want;
    graded = false;
  }
  slab = std::max<int64_t>(4096, (slab + 4095) & ~(int64_t)4095);
  std::vector<int64_t> bounds{0};
  if (graded && n_vox > slab) bounds.push_back(std::max<int64_t>(4096, (slab / 4) & ~(int64_t)4095));
  while (bounds.back() < n_vox) bounds.push_back(std::min<int64_t>(n_vox, bounds.back() + slab));
  const int n_slabs = (int)bounds.size() - 1;
  // outputs: float maps (t2, k, sigma, res, r2, fun, t2_se), then nit (int32), then status (uint8)
  float* host_f[7] = {maps->t2, maps->k, maps->sigma, maps->res, maps->r2, maps->fun, maps->t2_se};
  const size_t slab_in = (size_t)slab * n_te * 4 + (size_t)slab;          // samples + mask bytes of one slab
  const size_t slab_out = (size_t)slab * (7 * 4 + 4 + 1);                  // every optional map wanted
  auto cleanup = [&]() {
    (void)hipStreamSynchronize(c->s_in);
    (void)hipStreamSynchronize(c->s_fit);
    (void)hipStreamSynchronize(c->s_out);
  };
  if (c->pin_in_cap < slab_in) {
    for (int j = 0; j < 2; ++j) {
      if (c->pin_in[j]) (void)hipHostFree(c->pin_in[j]);
      c->pin_in[j] = nullptr;
    }
    c->pin_in_cap = 0;
    for (int j = 0; j < 2; ++j) T2_HIP_C(hipHostMalloc((void**)&c->pin_in[j], slab_in, hipHostMallocDefault));
    c->pin_in_cap = slab_in;
  }
  if (c->pin_out_cap < slab_out) {
    for (int j = 0; j < 2; ++j) {
      if (c->pin_out[j]) (void)hipHostFree(c->pin_out[j]);
      c->pin_out[j] = nullptr;
    }
    c->pin_out_cap = 0;
    for (int j = 0; j < 2; ++j) T2_HIP_C(hipHostMalloc((void**)&c->pin_out[j], slab_out, hipHostMallocDefault));
    c->pin_out_cap = slab_out;
  }
  // device arena: echoes (slab after slab, each (n_te, len) or (len, n_te)) | 7 float maps | nit | mask | status
  const size_t nb_e = (size_t)n_vox * n_te * sizeof(float);
  const size_t off_maps = align_up(nb_e, 256);
  const size_t map_b = align_up((size_t)n_vox * 4, 256);
  const size_t off_nit = off_maps + 7 * map_b;
  const size_t off_mask = off_nit + map_b;
  const size_t byte_b = align_up((size_t)n_vox, 256);
  const size_t off_status = off_mask + byte_b;
  const size_t total = off_status + byte_b;
  if (c->dev_cap < total) {
    if (c->dev) (void)hipFree(c->dev);
    c->dev = nullptr;
    c->dev_cap = 0;
    T2_HIP_C(hipMalloc((void**)&c->dev, total));
    c->dev_cap = total;
  }
  char* buf = c->dev;
  while (c->events.size() < (size_t)3 * n_slabs) {
    hipEvent_t ev;
    T2_HIP_C(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    c->events.push_back(ev);
  }
  hipEvent_t* ev_in = c->events.data();
  hipEvent_t* ev_fit = ev_in + n_slabs;
  hipEvent_t* ev_out = ev_fit + n_slabs;
  float* fm[7];
  for (int j = 0; j < 7; ++j) fm[j] = (float*)(buf + off_maps + j * map_b);
  const bool want[7] = {true, true, true, true, maps->r2 != nullptr, maps->fun != nullptr, maps->t2_se != nullptr};
  auto span = [&](int k, int64_t& lo, int64_t& len) { lo = bounds[k]; len = bounds[k + 1] - lo; };
  // Blocks of 4096 voxels without a single voxel in the mask are neither copied in (the kernels never read the samples
  // of a masked-out voxel) nor copied out (their maps are zeros: written here, not fetched): on a brain mask that is
  // half of the host-side copy traffic, which is what bounds this entry point.  runs[k]: the [start, end) voxel
  // ranges of slab k, relative to its start, that do hold masked voxels.
  constexpr int64_t kBlockVox = 4096;
  std::vector<std::vector<std::pair<int64_t, int64_t>>> runs(n_slabs);
  auto find_runs = [&](int k) {
    int64_t lo, len;
    span(k, lo, len);
    auto& r = runs[k];
    if (!mask) { r.emplace_back(0, len); return; }
    for (int64_t b = 0; b < len; b += kBlockVox) {
      const int64_t e = std::min(len, b + kBlockVox);
      const uint8_t* p = mask + lo + b;
      bool any = false;
      int64_t i = 0;
      for (; i + 8 <= e - b && !any; i += 8) {
        uint64_t w;
        std::memcpy(&w, p + i, 8);
        any = w != 0;
      }
      for (; i < e - b && !any; ++i) any = p[i] != 0;
      if (!any) continue;
      if (!r.empty() && r.back().second == b) r.back().second = e;
      else r.emplace_back(b, e);
    }
  };
  // device -> pinned: the maps of slab k, packed one after the other in its staging slot
  auto queue_d2h = [&](int k) -> hipError_t {
    int64_t lo, len;
    span(k, lo, len);
    char* dst = c->pin_out[k & 1];
    hipError_t e = hipStreamWaitEvent(c->s_out, ev_fit[k], 0);
    size_t off = 0;
    for (int j = 0; j < 7 && e == hipSuccess; ++j)
      if (want[j]) { e = hipMemcpyAsync(dst + off, fm[j] + lo, (size_t)len * 4, hipMemcpyDeviceToHost, c->s_out); off += (size_t)len * 4; }
    if (e == hipSuccess && maps->nit) { e = hipMemcpyAsync(dst + off, buf + off_nit + (size_t)lo * 4, (size_t)len * 4, hipMemcpyDeviceToHost, c->s_out); off += (size_t)len * 4; }
    if (e == hipSuccess && maps->status) e = hipMemcpyAsync(dst + off, buf + off_status + lo, (size_t)len, hipMemcpyDeviceToHost, c->s_out);
    if (e == hipSuccess) e = hipEventRecord(ev_out[k], c->s_out);
    return e;
  };
  // pinned -> the caller's arrays (worker threads)
  auto finish_out = [&](int k) -> hipError_t {
    int64_t lo, len;
    span(k, lo, len);
    hipError_t e = hipEventSynchronize(ev_out[k]);
    if (e != hipSuccess) return e;
    const char* src = c->pin_out[k & 1];
    std::vector<t2fit::CopyPool::Row> rows;
    size_t off = 0;
    auto add = [&](char* dst, size_t elem) {  // one map of this slab: copy the runs, zero the gaps (src == nullptr)
      int64_t at = 0;
      for (const auto& r : runs[k]) {
        if (r.first > at) rows.push_back({dst + at * elem, nullptr, (size_t)(r.first - at) * elem});
        rows.push_back({dst + r.first * elem, src + off + r.first * elem, (size_t)(r.second - r.first) * elem});
        at = r.second;
      }
      if (at < len) rows.push_back({dst + at * elem, nullptr, (size_t)(len - at) * elem});
      off += (size_t)len * elem;
    };
    for (int j = 0; j < 7; ++j)
      if (want[j]) add((char*)(host_f[j] + lo), 4);
    if (maps->nit) add((char*)(maps->nit + lo), 4);
    if (maps->status) add((char*)(maps->status + lo), 1);  // T2FIT_ST_MASKED == 0
    c->pool->copy(rows);
    return hipSuccess;
  };
  for (int k = 0; k < n_slabs; ++k) {
    int64_t lo, len;
    span(k, lo, len);
    char* stage = c->pin_in[k & 1];
    if (k >= 2) T2_HIP_C(hipEventSynchronize(ev_in[k - 2]));  // the DMA out of this slot has finished
    find_runs(k);
    std::vector<t2fit::CopyPool::Row> rows;
    for (const auto& r : runs[k]) {
      const size_t nb = (size_t)(r.second - r.first);
      if (layout == T2FIT_LAYOUT_TE_MAJOR) {  // n_te rows of `len` samples out of planes of n_vox
        for (int i = 0; i < n_te; ++i)
          rows.push_back({stage + ((size_t)i * len + r.first) * 4, echoes + (size_t)i * n_vox + lo + r.first, nb * 4});
      } else {
        rows.push_back({stage + (size_t)r.first * n_te * 4, echoes + (size_t)(lo + r.first) * n_te, nb * n_te * 4});
      }
    }
    if (mask) rows.push_back({stage + (size_t)len * n_te * 4, mask + lo, (size_t)len});
    c->pool->copy(rows);
    float* d_e = (float*)buf + (size_t)lo * n_te;  // this slab's block of the device stack
    T2_HIP_C(hipMemcpyAsync(d_e, stage, (size_t)len * n_te * 4, hipMemcpyHostToDevice, c->s_in));
    uint8_t* dmask = nullptr;
    if (mask) {
      dmask = (uint8_t*)(buf + off_mask) + lo;
      T2_HIP_C(hipMemcpyAsync(dmask, stage + (size_t)len * n_te * 4, (size_t)len, hipMemcpyHostToDevice, c->s_in));
    }
    T2_HIP_C(hipEventRecord(ev_in[k], c->s_in));
    T2_HIP_C(hipStreamWaitEvent(c->s_fit, ev_in[k], 0));
    const t2fit_maps dm{fm[0] + lo, fm[1] + lo, fm[2] + lo, fm[3] + lo, maps->r2 ? fm[4] + lo : nullptr,
                        maps->fun ? fm[5] + lo : nullptr, maps->nit ? (int32_t*)(buf + off_nit) + lo : nullptr,
                        maps->status ? (uint8_t*)(buf + off_status) + lo : nullptr,
                        maps->t2_se ? fm[6] + lo : nullptr};
    rc = launch_fit(cfg, d_e, layout, dmask, len, dm, c->s_fit, is_large_volume(n_vox));
    if (rc != T2FIT_OK) { cleanup(); return rc; }
    T2_HIP_C(hipEventRecord(ev_fit[k], c->s_fit));
    // the device -> host copy of the previous slab is queued behind this slab's host -> device copy: both directions
    // share one copy queue, and a queued copy that waits for a kernel would hold up every copy behind it
    if (k >= 1) T2_HIP_C(queue_d2h(k - 1));
    if (k >= 2) T2_HIP_C(finish_out(k - 2));
  }
  T2_HIP_C(queue_d2h(n_slabs - 1));
  if (n_slabs >= 2) T2_HIP_C(finish_out(n_slabs - 2));
  T2_HIP_C(finish_out(n_slabs - 1));
  return T2FIT_OK;
}

// The same seam without a context of the caller's: a per-device default context, created on first use and kept
// for the life of the process.
int t2fit_volume_host(const t2fit_config* cfg, const float* echoes, int layout, const uint8_t* mask, int64_t n_vox,
                      const t2fit_maps* maps, int device) {
  static std::mutex m;
  static std::vector<t2fit_context*> ctxs;
  t2fit_context* c = nullptr;
  {
    std::lock_guard<std::mutex> g(m);
    if (device >= 0 && (size_t)device < ctxs.size()) c = ctxs[device];
    if (!c) {
      const int rc = t2fit_create(device, &c);
      if (rc != T2FIT_OK) return rc;
      if ((size_t)device >= ctxs.size()) ctxs.resize(device + 1, nullptr);
      ctxs[device] = c;
    }
  }
  return t2fit_context_volume_host(c, cfg, echoes, layout, mask, n_vox, maps);
}

static int voxels_host_impl(const t2fit_config* cfg, const float* echoes, int layout, int64_t n_vox, const int64_t* idx,
                            int64_t n_idx, double* x, double* fun, int32_t* nit, uint8_t* status, int cap,
                            double* trace_x, int32_t* trace_len, int device) {
  int rc = check_common(cfg, echoes, layout, n_vox);
  if (rc != T2FIT_OK) return rc;
  if (n_idx < 0 || (n_idx > 0 && (!idx || !x))) return fail(T2FIT_E_INVALID, "idx/x must be non-NULL");
  if (cap < 0 || (cap > 0 && (!trace_x || !trace_len))) return fail(T2FIT_E_INVALID, "trace buffers must be non-NULL");
  if (n_idx == 0) return T2FIT_OK;
  const int n_te = cfg->n_te;
  // gather the requested rows into a compact voxel-major block on the host
  std::vector<float> rows((size_t)n_idx * n_te);
  for (int64_t r = 0; r < n_idx; ++r) {
    const int64_t v = idx[r];
    if (v < 0 || v >= n_vox) return fail(T2FIT_E_INVALID, "voxel index out of range");
    for (int i = 0; i < n_te; ++i)
      rows[(size_t)r * n_te + i] =
          layout == T2FIT_LAYOUT_TE_MAJOR ? echoes[(size_t)i * n_vox + v] : echoes[(size_t)v * n_te + i];
  }
  T2_HIP(hipSetDevice(device));
  auto pad = [](size_t b) { return align_up(b, 256); };
  const size_t nb_e = rows.size() * sizeof(float);
  const size_t off_x = pad(nb_e);
  const size_t off_f = off_x + pad((size_t)n_idx * 24);
  const size_t off_maps = off_f + pad((size_t)n_idx * 8);
  const size_t map_b = pad((size_t)n_idx * 4);
  const size_t off_nit = off_maps + 4 * map_b;
  const size_t off_status = off_nit + map_b;
  const size_t off_tlen = off_status + pad((size_t)n_idx);
  const size_t off_trace = off_tlen + map_b;
  const size_t total = off_trace + pad((size_t)n_idx * cap * 32);
  char* buf = nullptr;
  T2_HIP(hipMalloc((void**)&buf, total));
  auto cleanup = [&]() { (void)hipFree(buf); };
  T2_HIP_C(hipMemcpy(buf, rows.data(), nb_e, hipMemcpyHostToDevice));
  const t2fit_maps dm{(float*)(buf + off_maps), (float*)(buf + off_maps + map_b), (float*)(buf + off_maps + 2 * map_b),
                      (float*)(buf + off_maps + 3 * map_b), nullptr, nullptr, (int32_t*)(buf + off_nit),
                      (uint8_t*)(buf + off_status), nullptr};
  VoxelOutputs vox{(double*)(buf + off_x), (double*)(buf + off_f)};
  if (cap > 0) {
    T2_HIP_C(hipMemset(buf + off_tlen, 0, map_b));
    vox.trace = (double*)(buf + off_trace);
    vox.trace_len = (int32_t*)(buf + off_tlen);
    vox.trace_cap = cap;
  }
  rc = launch_fit(cfg, (const float*)buf, T2FIT_LAYOUT_VOXEL_MAJOR, nullptr, n_idx, dm, nullptr, false, vox);
  if (rc != T2FIT_OK) { cleanup(); return rc; }
  T2_HIP_C(hipDeviceSynchronize());
  T2_HIP_C(hipMemcpy(x, buf + off_x, (size_t)n_idx * 24, hipMemcpyDeviceToHost));
  if (fun) T2_HIP_C(hipMemcpy(fun, buf + off_f, (size_t)n_idx * 8, hipMemcpyDeviceToHost));
  if (nit) T2_HIP_C(hipMemcpy(nit, buf + off_nit, (size_t)n_idx * 4, hipMemcpyDeviceToHost));
  if (status) T2_HIP_C(hipMemcpy(status, buf + off_status, (size_t)n_idx, hipMemcpyDeviceToHost));
  if (cap > 0) {
    T2_HIP_C(hipMemcpy(trace_x, buf + off_trace, (size_t)n_idx * cap * 32, hipMemcpyDeviceToHost));
    T2_HIP_C(hipMemcpy(trace_len, buf + off_tlen, (size_t)n_idx * 4, hipMemcpyDeviceToHost));
  }
  cleanup();
  return T2FIT_OK;
}

int t2fit_voxels_host(const t2fit_config* cfg, const float* echoes, int layout, int64_t n_vox, const int64_t* idx,
                      int64_t n_idx, double* x, double* fun, int32_t* nit, uint8_t* status, int device) {
  return voxels_host_impl(cfg, echoes, layout, n_vox, idx, n_idx, x, fun, nit, status, 0, nullptr, nullptr, device);
}

int t2fit_voxels_trace_host(const t2fit_config* cfg, const float* echoes, int layout, int64_t n_vox,
                            const int64_t* idx, int64_t n_idx, double* x, double* fun, int32_t* nit, uint8_t* status,
                            int trace_cap, double* trace, int32_t* trace_len, int device) {
  if (trace_cap < 1) return fail(T2FIT_E_INVALID, "trace_cap must be >= 1");
  return voxels_host_impl(cfg, echoes, layout, n_vox, idx, n_idx, x, fun, nit, status, trace_cap, trace, trace_len,
                          device);
}

}  // extern "C"

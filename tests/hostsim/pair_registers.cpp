// pair_registers.cpp -- TEST INFRASTRUCTURE (see hostsim.cpp): the reference-trajectory lane solver with the last ratio
// of every correction pair in members of the solver (Lbfgsb<.., PAIRS_REG>, what the one-wave-workgroup kernels run)
// beside the form with the whole ring in one array (PAIRS_LDS), row by row, with the solver's own counters.  Built by
// tests/test_pair_registers_hostsim.py into tests/hostsim/libt2fit_pair_registers.so.
#include "../../fetal_t2mapping_amd/csrc/t2fit_config.h"
#include "../../fetal_t2mapping_amd/csrc/t2fit_dispatch.h"

using namespace t2fit;

namespace {

struct RowOut {
  double x[3], fun;
  int32_t nit, nfev, status;
  int32_t col_end, n_drop, n_reset;  // pairs held at the end; times the oldest pair was dropped, the memory was dropped
  int32_t trace_len;
};

// one row through Lbfgsb<MODEL, NTE, HOME>; trace: cap x 4 doubles (x0, x1, x2, f per iteration)
template <int MODEL, int NTE, int HOME>
int run_row(const LaneParams& P, const float* row, RowOut& o, double* trace, int cap) {
  float buf[T2FIT_MAX_TE];
  for (int i = 0; i < P.n_te; ++i) buf[i] = row[i];
  bool finite;
  float y0_raw;
  ObjCtx c = prepare_samples(P, buf, 1, finite, y0_raw);
  double lb[3], ub[3];
  if (!lane_bounds(P, y0_raw, lb, ub) || !finite) return -10;
  int n_trace = 0;
  c.trace = trace; c.trace_cap = cap; c.trace_n = &n_trace;
  using S = Lbfgsb<MODEL, NTE, HOME>;
  static_assert(HOME == PAIRS_LDS ? !S::kSplit : S::kPairRegs, "the two forms under comparison");
  S s;
  double hist[S::M * S::PAIR] = {};
  s.init(P.x0, lb, ub, hist, 1);
  for (int i = 0; i < NTE; ++i) s.ys[i] = c.sample(i);
  int drops = 0;
  bool done;
  do {
    s.eval(c);
    const int head0 = s.head;
    done = s.advance(c);
    // (`head` moves in one place only, digest() dropping the oldest pair of a full ring; dropping the whole memory sets
    // col = 0 and leaves it alone, so restarts are not counted here; at most one pair is stored per evaluation)
    if (s.head != head0) ++drops;
  } while (!done);
  LaneResult r;
  s.result(r);
  for (int j = 0; j < 3; ++j) o.x[j] = r.x[j];
  o.fun = r.fun; o.nit = r.nit; o.nfev = r.nfev; o.status = r.status;
  o.col_end = s.col; o.n_drop = drops; o.n_reset = s.n_reset; o.trace_len = n_trace;
  return 0;
}

template <int MODEL, int HOME>
int run_nte(const LaneParams& P, const float* row, RowOut& o, double* trace, int cap) {
  switch (P.n_te) {
    case 3: return run_row<MODEL, 3, HOME>(P, row, o, trace, cap);
    case 6: return run_row<MODEL, 6, HOME>(P, row, o, trace, cap);
    case 8: return run_row<MODEL, 8, HOME>(P, row, o, trace, cap);
  }
  return -2;
}

}  // namespace

// rows: (n, nTE) float32.  home: 0 = whole ring in one array, 1 = last ratio in members.  out: n records of 14 doubles
// (x0, x1, x2, fun, nit, nfev, status, col_end, n_drop, n_reset, trace_len, rc, 0, 0); trace: n x cap x 4 doubles.
extern "C" int hostsim_pairs_fit_rows(const t2fit_config* cfg, const float* rows, int64_t n, int home, double* out,
                                      double* trace, int cap) {
  const char* why;
  int rc = config_check(cfg, &why);
  if (rc != T2FIT_OK) return rc;
  if (cfg->solver != T2FIT_SOLVER_LBFGSB || cfg->model == T2FIT_MODEL_GAUSSIAN) return -1;
  const LaneParams P = make_lane_params(*cfg);
  for (int64_t v = 0; v < n; ++v) {
    RowOut o = {};
    const float* row = rows + v * cfg->n_te;
    double* tr = trace + (size_t)v * cap * 4;
    int e;
    if (cfg->model == T2FIT_MODEL_GAUSSIAN_RICIAN)
      e = home ? run_nte<T2FIT_MODEL_GAUSSIAN_RICIAN, PAIRS_REG>(P, row, o, tr, cap)
               : run_nte<T2FIT_MODEL_GAUSSIAN_RICIAN, PAIRS_LDS>(P, row, o, tr, cap);
    else
      e = home ? run_nte<T2FIT_MODEL_RICIAN, PAIRS_REG>(P, row, o, tr, cap)
               : run_nte<T2FIT_MODEL_RICIAN, PAIRS_LDS>(P, row, o, tr, cap);
    if (e == -2) return e;
    double* d = out + 14 * v;
    d[0] = o.x[0]; d[1] = o.x[1]; d[2] = o.x[2]; d[3] = o.fun;
    d[4] = o.nit; d[5] = o.nfev; d[6] = o.status; d[7] = o.col_end; d[8] = o.n_drop; d[9] = o.n_reset;
    d[10] = o.trace_len; d[11] = e; d[12] = 0.0; d[13] = 0.0;
  }
  return 0;
}

// store_s / load_s of the member form: `n` vectors of three components pushed one after the other (the ring fills,
// then drops its oldest pair at every push, as digest() does it), each read back right after its push and every pair
// still held read back again after the last push.  s_out: what came back after each push; held: M x 3, oldest first,
// unused rows zero.  Returns the number of pairs held.
extern "C" int hostsim_pairs_roundtrip(const double* s_in, int64_t n, double* s_out, double* held) {
  using S = Lbfgsb<T2FIT_MODEL_GAUSSIAN_RICIAN, 0, PAIRS_REG>;
  S s;
  double hist[S::M * S::PAIR_L] = {};
  s.hist = hist; s.hstride = 1; s.head = 0; s.col = 0;
  for (int64_t v = 0; v < n; ++v) {
    if (s.col == S::M) { s.head = (s.head + 1) % S::M; s.col = S::M - 1; }
    const int q = s.slot_of(s.col);
    s.store_s(q, s_in + 3 * v);
    ++s.col;
    s.load_s(q, s_out + 3 * v);
  }
  for (int p = 0; p < S::M; ++p)
    for (int j = 0; j < 3; ++j) held[3 * p + j] = 0.0;
  for (int p = 0; p < s.col; ++p) s.load_s(s.slot_of(p), held + 3 * p);
  return s.col;
}

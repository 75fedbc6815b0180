// Host build of the bookkeeping of the batched p-Laplace Jacobi iteration (csrc/lp_plan.h) for tests/test_plaplace_host.py: the plan
// (vertex blocks, invdeg, dt, start values, boundary map), and the chunked two-buffer schedule with its per-chunk error slots and
// per-column stops, a plain loop over (vertex, column) standing in for the kernel of plaplace.hip.  The chunk length is an argument, so
// that the carry of the last slot into the next chunk is exercised.  Compile with -ffp-contract=off.
#include "../graphlearning_amd/csrc/lp_plan.h"

extern "C" void lpb_constants(int64_t* out) {
  out[0] = LP_BLOCK;
  out[1] = LP_BATCH_CHUNK;
  out[2] = LP_LDS_COLS;
  out[3] = LP_MAX_COLS;
}

extern "C" int64_t lpb_result_iterate(int64_t stop, int64_t T) { return lp_result_iterate(stop, T); }

// start_out (n + 1), invdeg_out (n), bdy_out (n), hi_out / lo_out (B), scal_out: alpha, delta, dt.  Returns lp_make_plan's code.
extern "C" int lpb_plan(int64_t n, int64_t M, const int32_t* nbr, const int32_t* row, const double* W, int B, int64_t m, const int32_t* ind,
                        const double* val, double p, int64_t T, int64_t* start_out, double* invdeg_out, int32_t* bdy_out, double* hi_out,
                        double* lo_out, double* scal_out) {
  LpPlan P;
  char msg[200];
  const int rc = lp_make_plan(n, M, nbr, row, W, B, m, ind, val, p, T, &P, msg, sizeof msg);
  if (rc) return rc;
  for (int64_t i = 0; i <= n; ++i) start_out[i] = P.start[i];
  for (int64_t i = 0; i < n; ++i) { invdeg_out[i] = P.invdeg[i]; bdy_out[i] = P.bdy[i]; }
  for (int b = 0; b < B; ++b) { hi_out[b] = P.hi[b]; lo_out[b] = P.lo[b]; }
  scal_out[0] = P.alpha;
  scal_out[1] = P.delta;
  scal_out[2] = P.dt;
  return 0;
}

namespace {
struct Rec { double x, y; };

// what one thread of the kernel does for (vertex i, column b) of iteration `it`, slot r of the chunk
void visit(const Rec* xin, Rec* xout, const LpPlan& P, const int32_t* nbr, const double* W, const double* val, int B, int64_t i, int b,
           int64_t it, int r, double tol, unsigned long long* err) {
  if (lp_frozen(it, err[(size_t)(r - 1) * B + b], tol)) return;
  const Rec me = xin[i * B + b];
  double minu = 0, maxu = 0, sumu = 0, minl = 0, maxl = 0, suml = 0;
  for (int64_t j = P.start[i]; j < P.start[i + 1]; ++j) {
    const Rec x = xin[(int64_t)nbr[j] * B + b];
    const double w = W[j];
    const double tu = w * (x.x - me.x);
    minu = (tu < minu) ? tu : minu;
    maxu = (tu > maxu) ? tu : maxu;
    sumu = sumu + tu;
    const double tl = w * (x.y - me.y);
    minl = (tl < minl) ? tl : minl;
    maxl = (tl > maxl) ? tl : maxl;
    suml = suml + tl;
  }
  Rec out;
  out.x = me.x + P.dt * (P.invdeg[i] * sumu + P.delta * (minu + maxu));
  out.y = me.y + P.dt * (P.invdeg[i] * suml + P.delta * (minl + maxl));
  if (P.bdy[i] >= 0) out.x = out.y = val[(int64_t)P.bdy[i] * B + b];
  xout[i * B + b] = out;
  const double gap = me.x - me.y;
  if (gap > 0.0) {
    const unsigned long long e = __builtin_bit_cast(unsigned long long, gap);
    unsigned long long& slot = err[(size_t)r * B + b];
    if (e > slot) slot = e;
  }
}
}  // namespace

// uu, ul (n, B): the content of the first buffer; iters (B).  chunk >= 1: iterations between two reads of the slots.  The vertices are
// walked backwards (the order inside an iteration must not matter).  Returns lp_make_plan's code.
extern "C" int lpb_run(int64_t n, int64_t M, const int32_t* nbr, const int32_t* row, const double* W, int B, int64_t m, const int32_t* ind,
                       const double* val, double p, int64_t T, double tol, int chunk, double* uu, double* ul, int64_t* iters) {
  LpPlan P;
  char msg[200];
  const int rc = lp_make_plan(n, M, nbr, row, W, B, m, ind, val, p, T, &P, msg, sizeof msg);
  if (rc) return rc;
  const int64_t total = n * B;
  const double poison = __builtin_bit_cast(double, 0x7ff8dead0000beefull);
  std::vector<Rec> a((size_t)total), bb((size_t)total, Rec{poison, poison});      // the second buffer is never read before it is written
  for (int64_t i = 0; i < n; ++i)
    for (int b = 0; b < B; ++b) {
      Rec v;
      if (P.bdy[i] >= 0) v.x = v.y = val[(int64_t)P.bdy[i] * B + b];
      else { v.x = P.hi[b]; v.y = P.lo[b]; }
      a[i * B + b] = v;
    }
  std::vector<unsigned long long> slots((size_t)(chunk + 1) * B, 0xffffffffffffffffull);      // cleared by lp_slots_next before use
  LpStops stops(B, T, tol);
  for (int len; (len = stops.next_len(chunk)) > 0;) {
    lp_slots_next(slots.data(), B, chunk, stops.prev_len);
    for (int r = 1; r <= len; ++r) {
      const int64_t it = stops.it + r - 1;
      const Rec* xin = (it & 1) ? bb.data() : a.data();
      Rec* xout = (it & 1) ? a.data() : bb.data();
      for (int64_t i = n - 1; i >= 0; --i)
        for (int b = 0; b < B; ++b) visit(xin, xout, P, nbr, W, val, B, i, b, it, r, tol, slots.data());
    }
    stops.decide(slots.data() + B, len);
  }
  for (int64_t q = 0; q < total; ++q) { uu[q] = a[q].x; ul[q] = a[q].y; }
  for (int b = 0; b < B; ++b) iters[b] = stops.iters(b);
  return 0;
}

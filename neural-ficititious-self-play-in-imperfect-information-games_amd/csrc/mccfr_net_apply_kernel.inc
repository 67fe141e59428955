// The text of k_mccfr_net_apply and of k_mccfr_net_apply_w<H> (mccfr.hip), included as the kernel's
// body.  In scope where it is included: NetApplyArgs A, and the width's names H, NP, ZS, OW2, OB2
// (nn's and fit_step.h's at 64, FIT_WIDTH_NAMES elsewhere).
#pragma clang fp contract(off)
  using namespace nfsp::fit;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int seat = blockIdx.x, run = blockIdx.y;
  const int tid = threadIdx.x;
  const bool fits = A.fitseat == 2 || A.fitseat == seat;
  const NetDevCfg C = A.net[run];
  const int N = A.nrows[seat] * 3;
  const int nmax = (A.nrows[0] > A.nrows[1] ? A.nrows[0] : A.nrows[1]) * 3;
  const FitLds S = fit_carve<H>(smem_raw, (nmax + 3) & ~3);
  const float lr = C.lr, mu = C.mu;
  const int head = NFSP_ACT_LINEAR, loss = C.loss;
  const size_t n9 = (size_t)A.ndec * 9;
  float* gw = A.w + ((size_t)run * 2 + seat) * NP;
  float* gv = A.v + ((size_t)run * 2 + seat) * NP;
  const long long* R = A.state + (size_t)run * 4 * n9;
  const double den = ((double)A.cfg[run].walkers * Q) * A.tw;
  const float what = (float)(1.0 / (double)N);

  for (int e = tid; e < NP; e += FIT_WG) {
    S.w[e] = gw[e];
    S.v[e] = gv[e];
  }
  for (int b = tid; b < N; b += FIT_WG) {
    const int c = b / 3, r = b - c * 3;
    const int d = A.rows[seat * FIT_SEAT_ROWS + c];
    const int sid = d * 3 + r;
    const bool raise = A.legal[d] & 1;
    S.x[b] = A.obs[sid];
    S.wh[b] = what;
    const long long r0 = R[sid * 3], r1 = R[sid * 3 + 1], r2 = raise ? R[sid * 3 + 2] : 0;
    double y0, y1, y2;
    if (C.target == NFSP_MCCFR_NET_TARGET_AVG) {
      y0 = (double)r0 / den;
      y1 = (double)r1 / den;
      y2 = (double)r2 / den;
    } else {
      const long long a0 = r0 < 0 ? -r0 : r0, a1 = r1 < 0 ? -r1 : r1, a2 = r2 < 0 ? -r2 : r2;
      const long long m01 = a0 > a1 ? a0 : a1, m = m01 > a2 ? m01 : a2;
      y0 = m ? (double)r0 / (double)m : 0.0;
      y1 = m ? (double)r1 / (double)m : 0.0;
      y2 = m ? (double)r2 / (double)m : 0.0;
    }
    S.t[3 * b] = (float)y0;
    S.t[3 * b + 1] = (float)y1;
    S.t[3 * b + 2] = raise ? (float)y2 : 0.f;
    S.m[3 * b] = 1.f;
    S.m[3 * b + 1] = 1.f;
    S.m[3 * b + 2] = raise ? 1.f : 0.f;
  }
  __syncthreads();

  if (fits) {                                        // the workgroup's: uniform
    fit_forward<H>(S, N);
    fit_rows(S, N, head, loss);
    if (tid == 0) {
      double L = 0.0;
      for (int b = 0; b < N; ++b) L += (double)S.lt[b];
      A.loss[((size_t)run * 2 + seat) * 2] = L;
    }
    for (int s = 0; s < C.steps; ++s) {              // the run's: uniform
#include "fit_step_body.inc"
    }
  }

  fit_forward<H>(S, N);
  if (fits) {
    fit_rows(S, N, head, loss);
    if (tid == 0) {
      double L = 0.0;
      for (int b = 0; b < N; ++b) L += (double)S.lt[b];
      A.loss[((size_t)run * 2 + seat) * 2 + 1] = L;
    }
    for (int e = tid; e < NP; e += FIT_WG) {
      gw[e] = S.w[e];
      gv[e] = S.v[e];
    }
  }
  for (int b = tid; b < N; b += FIT_WG) {
    const int c = b / 3, r = b - c * 3;
    const int d = A.rows[seat * FIT_SEAT_ROWS + c];
    const size_t at = ((size_t)d * 3 + r) * 3;      // < n9
    const bool raise = A.legal[d] & 1;
    double rp[3];
    for (int k = 0; k < 3; ++k) {
      const float z = S.o[3 * b + k];
      A.z[(size_t)run * n9 + at + k] = z;
      rp[k] = (double)z > 0.0 ? (double)z : 0.0;
    }
    if (!raise) rp[2] = 0.0;
    average_row(rp, raise, A.tabs + (size_t)run * 2 * n9 + at);
  }

// The text of k_fit_tables and of k_fit_tables_w<H> (fit_tables.hip), included as the kernel's
// body.  In scope where it is included: FitArgs A, and the width's names H, NP, ZS, OW2, OB2 (nn's
// and fit_step.h's at 64, FIT_WIDTH_NAMES elsewhere).
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const FitDevJob J = A.jobs[blockIdx.x];
  const int tid = threadIdx.x;
  const int N = A.nrows[J.seat] * 3;
  const int nmax = (A.nrows[0] > A.nrows[1] ? A.nrows[0] : A.nrows[1]) * 3;
  const FitLds S = fit_carve<H>(smem_raw, (nmax + 3) & ~3);
  const float lr = J.lr, mu = J.mu;
  const int head = J.head, loss = J.loss;

  for (int e = tid; e < NP; e += FIT_WG) {
    S.w[e] = J.w[e];
    S.v[e] = J.v ? J.v[e] : 0.f;
  }
  for (int b = tid; b < N; b += FIT_WG) {
    const int c = b / 3, r = b - c * 3;
    const int d = A.rows[J.seat * FIT_SEAT_ROWS + c];
    const int sid = d * 3 + r;
    const bool raise = A.legal[d] & 1;
    S.x[b] = A.obs[sid];
    S.wh[b] = (float)((J.weight ? J.weight[sid] : 1.0) / J.wsum);
    for (int k = 0; k < 3; ++k) {
      S.t[3 * b + k] = (float)J.target[sid * 3 + k];
      S.m[3 * b + k] = J.mask ? (J.mask[sid * 3 + k] ? 1.f : 0.f) : (k < 2 || raise ? 1.f : 0.f);
    }
  }
  __syncthreads();

  fit_forward<H>(S, N);
  fit_rows(S, N, J.head, J.loss);
  if (tid == 0) {
    double L = 0.0;
    for (int b = 0; b < N; ++b) L += (double)S.lt[b];
    A.loss[2 * blockIdx.x] = L;
  }

  for (int64_t s = 0; s < A.steps; ++s) {          // the launch's: uniform
#include "fit_step_body.inc"
  }

  fit_forward<H>(S, N);
  fit_rows(S, N, J.head, J.loss);
  if (tid == 0) {
    double L = 0.0;
    for (int b = 0; b < N; ++b) L += (double)S.lt[b];
    A.loss[2 * blockIdx.x + 1] = L;
  }
  for (int e = tid; e < NP; e += FIT_WG) {
    J.w[e] = S.w[e];
    if (J.v) J.v[e] = S.v[e];
  }

// The body of one full-batch step (fit_step.h states it), included inside the step loop of
// k_fit_tables and k_mccfr_net_apply.  In scope where it is included: FitLds S; int N, the net's
// row count; int tid = threadIdx.x; int head, loss; float lr, mu -- all but tid uniform over the
// workgroup; and the width's names H, ZS, OW2, OB2 (nn's and fit_step.h's at 64, FIT_WIDTH_NAMES
// elsewhere).  Every loop runs to N; ends behind a barrier.
  fit_forward<H>(S, N);
  fit_rows(S, N, head, loss);
  float g2 = 0.f;
  int w2i = -1;
  if (tid < H * NA) {
    const int j = tid / NA, k = tid - j * NA;
    for (int b = 0; b < N; ++b) {
      const float z = S.z[b * ZS + j];
      g2 = g2 + (z > 0.f ? z : 0.f) * S.dz[3 * b + k];
    }
    w2i = OW2 + tid;
  } else if (tid < H * NA + NA) {
    const int k = tid - H * NA;
    for (int b = 0; b < N; ++b) g2 = g2 + S.dz[3 * b + k];
    w2i = OB2 + k;
  }
  __syncthreads();
  for (int e = tid; e < N * H; e += FIT_WG) {     // z1 <- dz1 in place, W2 still the old one
    const int b = e / H, j = e - b * H;
    const float dh = (S.dz[3 * b] * S.w[OW2 + j * 3] + S.dz[3 * b + 1] * S.w[OW2 + j * 3 + 1]) +
                     S.dz[3 * b + 2] * S.w[OW2 + j * 3 + 2];
    S.z[b * ZS + j] = S.z[b * ZS + j] > 0.f ? dh : 0.f;
  }
  __syncthreads();
  if (w2i >= 0) {
    const float vv = mu * S.v[w2i] + g2;
    S.v[w2i] = vv;
    S.w[w2i] = S.w[w2i] - lr * vv;
  }
  for (int e = tid; e < OBS * H + H; e += FIT_WG) {
    float g = 0.f;
    if (e < OBS * H) {
      const int i = e / H, j = e - i * H;          // i is the wave's: the branch is uniform
      for (int b = 0; b < N; ++b)
        if ((S.x[b] >> i) & 1u) g = g + S.z[b * ZS + j];
    } else {
      const int j = e - OBS * H;
      for (int b = 0; b < N; ++b) g = g + S.z[b * ZS + j];
    }
    const float vv = mu * S.v[e] + g;
    S.v[e] = vv;
    S.w[e] = S.w[e] - lr * vv;
  }
  __syncthreads();

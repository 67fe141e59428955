// The body of k_br_targets (learner.hip): one BR update's targets -- the Q_target forwards of
// its 128 rows, TD values, the proxy, the row-0 quirk and its step records.  Included by the
// kernel (one workgroup per update) and by br_targets_item (br_targets.h: the persistent group
// BR kernel's helper workgroups).  In scope: J (TargetJob), bx (update within the segment), B,
// E, gamma, quirks, lr0, and br_targets.h's emit_recs.
  // threads 0..127: Q_target(s) of row b (waves 0-1); threads 128..255: Q_target(s2) of
  // row b - 128 (waves 2-3) -- the two forwards of a row run side by side
  __shared__ __attribute__((aligned(16))) float sw[NET_LDS];
  __shared__ float q[MAX_BATCH][3];
  __shared__ float val[MAX_BATCH];
  __shared__ uint32_t sb[MAX_BATCH];
  __shared__ uint8_t am[MAX_BATCH];
  __shared__ double part[2];
  __shared__ int lastw[2][3];
  if (bx >= J.n) return;                              // block-uniform
  const int tid = threadIdx.x;
  const int b = tid & (MAX_BATCH - 1);
  const bool s2half = tid >= MAX_BATCH;
  const int64_t u = J.u0 + bx;
  BrRow rr{};
  if (b < B) rr = J.rows[u * B + b];
  // the records of epoch e are emitted by threads 128 (e & 1) .. + 127 (below); their fit
  // order is loaded now, beside the net
  const int half = tid >> 7;
  int pk[2] = {0, 0};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int e = half + 2 * k;
    if (e < E && b < B) pk[k] = J.perm[(u * E + e) * B + b];
  }
  stage_net_lds(sw, J.tw, tid, blockDim.x);
  __syncthreads();
  if (b < B) {
    float y[3];
    if (!s2half) {
      fwd_lds(sw, rr.s, br_act(quirks), y);
      q[b][0] = y[0]; q[b][1] = y[1]; q[b][2] = y[2];
      am[b] = (uint8_t)(rr.meta & 0xFFu);
      sb[b] = rr.s;
    } else {
      fwd_lds(sw, rr.s2, br_act(quirks), y);
      const float qmax = fmaxf(fmaxf(y[0], y[1]), y[2]);
      const float r = (float)(int8_t)((rr.meta >> 16) & 0xFFu) * 0.5f;
      const bool terminal = !(quirks & NFSP_QUIRK_TERMINAL_BOOTSTRAP) && ((rr.meta >> 8) & 1u);
      val[b] = (float)(terminal ? (double)r : (double)r + gamma * (double)qmax);
    }
  }
  __syncthreads();
  const int lane = tid & 63, wv = tid >> 6;
  if (!s2half) {
    // exploitability proxy (agent/agent.py:235-238): mean of the row maxima, before the
    // row-0 overwrite; and for the quirk, the last row k with argmax a_k == action
    double m = b < B ? (double)fmaxf(fmaxf(q[b][0], q[b][1]), q[b][2]) : 0.0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m += __shfl_xor(m, off);
    if (lane == 0) part[wv] = m;
#pragma unroll
    for (int act = 0; act < 3; ++act) {
      const unsigned long long bal = __ballot(b < B && am[b] == act);
      if (lane == 0) lastw[wv][act] = bal ? 64 * wv + 63 - __builtin_clzll(bal) : -1;
    }
  }
  __syncthreads();
  if (tid == 0) J.expl[u] = (part[0] + part[1]) / B;
  if (quirks & NFSP_QUIRK_ROW0_TARGET) {
    if (tid < 3) {       // target[0][argmax a_k] = v_k for k = 0..B-1: the last k wins
      const int last = lastw[1][tid] >= 0 ? lastw[1][tid] : lastw[0][tid];
      if (last >= 0) q[0][tid] = val[last];
    }
  } else if (!s2half && b < B) {
    q[b][am[b]] = val[b];
  }
  __syncthreads();
  // lr of this update: lr0 / (1 + 0.003 sqrt(iteration)) with iteration = it0 + 2 u
  // (agent/agent.py:249, iteration += 2 per BR update), in the reference's double arithmetic
  const float lr = (float)(lr0 / (1.0 + 0.003 * sqrt((double)(J.it0 + 2 * u))));
  // epochs in pairs: threads 0..127 emit epoch e, threads 128..255 epoch e + 1
  for (int e = half, k = 0; e < E; e += 2, ++k) {
    uint32_t x = 0;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
    if (b < B) {
      const int r = k < 2 ? pk[k] : J.perm[(u * E + e) * B + b];
      x = sb[r];
      t0 = q[r][0]; t1 = q[r][1]; t2 = q[r][2];
    }
    emit_recs(J.rec + (u * E + e) * (B / CHAIN_MB), x, t0, t1, t2, lr, B, b);
  }

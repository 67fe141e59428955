// Nets fitted to tables (include/nfsp.h nfsp_fit_tables): a deterministic, weighted,
// full-batch gradient descent of packed 30-64-3 nets on the rows of the evaluator's tree
// (exploit_tree.h obs[ndec][3]), the way the evaluators are built: one workgroup per job, every
// step of the run inside one launch, everything in LDS.  The reference has nothing like it: its
// nets only ever see sampled minibatches (agent/agent.py:209-264).
//
// Per step, f32 with fp contract off, every gradient from the weights before the step:
//   z1[b][j]  = (sum over the SET bits i of obs[b], ascending, of W1[i][j]) + b1[j]
//               -- the bits of sgd_step's 30-input sum for finite weights: x is 0 or 1, and adding
//               0 * w = +-0 to a sum that started at +0 changes no bit
//   z[b][k]   = (sum over j ascending of relu(z1[b][j]) * W2[j][k]) + b2[k]
//   dz[b][k]  per row, as include/nfsp.h states for the (head, loss) pair
//   dW2[j][k] = sum over rows b ascending of relu(z1[b][j]) * dz[b][k];  db2[k] = sum_b dz[b][k]
//   dz1[b][j] = z1[b][j] > 0 ? (dz[b][0] W2[j][0] + dz[b][1] W2[j][1]) + dz[b][2] W2[j][2] : 0
//   dW1[i][j] = sum over the rows b with bit i set, ascending, of dz1[b][j];  db1[j] = sum_b dz1[b][j]
//   v <- mu v + g,  w <- w - lr v
// Every sum starts at +0 and runs in the order above, fixed by the job alone: one thread owns one
// parameter, so no partial sums, no atomics, and neither the grid nor the job's place in it enters.
// A zero-weight row and a masked entry contribute dz = +-0 and change no bit.
//
// Barriers: the step loop runs to A.steps and every loop inside a phase to the job's row count,
// both uniform over the workgroup; the two single-thread regions (the loss sums) lie outside the
// step loop.
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "exploit_tree.h"
#include "nn_device.h"

using namespace nfsp::nn;
using nfsp::NA;
using nfsp::OBS;

namespace {

constexpr int FIT_WG = 512;
constexpr int FIT_SEAT_ROWS = 128;            // decision rows of one seat (Leduc: 65, Kuhn: 4)
constexpr int ZS = H + 1;                     // z1's row stride: breaks the 64-float stride of column walks
constexpr int NPP = (NP + 3) & ~3;            // keeps every carve offset a multiple of 16 bytes
static_assert(FIT_WG >= H * NA + NA, "one W2 / b2 entry per thread");

struct FitDevJob {
  float* w;
  float* v;
  const double* target;
  const double* weight;
  const uint8_t* mask;
  double wsum;                                // sum of the seat's weights, ascending rows, in double
  int32_t seat, head, loss;
  float lr, mu;
  int32_t pad;
};

struct FitArgs {
  const FitDevJob* jobs;
  const int32_t* rows;                        // [2][FIT_SEAT_ROWS]: a seat's decision rows, ascending
  const uint32_t* obs;                        // [ndec][3]
  const uint8_t* legal;                       // [ndec]
  double* loss;                               // [jobs][2]
  int64_t steps;
  int32_t nrows[2];
};

// LDS carve, in floats, for at most nm (a multiple of 4) rows
struct FitLds {
  float *w, *v, *t, *m, *wh, *o, *dz, *lt, *z;
  uint32_t* x;
};
__host__ __device__ inline size_t fit_lds_floats(int nm) { return 2 * (size_t)NPP + (size_t)nm * (3 + 4 * NA + ZS); }
__device__ inline FitLds fit_carve(char* raw, int nm) {
  FitLds S;
  S.w = (float*)raw;
  S.v = S.w + NPP;
  S.x = (uint32_t*)(S.v + NPP);
  S.wh = (float*)(S.x + nm);
  S.lt = S.wh + nm;
  S.t = S.lt + nm;
  S.m = S.t + NA * nm;
  S.o = S.m + NA * nm;
  S.dz = S.o + NA * nm;
  S.z = S.dz + NA * nm;
  return S;
}

// z1 and the raw head sums of every row from the weights in LDS; ends behind a barrier
__device__ inline void fit_forward(const FitLds& S, int N) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  for (int e = tid; e < N * H; e += FIT_WG) {
    const int b = e / H, j = e - b * H;
    uint32_t bits = S.x[b];
    float acc = 0.f;
    while (bits) {
      const int i = __builtin_ctz(bits);
      bits &= bits - 1;
      acc = acc + S.w[OW1 + i * H + j];
    }
    S.z[b * ZS + j] = acc + S.w[OB1 + j];
  }
  __syncthreads();
  for (int e = tid; e < N * NA; e += FIT_WG) {
    const int b = e / NA, k = e - b * NA;
    float acc = 0.f;
    for (int j = 0; j < H; ++j) {
      const float z = S.z[b * ZS + j];
      acc = acc + (z > 0.f ? z : 0.f) * S.w[OW2 + j * NA + k];
    }
    S.o[e] = acc + S.w[OB2 + k];
  }
  __syncthreads();
}

// dz and the loss term of every row from the head sums; ends behind a barrier
__device__ inline void fit_rows(const FitLds& S, int N, int head, int loss) {
#pragma clang fp contract(off)
  for (int b = threadIdx.x; b < N; b += FIT_WG) {
    const float z[3] = {S.o[3 * b], S.o[3 * b + 1], S.o[3 * b + 2]};
    const float t[3] = {S.t[3 * b], S.t[3 * b + 1], S.t[3 * b + 2]};
    const float wh = S.wh[b];
    float d[3], l;
    if (loss == NFSP_FIT_CE) {
      const float mx = fmaxf(fmaxf(z[0], z[1]), z[2]);
      const float c0 = z[0] - mx, c1 = z[1] - mx, c2 = z[2] - mx;
      const float e0 = expf(c0), e1 = expf(c1), e2 = expf(c2);
      const float s = (e0 + e1) + e2;
      const float T = (t[0] + t[1]) + t[2];
      d[0] = wh * ((e0 / s) * T - t[0]);
      d[1] = wh * ((e1 / s) * T - t[1]);
      d[2] = wh * ((e2 / s) * T - t[2]);
      const float ls = logf(s);
      l = -((t[0] * (c0 - ls) + t[1] * (c1 - ls)) + t[2] * (c2 - ls));
    } else {
      float lk[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const bool on = head == NFSP_ACT_LINEAR || z[k] > 0.f;
        const float e = (on ? z[k] : 0.f) - t[k];
        const float a = fabsf(e);
        const bool clip = loss == NFSP_FIT_HUBER && a > 1.0f;
        const float g = clip ? (e > 0.f ? 1.0f : -1.0f) : e;
        d[k] = on ? (wh * S.m[3 * b + k]) * g : 0.f;
        lk[k] = S.m[3 * b + k] * (clip ? a - 0.5f : (0.5f * e) * e);
      }
      l = (lk[0] + lk[1]) + lk[2];
    }
    S.dz[3 * b] = d[0];
    S.dz[3 * b + 1] = d[1];
    S.dz[3 * b + 2] = d[2];
    S.lt[b] = wh * l;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(FIT_WG) k_fit_tables(FitArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const FitDevJob J = A.jobs[blockIdx.x];
  const int tid = threadIdx.x;
  const int N = A.nrows[J.seat] * 3;
  const int nmax = (A.nrows[0] > A.nrows[1] ? A.nrows[0] : A.nrows[1]) * 3;
  const FitLds S = fit_carve(smem_raw, (nmax + 3) & ~3);
  const float lr = J.lr, mu = J.mu;

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

  fit_forward(S, N);
  fit_rows(S, N, J.head, J.loss);
  if (tid == 0) {
    double L = 0.0;
    for (int b = 0; b < N; ++b) L += (double)S.lt[b];
    A.loss[2 * blockIdx.x] = L;
  }

  for (int64_t s = 0; s < A.steps; ++s) {          // the launch's: uniform
    fit_forward(S, N);
    fit_rows(S, N, J.head, J.loss);
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
  }

  fit_forward(S, N);
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
}

std::string job_name(int k) { return "nfsp_fit job " + std::to_string(k); }

int check_job(const nfsp_fit_job& j, int k) {
  const std::string who = job_name(k);
  if (!j.dev_w || !j.dev_target) return nfsp::fail(NFSP_EINVAL, who + ": null dev_w or dev_target");
  if (j.seat != 0 && j.seat != 1) return nfsp::fail(NFSP_EINVAL, who + ": seat must be 0 or 1");
  if (j.head != NFSP_ACT_RELU && j.head != NFSP_ACT_SOFTMAX && j.head != NFSP_ACT_LINEAR)
    return nfsp::fail(NFSP_EINVAL, who + ": bad head");
  if (j.loss != NFSP_FIT_CE && j.loss != NFSP_FIT_MSE && j.loss != NFSP_FIT_HUBER)
    return nfsp::fail(NFSP_EINVAL, who + ": bad loss");
  if ((j.loss == NFSP_FIT_CE) != (j.head == NFSP_ACT_SOFTMAX))
    return nfsp::fail(NFSP_EINVAL, who + ": head and loss do not pair (CE needs the softmax head, MSE and Huber "
                                         "the ReLU or linear head)");
  if (j.loss == NFSP_FIT_CE && j.dev_mask) return nfsp::fail(NFSP_EINVAL, who + ": a mask with NFSP_FIT_CE");
  if (!(std::isfinite(j.lr) && j.lr >= 0.f)) return nfsp::fail(NFSP_EINVAL, who + ": lr must be finite and >= 0");
  if (!(j.momentum >= 0.f && j.momentum < 1.f)) return nfsp::fail(NFSP_EINVAL, who + ": momentum must be in [0, 1)");
  return NFSP_OK;
}

struct DevBuf {
  char* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

}  // namespace

extern "C" int nfsp_fit_jobs_check(const nfsp_fit_job* jobs, int n, int64_t steps) {
  NFSP_REQUIRE(n >= 0, "nfsp_fit: n must be >= 0");
  NFSP_REQUIRE(steps >= 0, "nfsp_fit: steps must be >= 0");
  NFSP_REQUIRE(jobs || n == 0, "nfsp_fit: null jobs");
  for (int k = 0; k < n; ++k) {
    const int rc = check_job(jobs[k], k);
    if (rc != NFSP_OK) return rc;
  }
  return NFSP_OK;
}

extern "C" int nfsp_fit_tables(nfsp_ctx* ctx, int game, const nfsp_fit_job* jobs, int n, int64_t steps,
                               double* host_loss) {
  NFSP_REQUIRE(ctx, "null argument");
  int rc = nfsp_fit_jobs_check(jobs, n, steps);
  if (rc != NFSP_OK) return rc;
  NFSP_REQUIRE(game == ctx->game, "nfsp_fit_tables: game is not the ctx's");
  static_assert(H == 64, "nfsp_fit_tables: hidden is 64");
  const nfsp::ex::HostTables* HT = nullptr;
  rc = nfsp::ex::host_tables(game, &HT);
  if (rc != NFSP_OK) return rc;
  const int ndec = (int)HT->legal.size();
  std::vector<int32_t> rows(2 * FIT_SEAT_ROWS, 0);
  int nrows[2] = {0, 0};
  for (int d = 0; d < ndec; ++d) {
    const int s = HT->legal[d] >> 1;
    NFSP_REQUIRE(s <= 1 && nrows[s] < FIT_SEAT_ROWS, "nfsp_fit_tables: the seat has more rows than the kernel holds");
    rows[s * FIT_SEAT_ROWS + nrows[s]++] = d;
  }
  const int nm = (std::max(nrows[0], nrows[1]) * 3 + 3) & ~3;
  const size_t lds = sizeof(float) * fit_lds_floats(nm);
  NFSP_REQUIRE(lds <= (size_t)nfsp::ex::EX_MAX_LDS, "nfsp_fit_tables: the rows do not fit in LDS");
  hipStream_t st = ctx->stream;
  if (n == 0) {
    NFSP_HIP(hipStreamSynchronize(st));
    return NFSP_OK;
  }

  // no two jobs may share a net or its momentum state
  {
    std::vector<uintptr_t> ps;
    for (int k = 0; k < n; ++k) {
      ps.push_back((uintptr_t)jobs[k].dev_w);
      if (jobs[k].dev_v) ps.push_back((uintptr_t)jobs[k].dev_v);
    }
    std::sort(ps.begin(), ps.end());
    for (size_t k = 1; k < ps.size(); ++k)
      NFSP_REQUIRE(ps[k] - ps[k - 1] >= sizeof(float) * NP, "nfsp_fit_tables: two jobs' dev_w / dev_v overlap");
  }

  // every job's data to the host once: all of it finite, the seat's weights >= 0 with a positive
  // sum, CE targets >= 0 -- before anything is launched
  struct HostJob {
    std::vector<double> t, wt;
    std::vector<float> w, v;
  };
  std::vector<HostJob> hj(n);
  for (int k = 0; k < n; ++k) {
    const nfsp_fit_job& j = jobs[k];
    hj[k].t.resize((size_t)ndec * 9);
    hj[k].w.resize(NP);
    NFSP_HIP(hipMemcpyAsync(hj[k].t.data(), j.dev_target, sizeof(double) * ndec * 9, hipMemcpyDeviceToHost, st));
    NFSP_HIP(hipMemcpyAsync(hj[k].w.data(), j.dev_w, sizeof(float) * NP, hipMemcpyDeviceToHost, st));
    if (j.dev_weight) {
      hj[k].wt.resize((size_t)ndec * 3);
      NFSP_HIP(hipMemcpyAsync(hj[k].wt.data(), j.dev_weight, sizeof(double) * ndec * 3, hipMemcpyDeviceToHost, st));
    }
    if (j.dev_v) {
      hj[k].v.resize(NP);
      NFSP_HIP(hipMemcpyAsync(hj[k].v.data(), j.dev_v, sizeof(float) * NP, hipMemcpyDeviceToHost, st));
    }
  }
  NFSP_HIP(hipStreamSynchronize(st));
  std::vector<FitDevJob> dj(n);
  for (int k = 0; k < n; ++k) {
    const nfsp_fit_job& j = jobs[k];
    const std::string who = job_name(k);
    for (int e = 0; e < NP; ++e)
      if (!std::isfinite(hj[k].w[e]) || (j.dev_v && !std::isfinite(hj[k].v[e])))
        return nfsp::fail(NFSP_EINVAL, who + ": dev_w or dev_v is not finite at parameter " + std::to_string(e));
    double wsum = 0.0;
    for (int c = 0; c < nrows[j.seat]; ++c) {
      const int d = rows[j.seat * FIT_SEAT_ROWS + c];
      for (int r = 0; r < 3; ++r) {
        const std::string where = who + ": row " + std::to_string(d) + " rank " + std::to_string(r);
        for (int a = 0; a < 3; ++a) {
          const double t = hj[k].t[((size_t)d * 3 + r) * 3 + a];
          if (!std::isfinite(t) || !std::isfinite((float)t))
            return nfsp::fail(NFSP_EINVAL, where + ": the target is not finite");
          if (j.loss == NFSP_FIT_CE && t < 0.0) return nfsp::fail(NFSP_EINVAL, where + ": a CE target is negative");
        }
        const double w = j.dev_weight ? hj[k].wt[(size_t)d * 3 + r] : 1.0;
        if (!std::isfinite(w) || w < 0.0) return nfsp::fail(NFSP_EINVAL, where + ": the weight is not finite or negative");
        wsum += w;
      }
    }
    if (!(wsum > 0.0) || !std::isfinite(wsum)) return nfsp::fail(NFSP_EINVAL, who + ": the weights' sum is not positive");
    dj[k] = FitDevJob{j.dev_w, j.dev_v, j.dev_target, j.dev_weight, j.dev_mask, wsum, j.seat, j.head, j.loss,
                      j.lr, j.momentum, 0};
  }

  const nfsp::ex::ExTables* T = nullptr;
  rc = nfsp::ex::device_tables(ctx, &T);
  if (rc != NFSP_OK) return rc;
  const size_t b_jobs = sizeof(FitDevJob) * n, b_rows = sizeof(int32_t) * rows.size(), b_loss = sizeof(double) * 2 * n;
  DevBuf buf;
  NFSP_HIP(hipMalloc((void**)&buf.p, b_jobs + b_loss + b_rows));
  NFSP_HIP(hipMemcpyAsync(buf.p, dj.data(), b_jobs, hipMemcpyHostToDevice, st));
  NFSP_HIP(hipMemcpyAsync(buf.p + b_jobs + b_loss, rows.data(), b_rows, hipMemcpyHostToDevice, st));
  NFSP_HIP(hipFuncSetAttribute((const void*)k_fit_tables, hipFuncAttributeMaxDynamicSharedMemorySize,
                               nfsp::ex::EX_MAX_LDS));
  for (int k0 = 0; k0 < n; k0 += NFSP_FIT_MAX_JOBS) {
    FitArgs A{};
    A.jobs = (const FitDevJob*)buf.p + k0;
    A.loss = (double*)(buf.p + b_jobs) + 2 * (size_t)k0;
    A.rows = (const int32_t*)(buf.p + b_jobs + b_loss);
    A.obs = T->obs;
    A.legal = T->legal;
    A.steps = steps;
    A.nrows[0] = nrows[0];
    A.nrows[1] = nrows[1];
    k_fit_tables<<<std::min(n - k0, NFSP_FIT_MAX_JOBS), FIT_WG, lds, st>>>(A);
    NFSP_LAUNCHED("k_fit_tables");
  }
  std::vector<double> loss(2 * (size_t)n);
  NFSP_HIP(hipMemcpyAsync(loss.data(), buf.p + b_jobs, b_loss, hipMemcpyDeviceToHost, st));
  NFSP_HIP(hipStreamSynchronize(st));
  if (host_loss) std::copy(loss.begin(), loss.end(), host_loss);
  return NFSP_OK;
}

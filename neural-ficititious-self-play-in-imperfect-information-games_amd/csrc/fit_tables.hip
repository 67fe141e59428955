// Nets fitted to tables (include/nfsp.h nfsp_fit_tables): a deterministic, weighted,
// full-batch gradient descent of packed 30-64-3 nets on the rows of the evaluator's tree
// (exploit_tree.h obs[ndec][3]), the way the evaluators are built: one workgroup per job, every
// step of the run inside one launch, everything in LDS.  The reference has nothing like it: its
// nets only ever see sampled minibatches (agent/agent.py:209-264).
//
// The step itself (the carve, the forward, the rows, the gradients and the update) is fit_step.h's,
// shared with k_mccfr_net_apply (mccfr.hip).  nfsp_fit_tables_h takes the hidden width: 64 is
// k_fit_tables, 16, 32 and 128 are k_fit_tables_w<H>, the same kernel text (fit_tables_kernel.inc)
// with the width's layout.
//
// Barriers: the step loop runs to A.steps and every loop inside a phase to the job's row count,
// both uniform over the workgroup; the two single-thread regions (the loss sums) lie outside the
// step loop.
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "exploit_tree.h"
#include "fit_step.h"

using namespace nfsp::fit;

namespace {

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

__global__ void __launch_bounds__(FIT_WG) k_fit_tables(FitArgs A) {
#include "fit_tables_kernel.inc"
}

// the same text at another width: one instantiation per entry of FIT_WIDTHS but 64
template <int HH>
__global__ void __launch_bounds__(FIT_WG) k_fit_tables_w(FitArgs A) {
  FIT_WIDTH_NAMES(HH);
  {
#include "fit_tables_kernel.inc"
  }
}

using FitKernel = void (*)(FitArgs);
FitKernel fit_kernel(int hidden) {
  switch (hidden) {
    case 16: return k_fit_tables_w<16>;
    case 32: return k_fit_tables_w<32>;
    case 64: return k_fit_tables;
    case 128: return k_fit_tables_w<128>;
  }
  return nullptr;
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

extern "C" int nfsp_net_params(int hidden, int64_t* np) {
  NFSP_REQUIRE(np, "null argument");
  if (!fit_width_ok(hidden))
    return nfsp::fail(NFSP_EINVAL, "hidden is " + std::to_string(hidden) + ": the widths built are " NFSP_FIT_WIDTHS_TEXT);
  *np = (int64_t)fit_np(hidden);
  return NFSP_OK;
}

extern "C" int nfsp_fit_width_check(int game, int hidden, int64_t* lds_bytes) {
  const nfsp::ex::HostTables* HT = nullptr;
  int rc = nfsp::ex::host_tables(game, &HT);
  if (rc != NFSP_OK) return rc;
  NFSP_REQUIRE(hidden >= 1 && hidden <= 65536, "hidden is not a width: the widths built are " NFSP_FIT_WIDTHS_TEXT);
  int nrows[2] = {0, 0};
  for (uint8_t l : HT->legal) {
    NFSP_REQUIRE((l >> 1) <= 1, "nfsp_fit_width_check: a row of a third seat");
    ++nrows[l >> 1];
  }
  const int nm = (std::max(nrows[0], nrows[1]) * 3 + 3) & ~3;
  const size_t lds = sizeof(float) * fit_lds_floats_h(hidden, nm);
  if (lds > (size_t)nfsp::ex::EX_MAX_LDS)
    return nfsp::fail(NFSP_EINVAL, "hidden " + std::to_string(hidden) + ": a job's rows need " + std::to_string(lds) +
                                       " bytes of LDS, more than the " + std::to_string(nfsp::ex::EX_MAX_LDS) +
                                       " a workgroup may take");
  int64_t np = 0;
  rc = nfsp_net_params(hidden, &np);              // a width that would fit, but is not built
  if (rc != NFSP_OK) return rc;
  if (lds_bytes) *lds_bytes = (int64_t)lds;
  return NFSP_OK;
}

namespace {

// nfsp_fit_tables (hidden 64: k_fit_tables itself) and nfsp_fit_tables_h
int fit_tables_run(nfsp_ctx* ctx, int game, int hidden, const nfsp_fit_job* jobs, int n, int64_t steps,
                   double* host_loss) {
  NFSP_REQUIRE(ctx, "null argument");
  int rc = nfsp_fit_jobs_check(jobs, n, steps);
  if (rc != NFSP_OK) return rc;
  NFSP_REQUIRE(game == ctx->game, "nfsp_fit_tables: game is not the ctx's");
  int64_t lds_need = 0;
  rc = nfsp_fit_width_check(game, hidden, &lds_need);
  if (rc != NFSP_OK) return rc;
  const int NP = (int)fit_np(hidden);             // the width's, not nn's, from here on
  const FitKernel kernel = fit_kernel(hidden);
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
  const size_t lds = sizeof(float) * fit_lds_floats_h(hidden, nm);
  NFSP_REQUIRE(lds <= (size_t)nfsp::ex::EX_MAX_LDS && lds == (size_t)lds_need, "nfsp_fit_tables: the rows do not fit in LDS");
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
  NFSP_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
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
    kernel<<<std::min(n - k0, NFSP_FIT_MAX_JOBS), FIT_WG, lds, st>>>(A);
    NFSP_LAUNCHED("k_fit_tables");
  }
  std::vector<double> loss(2 * (size_t)n);
  NFSP_HIP(hipMemcpyAsync(loss.data(), buf.p + b_jobs, b_loss, hipMemcpyDeviceToHost, st));
  NFSP_HIP(hipStreamSynchronize(st));
  if (host_loss) std::copy(loss.begin(), loss.end(), host_loss);
  return NFSP_OK;
}

}  // namespace

extern "C" int nfsp_fit_tables(nfsp_ctx* ctx, int game, const nfsp_fit_job* jobs, int n, int64_t steps,
                               double* host_loss) {
  return fit_tables_run(ctx, game, nfsp::nn::H, jobs, n, steps, host_loss);
}

extern "C" int nfsp_fit_tables_h(nfsp_ctx* ctx, int game, int hidden, const nfsp_fit_job* jobs, int n, int64_t steps,
                                 double* host_loss) {
  return fit_tables_run(ctx, game, hidden, jobs, n, steps, host_loss);
}

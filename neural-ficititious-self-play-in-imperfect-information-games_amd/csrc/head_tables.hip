// The raw head outputs of packed nets at every information set (include/nfsp.h nfsp_head_tables;
// DESIGN.md §9): what a BR net holds as Q values, where k_policy_table only has the one-hot argmax
// it executes.  One workgroup per net: the net staged with stage_net_lds and one observation of
// the evaluator's tree (exploit_tree.h obs[ndec][3]) per lane through fwd_lds, so the bits are
// the rollout's and k_br_targets' (agent/agent.py:126,219,230).  fwd_lds ballots: every lane of a
// wave calls it, the lanes past the last observation with x = 0, and act is a function of
// blockIdx, uniform over the workgroup.
#include <vector>

#include "engine_internal.h"
#include "exploit_tree.h"

using namespace nfsp::eng;

namespace {

constexpr int HT_NETS = 64;    // nets per launch, as k_evaluate's pairs
constexpr int HT_WG = 256;
struct HtArgs {
  const uint32_t* obs;         // [n3]
  const float* w[HT_NETS];
  float* out;                  // [nets][n3][3]
  int32_t n3;                  // ndec x 3
  int8_t act[HT_NETS];
};

__global__ void __launch_bounds__(HT_WG) k_head_tables(HtArgs A) {
  __shared__ __attribute__((aligned(16))) float sw[NET_LDS];
  const int act = A.act[blockIdx.x];
  stage_net_lds(sw, A.w[blockIdx.x], threadIdx.x, HT_WG);
  __syncthreads();
  float* __restrict__ out = A.out + (size_t)blockIdx.x * A.n3 * 3;
  for (int k0 = 0; k0 < A.n3; k0 += HT_WG) {          // the bound is the workgroup's
    const int k = k0 + (int)threadIdx.x;
    float y[3];
    fwd_lds(sw, k < A.n3 ? A.obs[k] : 0u, act, y);
    if (k < A.n3) {
      out[3 * k + 0] = y[0];
      out[3 * k + 1] = y[1];
      out[3 * k + 2] = y[2];
    }
  }
}

// The same read-out for packed nets of any supported width (fit_step.h FIT_WIDTHS): a plain kernel,
// the net in LDS in packed order, one observation per lane.  Per hidden unit the set bits' W1
// entries ascending from +0, plus b1, ReLU; the units ascending into the three sums, plus b2, then
// the activation -- fwd_lds' operations in fwd_lds' order, so at 64 the bits are k_head_tables'.
// No ballot: a lane past the last observation does nothing.
using nfsp::NA;
using nfsp::OBS;
constexpr int HT_MAX_H = 128;
__global__ void __launch_bounds__(HT_WG) k_head_tables_h(HtArgs A, int H) {
#pragma clang fp contract(off)
  __shared__ float sw[(OBS + 1 + NA) * HT_MAX_H + NA];
  const int act = A.act[blockIdx.x];
  const int np = (OBS + 1 + NA) * H + NA;          // <= the array: the host admits H <= HT_MAX_H only
  const float* __restrict__ w = A.w[blockIdx.x];
  for (int q = threadIdx.x; q < np; q += HT_WG) sw[q] = w[q];
  __syncthreads();
  const float* b1 = sw + OBS * H;
  const float* W2 = b1 + H;
  const float* b2 = W2 + NA * H;
  float* __restrict__ out = A.out + (size_t)blockIdx.x * A.n3 * 3;
  for (int k = threadIdx.x; k < A.n3; k += HT_WG) {
    const uint32_t x = A.obs[k] & ((1u << OBS) - 1u);
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    for (int j = 0; j < H; ++j) {
      float a = 0.f;
      for (uint32_t b = x; b; b &= b - 1) a = a + sw[__builtin_ctz(b) * H + j];
      float h = a + b1[j];
      h = h > 0.f ? h : 0.f;
      o0 = o0 + h * W2[3 * j + 0];
      o1 = o1 + h * W2[3 * j + 1];
      o2 = o2 + h * W2[3 * j + 2];
    }
    o0 = o0 + b2[0];
    o1 = o1 + b2[1];
    o2 = o2 + b2[2];
    float y0, y1, y2;
    if (act == NFSP_ACT_RELU) {
      y0 = o0 > 0.f ? o0 : 0.f;
      y1 = o1 > 0.f ? o1 : 0.f;
      y2 = o2 > 0.f ? o2 : 0.f;
    } else if (act == NFSP_ACT_LINEAR) {
      y0 = o0; y1 = o1; y2 = o2;
    } else {
      const float m = fmaxf(fmaxf(o0, o1), o2);
      const float e0 = expf(o0 - m), e1 = expf(o1 - m), e2 = expf(o2 - m);
      const float s = (e0 + e1) + e2;
      y0 = e0 / s; y1 = e1 / s; y2 = e2 / s;
    }
    out[3 * k + 0] = y0;
    out[3 * k + 1] = y1;
    out[3 * k + 2] = y2;
  }
}

// what both entry points check and loop over; hidden 0: k_head_tables
int head_tables_run(nfsp_ctx* ctx, int game, int hidden, const float* const* dev_w, const int* act, int n,
                    float* dev_out) {
  NFSP_REQUIRE(ctx && ((dev_w && act && dev_out) || n == 0), "null argument");
  NFSP_REQUIRE(n >= 0, "n must be >= 0");
  NFSP_REQUIRE(game == ctx->game, "nfsp_head_tables: game is not the ctx's");
  for (int k = 0; k < n; ++k) {
    NFSP_REQUIRE(dev_w[k], "null weight pointer");
    NFSP_REQUIRE(act[k] == NFSP_ACT_RELU || act[k] == NFSP_ACT_SOFTMAX || act[k] == NFSP_ACT_LINEAR, "bad act");
  }
  const nfsp::ex::ExTables* T = nullptr;
  const int rc = nfsp::ex::device_tables(ctx, &T);
  if (rc != NFSP_OK) return rc;
  const int n3 = T->ndec * 3;
  for (int k0 = 0; k0 < n; k0 += HT_NETS) {
    const int m = n - k0 < HT_NETS ? n - k0 : HT_NETS;
    HtArgs A{};
    A.obs = T->obs;
    A.out = dev_out + (size_t)k0 * n3 * 3;
    A.n3 = n3;
    for (int k = 0; k < m; ++k) {
      A.w[k] = dev_w[k0 + k];
      A.act[k] = (int8_t)act[k0 + k];
    }
    if (hidden) {
      k_head_tables_h<<<m, HT_WG, 0, ctx->stream>>>(A, hidden);
      NFSP_LAUNCHED("k_head_tables_h");
    } else {
      k_head_tables<<<m, HT_WG, 0, ctx->stream>>>(A);
      NFSP_LAUNCHED("k_head_tables");
    }
  }
  NFSP_HIP(hipStreamSynchronize(ctx->stream));
  return NFSP_OK;
}

}  // namespace

extern "C" int nfsp_head_tables_h(nfsp_ctx* ctx, int game, int hidden, const float* const* dev_w, const int* act,
                                  int n, float* dev_out) {
  int64_t np = 0;
  const int rc = nfsp_net_params(hidden, &np);
  if (rc != NFSP_OK) return rc;
  static_assert(HT_MAX_H == 128, "the widest width nfsp_net_params admits");
  NFSP_REQUIRE(hidden <= HT_MAX_H, "nfsp_head_tables_h: hidden is wider than the kernel's LDS");
  return head_tables_run(ctx, game, hidden, dev_w, act, n, dev_out);
}

extern "C" int nfsp_head_tables(nfsp_ctx* ctx, int game, const float* const* dev_w, const int* act, int n,
                                float* dev_out) {
  return head_tables_run(ctx, game, 0, dev_w, act, n, dev_out);
}

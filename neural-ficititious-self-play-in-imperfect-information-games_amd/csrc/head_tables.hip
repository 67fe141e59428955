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

}  // namespace

extern "C" int nfsp_head_tables(nfsp_ctx* ctx, int game, const float* const* dev_w, const int* act, int n,
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
    k_head_tables<<<m, HT_WG, 0, ctx->stream>>>(A);
    NFSP_LAUNCHED("k_head_tables");
  }
  NFSP_HIP(hipStreamSynchronize(ctx->stream));
  return NFSP_OK;
}

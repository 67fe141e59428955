// Exact scores of a pair of policies in the reference's Leduc variant (or the Kuhn swap-in,
// NFSP_GAME_KUHN), played the way main.train plays it (main.py:21-67: dealer alternating per
// hand, the dealer acting first in both rounds, the D / L / D scheduler) with the env's rules
// (leduc/newenv.py, nfsp_device.h hand_step).  SURVEY.md §8(f)1: the true curve beside the
// reference's proxy (agent/agent.py:235-238 summed at main.py:73) and the MC evaluator the
// reference left commented out (main.py:82-120: a BR player against the AR player).
//
// One workgroup per pair walks the evaluator's public tree (exploit_tree.h) on the GPU:
//   1. the policies: each seat's policy spec on every decision row, for each of its ranks --
//        * the AR net (LDS) as a mixed strategy (the softmax, NFSP's average strategy; an illegal
//          raise's mass goes to call, the env's remap) or as the env executes it (argmax, first
//          max wins, leduc/newenv.py:135-145): nfsp_exploitability's modes 0 / 1;
//        * the BR net's greedy action, ReLU or linear Q head: what k_rollout executes when the
//          epsilon draw does not fire (rollout.hip; agent/agent.py:124-128), the learned best
//          response of the evaluator the reference left commented out;
//        * a table [ndec][3 ranks][3 actions] of doubles, for whatever is not a net;
//   2. reach, top-down one depth level at a time: for each evaluation (seat 0's best response,
//      seat 1's, seat 0's on-policy value) and (own rank, opponent rank), chance x opponent
//      reach (x own reach on-policy);
//   3. values, bottom-up: the best-responding seat takes the max over its actions per own rank.
// 2 and 3 are tree_walk.h's steps: f64, no FMA contraction, sums in the order of the recursive
// definition.  Values are in the env's reward units (chips); exploitability = BR_0 + BR_1 (the
// sum, as main.py:73 sums the two proxies).  k_policy_table writes the policy phase's result out
// as a table; k_best_response keeps the argmax the best-response evaluations take a max over, as
// a joint one-hot table with the action values beside it.  Oracle: oracle/exploit_oracle.py
// (independent brute force over full histories with the reference-restated Env).
#include <vector>

#include "nn_device.h"
#include "tree_walk.h"

namespace {

using namespace nfsp::ex;

constexpr int EV_PAIRS = 64;   // pairs per launch: 64 x 2 specs x 16 B + the tables < 4 KB of arguments
struct EvArgs {
  ExTables T;
  nfsp_policy pol[EV_PAIRS][2];  // seat 0 / seat 1, per pair
  double* out;                   // [pairs][ncols]
  int ncols;                     // 6, or 4: without seat 0's value per dealer
};
struct PtArgs {
  ExTables T;
  nfsp_policy pol;
  double* out;                   // [ndec][3][3]
};

// dynamic LDS: the two seats' nets (f32; unused by a table), then policies / reach / values (f64)
__host__ __device__ inline size_t ev_off_pol() { return ((size_t)2 * nfsp::nn::NP * 4 + 15) & ~(size_t)15; }
__host__ __device__ inline size_t ev_lds(int nn, int ndec) {
  return ev_off_pol() + 8 * ((size_t)ndec * 9 + (size_t)nn * 27 + (size_t)nn * 9);
}

__device__ inline bool kind_is_net(int kind) { return kind != NFSP_POL_TABLE; }

// The linear Q head: mlp_forward_bits' sums without its output activation.
__device__ inline void forward_linear_bits(const float* w, uint32_t x, float& y0, float& y1, float& y2) {
#pragma clang fp contract(off)
  constexpr int H = nfsp::nn::H;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f;
  for (int j = 0; j < H; ++j) {
    float acc = 0.f;
    uint32_t bits = x;
    while (bits) {
      const int i = __builtin_ctz(bits);
      bits &= bits - 1;
      acc = acc + w[nfsp::nn::OW1 + i * H + j];
    }
    float hj = acc + w[nfsp::nn::OB1 + j];
    hj = hj > 0.f ? hj : 0.f;
    o0 = o0 + hj * w[nfsp::nn::OW2 + j * 3 + 0];
    o1 = o1 + hj * w[nfsp::nn::OW2 + j * 3 + 1];
    o2 = o2 + hj * w[nfsp::nn::OW2 + j * 3 + 2];
  }
  y0 = o0 + w[nfsp::nn::OB2 + 0];
  y1 = o1 + w[nfsp::nn::OB2 + 1];
  y2 = o2 + w[nfsp::nn::OB2 + 2];
}

// Row k = (decision d, rank r) of a policy as the walk executes it: o[0..2].  net: the policy's
// weights in LDS (net kinds); tab: its table in device memory (NFSP_POL_TABLE).
__device__ inline void policy_row(int kind, const float* net, const double* tab, const ExTables& T, int k,
                                  double* o) {
#pragma clang fp contract(off)
  const bool legal_raise = T.legal[k / 3] & 1;
  if (kind == NFSP_POL_TABLE) {
    const double* t = tab + 3 * (size_t)k;
    o[0] = t[0];
    o[1] = legal_raise ? t[1] : t[1] + t[2];
    o[2] = legal_raise ? t[2] : 0.0;
    return;
  }
  float y0, y1, y2;
  if (kind == NFSP_POL_BR_GREEDY_LINEAR)
    forward_linear_bits(net, T.obs[k], y0, y1, y2);
  else
    nfsp::mlp_forward_bits<nfsp::nn::H>(net, T.obs[k], kind == NFSP_POL_BR_GREEDY ? NFSP_ACT_RELU : NFSP_ACT_SOFTMAX,
                                        y0, y1, y2);
  if (kind == NFSP_POL_AR_SOFTMAX) {
    o[0] = y0;
    o[1] = legal_raise ? (double)y1 : (double)y1 + (double)y2;
    o[2] = legal_raise ? (double)y2 : 0.0;
  } else {
    int a = nfsp::argmax3(y0, y1, y2);
    if (a == 2 && !legal_raise) a = 1;
    o[0] = a == 0 ? 1.0 : 0.0;
    o[1] = a == 1 ? 1.0 : 0.0;
    o[2] = a == 2 ? 1.0 : 0.0;
  }
}

struct BrOut {
  double* beta;                  // [ndec][3][3]
  double* q;                     // [ndec][3][3] or null
  double* rch;                   // [ndec][3] or null
};

// The three phases for the first NE evaluations, side by side: e = 0 seat 0 best-responds, 1 seat
// 1 best-responds, 2 seat 0 on-policy; ri is the rank of seat i = (e == 1).  LDS as ev_lds (NE 3)
// / br_lds (NE 2) size it.  With KEEP_ARGMAX a best responder's decision writes its row of O.
// Returns the values [nn][NE][ri].  Every thread calls it, with the same arguments: 2 nlev + 2
// barriers.
template <int NE, bool KEEP_ARGMAX>
__device__ inline const double* walk(char* smem, const ExTables& T, nfsp_policy P0, nfsp_policy P1, const BrOut& O) {
#pragma clang fp contract(off)
  float* sw = reinterpret_cast<float*>(smem);                          // [2][NP]
  double* pol = reinterpret_cast<double*>(smem + ev_off_pol());        // [ndec][3 ranks][3]
  double* reach = pol + (size_t)T.ndec * 9;                            // [nn][NE][ri][ro]
  double* val = reach + (size_t)T.nn * 9 * NE;                         // [nn][NE][ri]
  const int tid = threadIdx.x, nt = blockDim.x;
  const int NP = nfsp::nn::NP;
  for (int k = tid; k < 2 * NP; k += nt) {
    const nfsp_policy& P = k < NP ? P0 : P1;
    if (kind_is_net(P.kind)) sw[k] = static_cast<const float*>(P.dev)[k < NP ? k : k - NP];
  }
  __syncthreads();
  // 1. policies of the acting seat at every decision, for each of its ranks
  for (int k = tid; k < T.ndec * 3; k += nt) {
    const int p = T.legal[k / 3] >> 1;           // the acting seat
    const nfsp_policy& P = p ? P1 : P0;
    policy_row(P.kind, sw + p * NP, static_cast<const double*>(P.dev), T, k, pol + 3 * (size_t)k);
  }
  __syncthreads();
  // 2. reach, top-down
  for (int L = 0; L < T.nlev; ++L) {
    const int n0 = T.lev[L], cnt = (T.lev[L + 1] - n0) * 9 * NE;
    for (int k = tid; k < cnt; k += nt) {
      const int n = n0 + k / (9 * NE), e = (k / 9) % NE, ri = (k / 3) % 3, ro = k % 3;
      double* item = reach + e * 9 + ri * 3 + ro;
      item[(size_t)n * 9 * NE] = reach_step(T, T.nodes, T.nodes[n], e == 1, ri, ro, pol, item, 9 * NE, e == 2);
    }
    __syncthreads();
  }
  // 3. values, bottom-up
  for (int L = T.nlev - 1; L >= 0; --L) {
    const int n0 = T.lev[L], cnt = (T.lev[L + 1] - n0) * 3 * NE;
    for (int k = tid; k < cnt; k += nt) {
      const int n = n0 + k / (3 * NE), e = (k / 3) % NE, ri = k % 3;
      const int i = e == 1;
      const DevNode& N = T.nodes[n];
      const double* rr = reach + (size_t)n * 9 * NE + e * 9 + ri * 3;
      double* item = val + e * 3 + ri;
      double v;
      if (N.kind == TNode::TERMINAL) {
        v = terminal_value(T, N, i, ri, rr);
      } else if (N.kind == TNode::DECISION && N.p == i && e < 2) {
        int best;
        v = first_max_child(N, item, 3 * NE, best);
        if (KEEP_ARGMAX) {
          const size_t row = (size_t)N.row * 3 + ri;
          for (int a = 0; a < 3; ++a) {
            O.beta[3 * row + a] = a == best ? 1.0 : 0.0;
            if (O.q) O.q[3 * row + a] = N.child[a] >= 0 ? item[(size_t)N.child[a] * 3 * NE] : 0.0;
          }
          if (O.rch) O.rch[row] = sum3(rr);
        }
      } else {
        v = sum_children(N, item, 3 * NE);
      }
      item[(size_t)n * 3 * NE] = v;
    }
    __syncthreads();
  }
  return val;
}

__global__ void __launch_bounds__(256) k_evaluate(EvArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const ExTables& T = A.T;
  const double* val = walk<3, false>(smem_raw, T, A.pol[blockIdx.x][0], A.pol[blockIdx.x][1], BrOut{});
  if (threadIdx.x == 0) {
    double* o = A.out + (size_t)A.ncols * blockIdx.x;
    const double br0 = root_value(T, val, 9), br1 = root_value(T, val + 3, 9);
    o[0] = br0;
    o[1] = br1;
    o[2] = br0 + br1;
    o[3] = root_value(T, val + 6, 9);
    if (A.ncols == 6) {                            // seat 0's on-policy value given the dealer
      o[4] = sum3(val + (size_t)T.root[0] * 9 + 6);
      o[5] = sum3(val + (size_t)T.root[1] * 9 + 6);
    }
  }
}

// The policy phase alone, for every decision row whichever seat acts there.
__global__ void __launch_bounds__(256) k_policy_table(PtArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* sw = reinterpret_cast<float*>(smem_raw);                      // [NP]
  const int tid = threadIdx.x, nt = blockDim.x;
  if (kind_is_net(A.pol.kind))
    for (int k = tid; k < nfsp::nn::NP; k += nt) sw[k] = static_cast<const float*>(A.pol.dev)[k];
  __syncthreads();
  for (int k = tid; k < A.T.ndec * 3; k += nt) {
    double o[3];
    policy_row(A.pol.kind, sw, static_cast<const double*>(A.pol.dev), A.T, k, o);
    A.out[3 * (size_t)k + 0] = o[0];
    A.out[3 * (size_t)k + 1] = o[1];
    A.out[3 * (size_t)k + 2] = o[2];
  }
}

// The exact best responses as a strategy: k_evaluate's walk for evaluations e = 0 and 1, with the
// argmax its max discards.  Seat e's rows of the joint table hold its best response against the
// other seat's policy; q is the child values the max runs over, rch the counterfactual reach of
// the information set summed over the opponent's rank.  The first maximum among the legal
// children wins, so a tie and every information set the opponent never reaches fold.  One
// workgroup.
struct BrArgs {
  ExTables T;
  nfsp_policy pol[2];
  BrOut out;
};
__host__ __device__ inline size_t br_lds(int nn, int ndec) {
  return ev_off_pol() + 8 * ((size_t)ndec * 9 + (size_t)nn * 18 + (size_t)nn * 6);
}

__global__ void __launch_bounds__(256) k_best_response(BrArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  walk<2, true>(smem_raw, A.T, A.pol[0], A.pol[1], A.out);
}

int check_policy(const nfsp_policy& p) {
  NFSP_REQUIRE(p.kind >= NFSP_POL_AR_SOFTMAX && p.kind <= NFSP_POL_TABLE, "unknown policy kind (NFSP_POL_*)");
  NFSP_REQUIRE(p.reserved == 0, "nfsp_policy.reserved must be 0");
  NFSP_REQUIRE(p.dev, "null policy pointer");
  return NFSP_OK;
}

// The launch path of both batch entry points: n checked pairs through k_evaluate, EV_PAIRS per
// launch, the first ncols of each pair's six results to host_out[n][ncols].
int evaluate_pairs(nfsp_ctx* ctx, const nfsp_policy* seat0, const nfsp_policy* seat1, int n, double* host_out,
                   int ncols) {
  if (n == 0) return NFSP_OK;
  const ExTables* T = nullptr;
  const int rc = device_tables(ctx, &T);
  if (rc != NFSP_OK) return rc;
  const size_t lds = ev_lds(T->nn, T->ndec);
  NFSP_REQUIRE(lds <= EX_MAX_LDS, "evaluation tables exceed the LDS");
  NFSP_HIP(hipFuncSetAttribute((const void*)k_evaluate, hipFuncAttributeMaxDynamicSharedMemorySize, EX_MAX_LDS));
  struct DevBuf {                               // freed on every exit path
    void* p = nullptr;
    hipStream_t s;
    explicit DevBuf(hipStream_t s_) : s(s_) {}
    ~DevBuf() { if (p) (void)hipFreeAsync(p, s); }
  } bo(ctx->stream);
  NFSP_HIP(hipMallocAsync(&bo.p, sizeof(double) * ncols * n, ctx->stream));
  for (int k0 = 0; k0 < n; k0 += EV_PAIRS) {
    const int m = n - k0 < EV_PAIRS ? n - k0 : EV_PAIRS;
    EvArgs A{};
    A.T = *T;
    for (int k = 0; k < m; ++k) {
      A.pol[k][0] = seat0[k0 + k];
      A.pol[k][1] = seat1[k0 + k];
    }
    A.out = static_cast<double*>(bo.p) + ncols * (size_t)k0;
    A.ncols = ncols;
    k_evaluate<<<m, 256, lds, ctx->stream>>>(A);
    NFSP_LAUNCHED("k_evaluate");
  }
  NFSP_HIP(hipMemcpyAsync(host_out, bo.p, sizeof(double) * ncols * n, hipMemcpyDeviceToHost, ctx->stream));
  NFSP_HIP(hipStreamSynchronize(ctx->stream));
  return NFSP_OK;
}

}  // namespace

extern "C" int nfsp_evaluate_batch(nfsp_ctx* ctx, const nfsp_policy* seat0, const nfsp_policy* seat1, int n,
                                   double* out) {
  NFSP_REQUIRE(ctx && seat0 && seat1 && out, "null argument");
  NFSP_REQUIRE(n >= 0, "n must be >= 0");
  for (int k = 0; k < n; ++k) {
    int rc = check_policy(seat0[k]);
    if (rc == NFSP_OK) rc = check_policy(seat1[k]);
    if (rc != NFSP_OK) return rc;
  }
  return evaluate_pairs(ctx, seat0, seat1, n, out, 6);
}

// Two AR nets per pair, both read the way `mode` says: the first four of nfsp_evaluate_batch's six.
extern "C" int nfsp_exploitability_batch(nfsp_ctx* ctx, const float* const* dev_w_ar0,
                                         const float* const* dev_w_ar1, int n, int mode, double* out) {
  NFSP_REQUIRE(ctx && dev_w_ar0 && dev_w_ar1 && out, "null argument");
  NFSP_REQUIRE(n >= 0, "n must be >= 0");
  NFSP_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (softmax mixed) or 1 (argmax as executed)");
  for (int k = 0; k < n; ++k) NFSP_REQUIRE(dev_w_ar0[k] && dev_w_ar1[k], "null weight pointer");
  const int kind = mode ? NFSP_POL_AR_ARGMAX : NFSP_POL_AR_SOFTMAX;
  std::vector<nfsp_policy> seat0(n), seat1(n);
  for (int k = 0; k < n; ++k) {
    seat0[k] = nfsp_policy{kind, 0, dev_w_ar0[k]};
    seat1[k] = nfsp_policy{kind, 0, dev_w_ar1[k]};
  }
  return evaluate_pairs(ctx, seat0.data(), seat1.data(), n, out, 4);
}

extern "C" int nfsp_exploitability(nfsp_ctx* ctx, const float* dev_w_ar0, const float* dev_w_ar1, int mode,
                                   double* out) {
  NFSP_REQUIRE(ctx && dev_w_ar0 && dev_w_ar1 && out, "null argument");
  return nfsp_exploitability_batch(ctx, &dev_w_ar0, &dev_w_ar1, 1, mode, out);
}

extern "C" int nfsp_best_response_table(nfsp_ctx* ctx, const nfsp_policy* seat0, const nfsp_policy* seat1,
                                        double* dev_beta, double* dev_q, double* dev_reach) {
  NFSP_REQUIRE(ctx && seat0 && seat1 && dev_beta, "null argument");
  int rc = check_policy(*seat0);
  if (rc == NFSP_OK) rc = check_policy(*seat1);
  if (rc != NFSP_OK) return rc;
  const ExTables* T = nullptr;
  rc = device_tables(ctx, &T);
  if (rc != NFSP_OK) return rc;
  const size_t n9 = sizeof(double) * 9 * (size_t)T->ndec;
  const char* outs[3] = {reinterpret_cast<const char*>(dev_beta), reinterpret_cast<const char*>(dev_q),
                         reinterpret_cast<const char*>(dev_reach)};
  const size_t outb[3] = {n9, n9, n9 / 3};
  for (const nfsp_policy* p : {seat0, seat1}) {      // the kernel reads the policies while it writes
    const char* lo = static_cast<const char*>(p->dev);
    const char* hi = lo + (p->kind == NFSP_POL_TABLE ? n9 : sizeof(float) * nfsp::nn::NP);
    for (int k = 0; k < 3; ++k)
      NFSP_REQUIRE(!outs[k] || outs[k] + outb[k] <= lo || hi <= outs[k],
                   "nfsp_best_response_table: an output aliases a policy");
  }
  for (int k = 0; k < 3; ++k)
    for (int j = k + 1; j < 3; ++j)
      NFSP_REQUIRE(!outs[k] || !outs[j] || outs[k] + outb[k] <= outs[j] || outs[j] + outb[j] <= outs[k],
                   "nfsp_best_response_table: two outputs alias each other");
  const size_t lds = br_lds(T->nn, T->ndec);
  NFSP_REQUIRE(lds <= EX_MAX_LDS, "best-response tables exceed the LDS");
  NFSP_HIP(hipFuncSetAttribute((const void*)k_best_response, hipFuncAttributeMaxDynamicSharedMemorySize, EX_MAX_LDS));
  BrArgs A{};
  A.T = *T;
  A.pol[0] = *seat0;
  A.pol[1] = *seat1;
  A.out = BrOut{dev_beta, dev_q, dev_reach};
  k_best_response<<<1, 256, lds, ctx->stream>>>(A);
  NFSP_LAUNCHED("k_best_response");
  NFSP_HIP(hipStreamSynchronize(ctx->stream));
  return NFSP_OK;
}

extern "C" int nfsp_policy_table(nfsp_ctx* ctx, const nfsp_policy* policy, double* dev_out) {
  NFSP_REQUIRE(ctx && policy && dev_out, "null argument");
  int rc = check_policy(*policy);
  if (rc != NFSP_OK) return rc;
  NFSP_REQUIRE(policy->dev != dev_out, "nfsp_policy_table in place");
  const ExTables* T = nullptr;
  rc = device_tables(ctx, &T);
  if (rc != NFSP_OK) return rc;
  PtArgs A{};
  A.T = *T;
  A.pol = *policy;
  A.out = dev_out;
  k_policy_table<<<1, 256, sizeof(float) * nfsp::nn::NP, ctx->stream>>>(A);
  NFSP_LAUNCHED("k_policy_table");
  NFSP_HIP(hipStreamSynchronize(ctx->stream));
  return NFSP_OK;
}

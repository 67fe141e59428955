// Exact scores of any pair of policies on the evaluator's public tree (exploit_tree.h): the
// walk of exploit.hip (k_exploit_walk: policies, reach top-down, values bottom-up; f64, no
// FMA contraction, sums in the order of the recursive definition) with the policy phase
// generalised from "the seat's AR net" to a policy spec per seat:
//   * the AR net as a softmax or as the executed argmax (k_exploit_walk's modes 0 / 1);
//   * the BR net's greedy action, ReLU or linear Q head: what k_rollout executes when the
//     epsilon draw does not fire (rollout.hip; agent/agent.py:124-128), the learned best
//     response of the evaluator the reference left commented out (main.py:82-120);
//   * a table [ndec][3 ranks][3 actions] of doubles, for whatever is not a net.
// and two more outputs, seat 0's value per dealer.  k_policy_table writes the policy phase's
// result out as such a table; k_best_response keeps the argmax the best-response evaluations
// take a max over, as a joint one-hot table with the action values beside it.  Oracle:
// oracle/exploit_oracle.py with a TabularPolicy.
#include "exploit_tree.h"
#include "nn_device.h"

namespace {

using namespace nfsp::ex;

constexpr int EV_PAIRS = 64;   // pairs per launch: 64 x 2 specs x 16 B + the tables < 4 KB of arguments
struct EvArgs {
  ExTables T;
  nfsp_policy pol[EV_PAIRS][2];  // seat 0 / seat 1, per pair
  double* out;                   // [pairs][6]
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

__global__ void __launch_bounds__(256) k_evaluate(EvArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const ExTables& T = A.T;
  float* sw = reinterpret_cast<float*>(smem_raw);                      // [2][NP]
  double* pol = reinterpret_cast<double*>(smem_raw + ev_off_pol());    // [ndec][3 ranks][3]
  double* reach = pol + (size_t)T.ndec * 9;                            // [nn][3 evals][3][3]
  double* val = reach + (size_t)T.nn * 27;                             // [nn][3 evals][3]
  const int tid = threadIdx.x, nt = blockDim.x;
  const int NP = nfsp::nn::NP;
  const nfsp_policy P0 = A.pol[blockIdx.x][0], P1 = A.pol[blockIdx.x][1];
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
  // 2. reach, top-down.  Evaluation e: 0 = seat 0 best-responds, 1 = seat 1 best-responds,
  //    2 = seat 0 on-policy.  Index [node][e][ri][ro], ri = seat i's rank (i = e == 1).
  for (int L = 0; L < T.nlev; ++L) {
    const int n0 = T.lev[L], cnt = (T.lev[L + 1] - n0) * 27;
    for (int k = tid; k < cnt; k += nt) {
      const int n = n0 + k / 27, e = (k / 9) % 3, ri = (k / 3) % 3, ro = k % 3;
      const DevNode& N = T.nodes[n];
      double r;
      if (N.parent < 0) {
        r = T.deal[ri][ro];
      } else {
        const DevNode& P = T.nodes[N.parent];
        const double r0 = reach[(size_t)N.parent * 27 + e * 9 + ri * 3 + ro];
        const int i = e == 1 ? 1 : 0;
        if (P.kind == TNode::CHANCE) r = r0 * p_public(N.via, ri, ro);
        else if (P.p == i) r = e < 2 ? r0 : r0 * pol[(size_t)P.row * 9 + ri * 3 + N.via];
        else r = r0 * pol[(size_t)P.row * 9 + ro * 3 + N.via];
      }
      reach[(size_t)n * 27 + e * 9 + ri * 3 + ro] = r;
    }
    __syncthreads();
  }
  // 3. values, bottom-up: [node][e][ri]
  for (int L = T.nlev - 1; L >= 0; --L) {
    const int n0 = T.lev[L], cnt = (T.lev[L + 1] - n0) * 9;
    for (int k = tid; k < cnt; k += nt) {
      const int n = n0 + k / 9, e = (k / 3) % 3, ri = k % 3;
      const int i = e == 1 ? 1 : 0;
      const DevNode& N = T.nodes[n];
      double v = 0.0;
      if (N.kind == TNode::TERMINAL) {
        const double* rr = reach + (size_t)n * 27 + e * 9 + ri * 3;
        const float* py = T.pay + (size_t)N.row * 18 + i * 9 + ri * 3;
        for (int ro = 0; ro < 3; ++ro)
          if (rr[ro] != 0.0) v += rr[ro] * (double)py[ro];
      } else if (N.kind == TNode::DECISION && N.p == i && e < 2) {
        v = -1e300;
        for (int a = 0; a < 3; ++a) {
          if (N.child[a] < 0) continue;
          const double c = val[(size_t)N.child[a] * 9 + e * 3 + ri];
          v = c > v ? c : v;
        }
      } else {
        for (int a = 0; a < 3; ++a)
          if (N.child[a] >= 0) v += val[(size_t)N.child[a] * 9 + e * 3 + ri];
      }
      val[(size_t)n * 9 + e * 3 + ri] = v;
    }
    __syncthreads();
  }
  if (tid == 0) {
    double br[2] = {0.0, 0.0}, onp = 0.0, per[2] = {0.0, 0.0};
    for (int e = 0; e < 3; ++e)
      for (int d = 0; d < 2; ++d) {
        const double* v = val + (size_t)T.root[d] * 9 + e * 3;
        const double s1 = (v[0] + v[1]) + v[2];    // the value given the dealer
        const double s = 0.5 * s1;
        if (e < 2) br[e] += s; else { onp += s; per[d] = s1; }
      }
    double* o = A.out + 6 * (size_t)blockIdx.x;
    o[0] = br[0];
    o[1] = br[1];
    o[2] = br[0] + br[1];
    o[3] = onp;
    o[4] = per[0];
    o[5] = per[1];
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

// The exact best responses as a strategy: k_evaluate's phases for evaluations e = 0 and 1 (the
// same sums in the same order), with the argmax its max discards.  Seat e's rows of the joint
// table hold its best response against the other seat's policy; q is the child values the max
// runs over, rch the counterfactual reach of the information set summed over the opponent's
// rank.  The first maximum among the legal children wins, so a tie and every information set
// the opponent never reaches fold.  One workgroup; 2 nlev + 2 barriers.
struct BrArgs {
  ExTables T;
  nfsp_policy pol[2];
  double* beta;                  // [ndec][3][3]
  double* q;                     // [ndec][3][3] or null
  double* rch;                   // [ndec][3] or null
};
__host__ __device__ inline size_t br_lds(int nn, int ndec) {
  return ev_off_pol() + 8 * ((size_t)ndec * 9 + (size_t)nn * 18 + (size_t)nn * 6);
}

__global__ void __launch_bounds__(256) k_best_response(BrArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const ExTables& T = A.T;
  float* sw = reinterpret_cast<float*>(smem_raw);                      // [2][NP]
  double* pol = reinterpret_cast<double*>(smem_raw + ev_off_pol());    // [ndec][3 ranks][3]
  double* reach = pol + (size_t)T.ndec * 9;                            // [nn][2 evals][3][3]
  double* val = reach + (size_t)T.nn * 18;                             // [nn][2 evals][3]
  const int tid = threadIdx.x, nt = blockDim.x;
  const int NP = nfsp::nn::NP;
  const nfsp_policy P0 = A.pol[0], P1 = A.pol[1];
  for (int k = tid; k < 2 * NP; k += nt) {
    const nfsp_policy& P = k < NP ? P0 : P1;
    if (kind_is_net(P.kind)) sw[k] = static_cast<const float*>(P.dev)[k < NP ? k : k - NP];
  }
  __syncthreads();
  for (int k = tid; k < T.ndec * 3; k += nt) {
    const int p = T.legal[k / 3] >> 1;
    const nfsp_policy& P = p ? P1 : P0;
    policy_row(P.kind, sw + p * NP, static_cast<const double*>(P.dev), T, k, pol + 3 * (size_t)k);
  }
  __syncthreads();
  // reach of seat e's ranks ri against the opponent's ro, without seat e's own actions
  for (int L = 0; L < T.nlev; ++L) {
    const int n0 = T.lev[L], cnt = (T.lev[L + 1] - n0) * 18;
    for (int k = tid; k < cnt; k += nt) {
      const int n = n0 + k / 18, e = (k / 9) % 2, ri = (k / 3) % 3, ro = k % 3;
      const DevNode& N = T.nodes[n];
      double r;
      if (N.parent < 0) {
        r = T.deal[ri][ro];
      } else {
        const DevNode& P = T.nodes[N.parent];
        const double r0 = reach[(size_t)N.parent * 18 + e * 9 + ri * 3 + ro];
        if (P.kind == TNode::CHANCE) r = r0 * p_public(N.via, ri, ro);
        else if (P.p == e) r = r0;
        else r = r0 * pol[(size_t)P.row * 9 + ro * 3 + N.via];
      }
      reach[(size_t)n * 18 + e * 9 + ri * 3 + ro] = r;
    }
    __syncthreads();
  }
  // values bottom-up; a decision of seat e writes its row of the outputs
  for (int L = T.nlev - 1; L >= 0; --L) {
    const int n0 = T.lev[L], cnt = (T.lev[L + 1] - n0) * 6;
    for (int k = tid; k < cnt; k += nt) {
      const int n = n0 + k / 6, e = (k / 3) % 2, ri = k % 3;
      const DevNode& N = T.nodes[n];
      double v = 0.0;
      if (N.kind == TNode::TERMINAL) {
        const double* rr = reach + (size_t)n * 18 + e * 9 + ri * 3;
        const float* py = T.pay + (size_t)N.row * 18 + e * 9 + ri * 3;
        for (int ro = 0; ro < 3; ++ro)
          if (rr[ro] != 0.0) v += rr[ro] * (double)py[ro];
      } else if (N.kind == TNode::DECISION && N.p == e) {
        int best = -1;
        double c3[3] = {0.0, 0.0, 0.0};
        for (int a = 0; a < 3; ++a) {
          if (N.child[a] < 0) continue;
          const double c = val[(size_t)N.child[a] * 6 + e * 3 + ri];
          c3[a] = c;
          if (best < 0 || c > v) {
            v = c;
            best = a;
          }
        }
        const size_t row = (size_t)N.row * 3 + ri;
        for (int a = 0; a < 3; ++a) {
          A.beta[3 * row + a] = a == best ? 1.0 : 0.0;
          if (A.q) A.q[3 * row + a] = c3[a];
        }
        if (A.rch) {
          const double* rr = reach + (size_t)n * 18 + e * 9 + ri * 3;
          A.rch[row] = (rr[0] + rr[1]) + rr[2];
        }
      } else {
        for (int a = 0; a < 3; ++a)
          if (N.child[a] >= 0) v += val[(size_t)N.child[a] * 6 + e * 3 + ri];
      }
      val[(size_t)n * 6 + e * 3 + ri] = v;
    }
    __syncthreads();
  }
}

int check_policy(const nfsp_policy& p) {
  NFSP_REQUIRE(p.kind >= NFSP_POL_AR_SOFTMAX && p.kind <= NFSP_POL_TABLE, "unknown policy kind (NFSP_POL_*)");
  NFSP_REQUIRE(p.reserved == 0, "nfsp_policy.reserved must be 0");
  NFSP_REQUIRE(p.dev, "null policy pointer");
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
  if (n == 0) return NFSP_OK;
  const DevTables* D = nullptr;
  const int rc = device_tables(ctx, &D);
  if (rc != NFSP_OK) return rc;
  const size_t lds = ev_lds(D->T.nn, D->T.ndec);
  NFSP_REQUIRE(lds <= EX_MAX_LDS, "evaluation tables exceed the LDS");
  NFSP_HIP(hipFuncSetAttribute((const void*)k_evaluate, hipFuncAttributeMaxDynamicSharedMemorySize, EX_MAX_LDS));
  struct DevBuf {                               // freed on every exit path
    void* p = nullptr;
    hipStream_t s;
    explicit DevBuf(hipStream_t s_) : s(s_) {}
    ~DevBuf() { if (p) (void)hipFreeAsync(p, s); }
  } bo(ctx->stream);
  NFSP_HIP(hipMallocAsync(&bo.p, sizeof(double) * 6 * n, ctx->stream));
  for (int k0 = 0; k0 < n; k0 += EV_PAIRS) {
    const int m = n - k0 < EV_PAIRS ? n - k0 : EV_PAIRS;
    EvArgs A{};
    A.T = D->T;
    for (int k = 0; k < m; ++k) {
      A.pol[k][0] = seat0[k0 + k];
      A.pol[k][1] = seat1[k0 + k];
    }
    A.out = static_cast<double*>(bo.p) + 6 * (size_t)k0;
    k_evaluate<<<m, 256, lds, ctx->stream>>>(A);
    NFSP_LAUNCHED("k_evaluate");
  }
  NFSP_HIP(hipMemcpyAsync(out, bo.p, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, ctx->stream));
  NFSP_HIP(hipStreamSynchronize(ctx->stream));
  return NFSP_OK;
}

extern "C" int nfsp_best_response_table(nfsp_ctx* ctx, const nfsp_policy* seat0, const nfsp_policy* seat1,
                                        double* dev_beta, double* dev_q, double* dev_reach) {
  NFSP_REQUIRE(ctx && seat0 && seat1 && dev_beta, "null argument");
  int rc = check_policy(*seat0);
  if (rc == NFSP_OK) rc = check_policy(*seat1);
  if (rc != NFSP_OK) return rc;
  const DevTables* D = nullptr;
  rc = device_tables(ctx, &D);
  if (rc != NFSP_OK) return rc;
  const size_t n9 = sizeof(double) * 9 * (size_t)D->T.ndec;
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
  const size_t lds = br_lds(D->T.nn, D->T.ndec);
  NFSP_REQUIRE(lds <= EX_MAX_LDS, "best-response tables exceed the LDS");
  NFSP_HIP(hipFuncSetAttribute((const void*)k_best_response, hipFuncAttributeMaxDynamicSharedMemorySize, EX_MAX_LDS));
  BrArgs A{};
  A.T = D->T;
  A.pol[0] = *seat0;
  A.pol[1] = *seat1;
  A.beta = dev_beta;
  A.q = dev_q;
  A.rch = dev_reach;
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
  const DevTables* D = nullptr;
  rc = device_tables(ctx, &D);
  if (rc != NFSP_OK) return rc;
  PtArgs A{};
  A.T = D->T;
  A.pol = *policy;
  A.out = dev_out;
  k_policy_table<<<1, 256, sizeof(float) * nfsp::nn::NP, ctx->stream>>>(A);
  NFSP_LAUNCHED("k_policy_table");
  NFSP_HIP(hipStreamSynchronize(ctx->stream));
  return NFSP_OK;
}

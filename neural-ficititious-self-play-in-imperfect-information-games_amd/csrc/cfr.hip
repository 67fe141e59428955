// CFR+ (Tammelin 2014: regret-matching+, alternating updates, linearly weighted average) on the
// evaluator's public tree (exploit_tree.h), so that its equilibrium is one of exactly the game
// nfsp_evaluate_batch scores: the absolute anchor of this Leduc variant (the reference has no
// solver; Kuhn's anchor is analytic).
//
// One workgroup of 256.  During a launch the regrets R, the strategy sums S, the current
// strategy sigma [ndec][3 ranks][3], the updating seat's counterfactual reach [nn][3][3], its own
// reach and the values [nn][3] live in LDS as f64 (Leduc: about 72 KB, + the node table); R and
// S live in device memory between launches.  Iteration t = 1, 2, ..; for seat i = 0, then 1:
//   1. sigma = R+ / sum R+ over the legal actions (1 / nlegal where the sum is 0), every row;
//   2. top-down, a level at a time: from a chance parent cf x p_public, from the opponent's
//      decision cf x sigma[opponent's rank], from seat i's decision own x sigma[own rank];
//   3. bottom-up: a terminal sums cf x pay over the opponent's rank, seat i's decision
//      sum_a sigma_a v(child_a), every other node sums its children;
//   4. at seat i's decisions R = max(0, R + v(child_a) - v), S += t x own x sigma.
// (4 recomputes sigma of the rows it changed, which is step 1 of the next half-iteration.)
// 3 and the rows of 1 are tree_walk.h's steps and 2 is its reach_step with the own reach beside
// it, so the sums are the evaluator's (actions, public ranks, opponent ranks ascending; no FMA
// contraction): tests/policy_ref.py restates it in numpy to the bit.
//
// The work per level is a few hundred items, so the workgroup is barrier-latency bound (2 nlev
// + 1 barriers per half-iteration, 34 per Leduc iteration); it runs on the device because
// that is where the tables and the evaluator are and the library has no host compute path,
// not for throughput.
#include "tree_walk.h"

struct nfsp_cfr {
  nfsp_ctx* ctx = nullptr;
  int ndec = 0;
  int64_t iterations = 0;
  double* dev = nullptr;       // R | S | average, [ndec][3][3] each
};

namespace {

using namespace nfsp::ex;

struct CfrArgs {
  ExTables T;
  double* R;                   // [ndec][3][3], in and out
  double* S;
  double* avg;                 // out: S normalised per row
  long long t0;                // iterations done before this launch
  int iters;
};

// dynamic LDS (f64 first, then the node table)
__host__ __device__ inline size_t cfr_lds(int nn, int ndec) {
  return 8 * ((size_t)ndec * 27 + (size_t)nn * 9 + (size_t)nn * 6) + sizeof(DevNode) * (size_t)nn;
}

// regret matching on one row; an illegal raise has R = 0 always
__device__ inline void match_row(const double* R, bool legal_raise, double* sg) {
#pragma clang fp contract(off)
  const double r[3] = {R[0] > 0.0 ? R[0] : 0.0, R[1] > 0.0 ? R[1] : 0.0, legal_raise && R[2] > 0.0 ? R[2] : 0.0};
  average_row(r, legal_raise, sg);
}

__global__ void __launch_bounds__(256) k_cfr_plus(CfrArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const ExTables& T = A.T;
  const int nn = T.nn, ndec = T.ndec, nlev = T.nlev;
  double* R = reinterpret_cast<double*>(smem_raw);     // [ndec][3][3]
  double* S = R + (size_t)ndec * 9;
  double* sg = S + (size_t)ndec * 9;
  double* cf = sg + (size_t)ndec * 9;                  // [nn][ri][ro]
  double* own = cf + (size_t)nn * 9;                   // [nn][ri]
  double* val = own + (size_t)nn * 3;                  // [nn][ri]
  DevNode* nodes = reinterpret_cast<DevNode*>(val + (size_t)nn * 3);
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int k = tid; k < ndec * 9; k += nt) {
    R[k] = A.R[k];
    S[k] = A.S[k];
  }
  for (int k = tid; k < nn; k += nt) nodes[k] = T.nodes[k];
  __syncthreads();
  for (int k = tid; k < ndec * 3; k += nt) match_row(R + 3 * k, T.legal[k / 3] & 1, sg + 3 * k);
  __syncthreads();
  for (int it = 0; it < A.iters; ++it) {
    const double t = (double)(A.t0 + 1 + it);
    for (int i = 0; i < 2; ++i) {
      // 2. reach of seat i's ranks ri against the opponent's ro, top-down
      for (int L = 0; L < nlev; ++L) {
        const int n0 = T.lev[L], cnt = (T.lev[L + 1] - n0) * 9;
        for (int k = tid; k < cnt; k += nt) {
          const int n = n0 + k / 9, ri = (k / 3) % 3, ro = k % 3;
          // tree_walk.h's reach_step and seat i's own reach in one chain of branches (see there)
          const DevNode& N = nodes[n];
          double c, o;
          if (N.parent < 0) {
            c = T.deal[ri][ro];
            o = 1.0;
          } else {
            const DevNode& P = nodes[N.parent];
            c = cf[(size_t)N.parent * 9 + ri * 3 + ro];
            o = own[(size_t)N.parent * 3 + ri];
            if (P.kind == TNode::CHANCE) c = c * p_public(N.via, ri, ro);
            else if (P.p == i) o = o * sg[(size_t)P.row * 9 + ri * 3 + N.via];
            else c = c * sg[(size_t)P.row * 9 + ro * 3 + N.via];
          }
          cf[(size_t)n * 9 + ri * 3 + ro] = c;
          if (ro == 0) own[(size_t)n * 3 + ri] = o;
        }
        __syncthreads();
      }
      // 3. counterfactual values of seat i, bottom-up
      for (int L = nlev - 1; L >= 0; --L) {
        const int n0 = T.lev[L], cnt = (T.lev[L + 1] - n0) * 3;
        for (int k = tid; k < cnt; k += nt) {
          const int n = n0 + k / 3, ri = k % 3;
          const DevNode& N = nodes[n];
          double v;
          if (N.kind == TNode::TERMINAL) v = terminal_value(T, N, i, ri, cf + (size_t)n * 9 + ri * 3);
          else if (N.kind == TNode::DECISION && N.p == i)
            v = weighted_children(N, val + ri, 3, sg + (size_t)N.row * 9 + ri * 3);
          else v = sum_children(N, val + ri, 3);
          val[(size_t)n * 3 + ri] = v;
        }
        __syncthreads();
      }
      // 4. regrets and strategy sums at seat i's decisions, then (1.) their new sigma
      for (int k = tid; k < nn * 3; k += nt) {
        const int n = k / 3, ri = k % 3;
        const DevNode& N = nodes[n];
        if (N.kind != TNode::DECISION || N.p != i) continue;
        const size_t row = (size_t)N.row * 9 + ri * 3;
        const double v = val[k], w = t * own[k];
        for (int a = 0; a < 3; ++a) {
          if (N.child[a] < 0) continue;
          const double r = (R[row + a] + val[(size_t)N.child[a] * 3 + ri]) - v;
          R[row + a] = r > 0.0 ? r : 0.0;
          S[row + a] = S[row + a] + w * sg[row + a];
        }
        match_row(R + row, N.child[2] >= 0, sg + row);
      }
      __syncthreads();
    }
  }
  for (int k = tid; k < ndec * 9; k += nt) {
    A.R[k] = R[k];
    A.S[k] = S[k];
  }
  for (int k = tid; k < ndec * 3; k += nt) average_row(S + 3 * k, T.legal[k / 3] & 1, A.avg + 3 * k);
}

}  // namespace

extern "C" int nfsp_cfr_create(nfsp_ctx* ctx, nfsp_cfr** out) {
  NFSP_REQUIRE(ctx && out, "null argument");
  const ExTables* T = nullptr;
  const int rc = device_tables(ctx, &T);
  if (rc != NFSP_OK) return rc;
  NFSP_REQUIRE(cfr_lds(T->nn, T->ndec) <= EX_MAX_LDS, "CFR+ tables exceed the LDS");
  nfsp_cfr* h = new nfsp_cfr;
  h->ctx = ctx;
  h->ndec = T->ndec;
  const size_t b = sizeof(double) * 9 * (size_t)h->ndec;
  hipError_t e = hipMalloc(&h->dev, 3 * b);
  if (e == hipSuccess) e = hipMemsetAsync(h->dev, 0, 3 * b, ctx->stream);
  if (e != hipSuccess) {
    if (h->dev) (void)hipFree(h->dev);
    delete h;
    return nfsp::hip_fail(e, "nfsp_cfr_create");
  }
  const int rc2 = nfsp_cfr_run(h, 0);   // the average before any iteration: uniform over legal actions
  if (rc2 != NFSP_OK) {
    (void)nfsp_cfr_destroy(h);
    return rc2;
  }
  *out = h;
  return NFSP_OK;
}

extern "C" int nfsp_cfr_run(nfsp_cfr* h, int64_t iters) {
  NFSP_REQUIRE(h, "null argument");
  NFSP_REQUIRE(iters >= 0, "iters must be >= 0");
  const ExTables* T = nullptr;
  const int rc = device_tables(h->ctx, &T);
  if (rc != NFSP_OK) return rc;
  NFSP_HIP(hipFuncSetAttribute((const void*)k_cfr_plus, hipFuncAttributeMaxDynamicSharedMemorySize, EX_MAX_LDS));
  const size_t n9 = 9 * (size_t)h->ndec;
  int64_t left = iters;
  do {
    const int m = (int)(left < NFSP_CFR_LAUNCH_ITERS ? left : NFSP_CFR_LAUNCH_ITERS);
    CfrArgs A{};
    A.T = *T;
    A.R = h->dev;
    A.S = h->dev + n9;
    A.avg = h->dev + 2 * n9;
    A.t0 = h->iterations;
    A.iters = m;
    k_cfr_plus<<<1, 256, cfr_lds(T->nn, T->ndec), h->ctx->stream>>>(A);
    NFSP_LAUNCHED("k_cfr_plus");
    h->iterations += m;
    left -= m;
  } while (left > 0);
  NFSP_HIP(hipStreamSynchronize(h->ctx->stream));
  return NFSP_OK;
}

extern "C" int nfsp_cfr_iterations(nfsp_cfr* h, int64_t* out) {
  NFSP_REQUIRE(h && out, "null argument");
  *out = h->iterations;
  return NFSP_OK;
}

extern "C" int nfsp_cfr_average(nfsp_cfr* h, const double** dev_table) {
  NFSP_REQUIRE(h && dev_table, "null argument");
  *dev_table = h->dev + 2 * 9 * (size_t)h->ndec;
  return NFSP_OK;
}

extern "C" int nfsp_cfr_state(nfsp_cfr* h, double* host_R, double* host_S) {
  NFSP_REQUIRE(h && host_R && host_S, "null argument");
  const size_t b = sizeof(double) * 9 * (size_t)h->ndec;
  NFSP_HIP(hipMemcpyAsync(host_R, h->dev, b, hipMemcpyDeviceToHost, h->ctx->stream));
  NFSP_HIP(hipMemcpyAsync(host_S, h->dev + 9 * (size_t)h->ndec, b, hipMemcpyDeviceToHost, h->ctx->stream));
  NFSP_HIP(hipStreamSynchronize(h->ctx->stream));
  return NFSP_OK;
}

extern "C" int nfsp_cfr_destroy(nfsp_cfr* h) {
  NFSP_REQUIRE(h, "null argument");
  if (h->dev) (void)hipFree(h->dev);
  delete h;
  return NFSP_OK;
}

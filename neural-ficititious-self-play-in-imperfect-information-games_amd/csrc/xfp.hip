// Full-width extensive-form fictitious play (XFP; Heinrich, Lanctot and Silver 2015) on the
// evaluator's public tree (exploit_tree.h): the algorithm NFSP samples and approximates, with an
// exact best response and exact averaging, so that its curve -- in nfsp_evaluate_batch's chips,
// on exactly the game the engine plays -- is what fictitious play itself does here.  The
// anticipatory variant responds to (1 - eta) x average + eta x last best response, mixed per
// hand: NFSP's eta.
//
// n independent runs (eta, weighting) in one launch, one workgroup of 256 per run.  Per run: the
// weighted sum S of the best responses' realisation plans, the last one's plan B (both
// [ndec][3 ranks][3]; B is 0 / 1, so S holds exact integers), the weight sum W.  Iteration
// t = 1, 2, .., with w = 1 (uniform weights) or t (linear):
//   1. sigma, every row: uniform over the legal actions while W = 0; else P = S (eta = 0) or
//      (1 - eta) (S / W) + eta B, sigma = P / ((P0 + P1) + P2), uniform where that sum is 0;
//   2. for each seat i, top-down: the counterfactual reach cf[ri][ro] of its ranks -- from a
//      chance parent x p_public, from the opponent's decision x sigma[opponent's rank], from its
//      own decision unchanged; bottom-up: a terminal sums cf x pay over the opponent's rank,
//      seat i's decision takes the first maximum over its legal children (a later action wins
//      only if strictly greater: nfsp_best_response_table's rule) and keeps the action as
//      beta_t, every other node sums its children;
//   3. gap_t = br_0 + br_1, br_i = 0.5 s(root[0]) + 0.5 s(root[1]), s = (v[0] + v[1]) + v[2]:
//      with eta = 0 the exploitability of the average after t - 1 iterations;
//   4. x = the own reach of beta_t top-down (1 at the roots, x beta_t at the acting seat's own
//      decisions); B = x beta_t;
//   5. S += w B, W += w.
// Both seats respond to the same sigma (simultaneous updates) and share the levels, as
// k_evaluate's evaluations do.  4, 5 and the next iteration's 1 ride on the next iteration's
// top-down sweep: at a level, the thread that owns (decision, rank) computes x there, then the
// row's B, S and sigma, which the level below reads after the barrier; a launch ends with one
// more sweep that only does 4 and 5.  So an iteration is 2 nlev barriers (Leduc, nlev = 8: 16)
// and a launch nlev + 2 more.  W is the same sum in every thread's registers; thread 0 writes
// the gap after the bottom-up sweep, inside the iteration.
// The reach, value and first-max steps are tree_walk.h's, so the sums are the evaluator's (no
// FMA contraction): tests/xfp_ref.py restates it in numpy, and S, B, W and the argmax path agree
// to the bit.
//
// LDS (f64): S, B, sigma [ndec][3][3], cf [nn][2][3][3], values and x [nn][2][3], then the node
// table and beta_t [ndec][3] as bytes -- Leduc (nn 364, ndec 130): 124,566 bytes.
#include "tree_walk.h"

struct nfsp_xfp {
  nfsp_ctx* ctx = nullptr;
  int ndec = 0, n = 0;
  int64_t iterations = 0;
  double* dev = nullptr;            // per run S | B | average ([ndec][3][3] each), then W [n], then gaps
  nfsp_xfp_cfg* dev_cfg = nullptr;  // [n]
};

namespace {

using namespace nfsp::ex;

struct XfpArgs {
  ExTables T;
  const nfsp_xfp_cfg* cfg;     // [n]
  double* state;               // [n][3][ndec][3][3]: S, B in and out; the average out
  double* W;                   // [n], in and out
  double* gaps;                // [n][iters], out
  long long t0;                // iterations done before this launch
  int iters;
};

__host__ __device__ inline size_t xfp_lds(int nn, int ndec) {
  return 8 * ((size_t)ndec * 27 + (size_t)nn * 18 + (size_t)nn * 12) + sizeof(DevNode) * (size_t)nn +
         (size_t)ndec * 3;
}

// step 1 on one row
__device__ inline void sigma_row(const double* S, const double* B, double W, double eta, bool legal_raise,
                                 double* sg) {
#pragma clang fp contract(off)
  double p[3] = {0.0, 0.0, 0.0};
  if (W != 0.0 && eta == 0.0) {
    for (int a = 0; a < 3; ++a) p[a] = S[a];
  } else if (W != 0.0) {
    const double k = 1.0 - eta;
    for (int a = 0; a < 3; ++a) p[a] = k * (S[a] / W) + eta * B[a];
  }
  average_row(p, legal_raise, sg);           // S and B are 0 at an illegal raise, so p[2] is too
}

struct XfpLds {
  double *S, *B, *sg, *cf, *val, *x;
  DevNode* nodes;
  uint8_t* beta;
};

// One top-down sweep.  update: steps 4 and 5 for the beta of the iteration before (weight w; W
// already includes it).  walk: step 1's sigma of the rows met and step 2's reach.  Every
// argument but L is uniform over the workgroup; nlev barriers.
__device__ inline void xfp_top_down(const ExTables& T, const XfpLds& M, bool update, bool walk, double w, double W,
                                    double eta) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int L = 0; L < T.nlev; ++L) {
    const int n0 = T.lev[L], cnt = (T.lev[L + 1] - n0) * 18;
    for (int k = tid; k < cnt; k += nt) {
      const int n = n0 + k / 18, i = (k / 9) % 2, ri = (k / 3) % 3, ro = k % 3;
      const DevNode& N = M.nodes[n];
      // both read the parent's level before either writes, so that the loads overlap
      double* item = M.cf + i * 9 + ri * 3 + ro;
      double c = 0.0, xo = 1.0;
      if (walk) c = reach_step(T, M.nodes, N, i, ri, ro, M.sg, item, 18, false);
      if (update && N.parent >= 0) {
        const DevNode& P = M.nodes[N.parent];
        xo = M.x[(size_t)N.parent * 6 + i * 3 + ri];
        if (P.kind == TNode::DECISION && P.p == i) xo = xo * (M.beta[P.row * 3 + ri] == N.via ? 1.0 : 0.0);
      }
      if (walk) item[(size_t)n * 18] = c;
      if (ro != 0) continue;
      // (node, seat i, its rank ri): the own reach, and at seat i's decision the row
      if (update) M.x[(size_t)n * 6 + i * 3 + ri] = xo;
      if (N.kind != TNode::DECISION || N.p != i) continue;
      const size_t row = (size_t)N.row * 9 + ri * 3;
      if (update) {
        const int b = M.beta[N.row * 3 + ri];
        for (int a = 0; a < 3; ++a) {
          const double Ba = xo * (a == b ? 1.0 : 0.0);
          M.B[row + a] = Ba;
          M.S[row + a] = M.S[row + a] + w * Ba;
        }
      }
      if (walk) sigma_row(M.S + row, M.B + row, W, eta, N.child[2] >= 0, M.sg + row);
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) k_xfp(XfpArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const ExTables& T = A.T;
  const int nn = T.nn, ndec = T.ndec, nlev = T.nlev;
  XfpLds M;
  M.S = reinterpret_cast<double*>(smem_raw);           // [ndec][3][3]
  M.B = M.S + (size_t)ndec * 9;
  M.sg = M.B + (size_t)ndec * 9;
  M.cf = M.sg + (size_t)ndec * 9;                      // [nn][seat i][ri][ro]
  M.val = M.cf + (size_t)nn * 18;                      // [nn][seat i][ri]
  M.x = M.val + (size_t)nn * 6;                        // [nn][seat][its rank]
  M.nodes = reinterpret_cast<DevNode*>(M.x + (size_t)nn * 6);
  M.beta = reinterpret_cast<uint8_t*>(M.nodes + nn);   // [ndec][3]: the action
  const int tid = threadIdx.x, nt = blockDim.x;
  const int run = blockIdx.x;
  const size_t n9 = (size_t)ndec * 9;
  double* gS = A.state + (size_t)run * 3 * n9;
  const double eta = A.cfg[run].eta;
  const bool linear = A.cfg[run].weight == NFSP_XFP_WEIGHT_LINEAR;
  double W = A.W[run];                                 // every thread carries the same sum
  for (size_t k = tid; k < n9; k += nt) {
    M.S[k] = gS[k];
    M.B[k] = gS[n9 + k];
  }
  for (int k = tid; k < nn; k += nt) M.nodes[k] = T.nodes[k];
  __syncthreads();
  double w = 0.0;                                      // the weight of the iteration before
  for (int it = 0; it < A.iters; ++it) {
    xfp_top_down(T, M, it > 0, true, w, W, eta);
    // 2. values of both seats, bottom-up; beta_t at the decisions
    for (int L = nlev - 1; L >= 0; --L) {
      const int n0 = T.lev[L], cnt = (T.lev[L + 1] - n0) * 6;
      for (int k = tid; k < cnt; k += nt) {
        const int n = n0 + k / 6, i = (k / 3) % 2, ri = k % 3;
        const DevNode& N = M.nodes[n];
        double* item = M.val + i * 3 + ri;
        double v;
        if (N.kind == TNode::TERMINAL) {
          v = terminal_value(T, N, i, ri, M.cf + (size_t)n * 18 + i * 9 + ri * 3);
        } else if (N.kind == TNode::DECISION && N.p == i) {
          int best;
          v = first_max_child(N, item, 6, best);
          M.beta[N.row * 3 + ri] = (uint8_t)best;
        } else {
          v = sum_children(N, item, 6);
        }
        item[(size_t)n * 6] = v;
      }
      __syncthreads();
    }
    // 3. the roots' values stand until the next bottom-up sweep ends
    if (tid == 0) A.gaps[(size_t)run * A.iters + it] = root_value(T, M.val, 6) + root_value(T, M.val + 3, 6);
    w = linear ? (double)(A.t0 + 1 + it) : 1.0;
    W = W + w;
  }
  if (A.iters > 0) xfp_top_down(T, M, true, false, w, W, eta);
  for (size_t k = tid; k < n9; k += nt) {
    gS[k] = M.S[k];
    gS[n9 + k] = M.B[k];
  }
  if (tid == 0) A.W[run] = W;
  for (int k = tid; k < ndec * 3; k += nt) average_row(M.S + 3 * k, T.legal[k / 3] & 1, gS + 2 * n9 + 3 * (size_t)k);
}

int check_cfg(const nfsp_xfp_cfg& c) {
  NFSP_REQUIRE(c.eta >= 0.0 && c.eta < 1.0, "nfsp_xfp_cfg.eta must be in [0, 1)");
  NFSP_REQUIRE(c.weight == NFSP_XFP_WEIGHT_UNIFORM || c.weight == NFSP_XFP_WEIGHT_LINEAR,
               "unknown nfsp_xfp_cfg.weight (NFSP_XFP_WEIGHT_*)");
  NFSP_REQUIRE(c.reserved == 0, "nfsp_xfp_cfg.reserved must be 0");
  return NFSP_OK;
}

}  // namespace

// Checks that need no handle or device come first, so that every rule answers without a GPU.
extern "C" int nfsp_xfp_create(nfsp_ctx* ctx, const nfsp_xfp_cfg* cfgs, int n, nfsp_xfp** out) {
  NFSP_REQUIRE(cfgs && out, "null argument");
  NFSP_REQUIRE(n >= 1 && n <= NFSP_XFP_MAX_RUNS, "n must be in 1 .. NFSP_XFP_MAX_RUNS");
  for (int k = 0; k < n; ++k) {
    const int rc = check_cfg(cfgs[k]);
    if (rc != NFSP_OK) return rc;
  }
  NFSP_REQUIRE(ctx, "null argument");
  const ExTables* T = nullptr;
  const int rc = device_tables(ctx, &T);
  if (rc != NFSP_OK) return rc;
  NFSP_REQUIRE(xfp_lds(T->nn, T->ndec) <= EX_MAX_LDS, "XFP tables exceed the LDS");
  nfsp_xfp* h = new nfsp_xfp;
  h->ctx = ctx;
  h->ndec = T->ndec;
  h->n = n;
  const size_t doubles = (size_t)n * (27 * (size_t)h->ndec + 1 + NFSP_XFP_LAUNCH_ITERS);
  hipError_t e = hipMalloc(&h->dev, sizeof(double) * doubles);
  if (e == hipSuccess) e = hipMalloc(&h->dev_cfg, sizeof(nfsp_xfp_cfg) * n);
  if (e == hipSuccess) e = hipMemsetAsync(h->dev, 0, sizeof(double) * doubles, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h->dev_cfg, cfgs, sizeof(nfsp_xfp_cfg) * n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // cfgs is the caller's
  if (e != hipSuccess) {
    (void)nfsp_xfp_destroy(h);
    return nfsp::hip_fail(e, "nfsp_xfp_create");
  }
  const int rc2 = nfsp_xfp_run(h, 0, nullptr);   // the average before any iteration: uniform over legal actions
  if (rc2 != NFSP_OK) {
    (void)nfsp_xfp_destroy(h);
    return rc2;
  }
  *out = h;
  return NFSP_OK;
}

extern "C" int nfsp_xfp_run(nfsp_xfp* h, int64_t iters, double* host_gaps) {
  NFSP_REQUIRE(iters >= 0, "iters must be >= 0");
  NFSP_REQUIRE(h, "null argument");
  const ExTables* T = nullptr;
  const int rc = device_tables(h->ctx, &T);
  if (rc != NFSP_OK) return rc;
  NFSP_HIP(hipFuncSetAttribute((const void*)k_xfp, hipFuncAttributeMaxDynamicSharedMemorySize, EX_MAX_LDS));
  const size_t n27 = 27 * (size_t)h->ndec;
  int64_t left = iters, done = 0;
  do {
    const int m = (int)(left < NFSP_XFP_LAUNCH_ITERS ? left : NFSP_XFP_LAUNCH_ITERS);
    XfpArgs A{};
    A.T = *T;
    A.cfg = h->dev_cfg;
    A.state = h->dev;
    A.W = h->dev + (size_t)h->n * n27;
    A.gaps = A.W + h->n;                         // [n][m] in this launch
    A.t0 = h->iterations;
    A.iters = m;
    k_xfp<<<h->n, 256, xfp_lds(T->nn, T->ndec), h->ctx->stream>>>(A);
    NFSP_LAUNCHED("k_xfp");
    if (host_gaps && m > 0)
      NFSP_HIP(hipMemcpy2DAsync(host_gaps + done, sizeof(double) * (size_t)iters, A.gaps, sizeof(double) * (size_t)m,
                                sizeof(double) * (size_t)m, (size_t)h->n, hipMemcpyDeviceToHost, h->ctx->stream));
    h->iterations += m;
    done += m;
    left -= m;
  } while (left > 0);
  NFSP_HIP(hipStreamSynchronize(h->ctx->stream));
  return NFSP_OK;
}

extern "C" int nfsp_xfp_iterations(nfsp_xfp* h, int64_t* out) {
  NFSP_REQUIRE(h && out, "null argument");
  *out = h->iterations;
  return NFSP_OK;
}

extern "C" int nfsp_xfp_average(nfsp_xfp* h, int run, const double** dev_table) {
  NFSP_REQUIRE(run >= 0, "run out of range");
  NFSP_REQUIRE(h && dev_table, "null argument");
  NFSP_REQUIRE(run < h->n, "run out of range");
  *dev_table = h->dev + ((size_t)run * 3 + 2) * 9 * (size_t)h->ndec;
  return NFSP_OK;
}

extern "C" int nfsp_xfp_state(nfsp_xfp* h, int run, double* host_S, double* host_B, double* W) {
  NFSP_REQUIRE(run >= 0, "run out of range");
  NFSP_REQUIRE(h && host_S && host_B && W, "null argument");
  NFSP_REQUIRE(run < h->n, "run out of range");
  const size_t n9 = 9 * (size_t)h->ndec;
  const double* s = h->dev + (size_t)run * 3 * n9;
  NFSP_HIP(hipMemcpyAsync(host_S, s, sizeof(double) * n9, hipMemcpyDeviceToHost, h->ctx->stream));
  NFSP_HIP(hipMemcpyAsync(host_B, s + n9, sizeof(double) * n9, hipMemcpyDeviceToHost, h->ctx->stream));
  NFSP_HIP(hipMemcpyAsync(W, h->dev + (size_t)h->n * 27 * (size_t)h->ndec + run, sizeof(double),
                          hipMemcpyDeviceToHost, h->ctx->stream));
  NFSP_HIP(hipStreamSynchronize(h->ctx->stream));
  return NFSP_OK;
}

extern "C" int nfsp_xfp_destroy(nfsp_xfp* h) {
  NFSP_REQUIRE(h, "null argument");
  if (h->dev) (void)hipFree(h->dev);
  if (h->dev_cfg) (void)hipFree(h->dev_cfg);
  delete h;
  return NFSP_OK;
}

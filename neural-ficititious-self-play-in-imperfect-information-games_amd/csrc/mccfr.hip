// External-sampling Monte-Carlo CFR (Lanctot, Waugh, Zinkevich and Bowling 2009) on the
// evaluator's public tree (exploit_tree.h): the sampled counterpart of cfr.hip's CFR+, as tabular
// NFSP is xfp.hip's -- what a plain sampled tabular learner reaches per traversal on exactly the
// game nfsp_evaluate_batch scores.  The rule is in include/nfsp.h; tests/mccfr_ref.py restates it
// in numpy, and R, S and the counts agree to the bit.
//
// The first solver here that is a throughput kernel, not one barrier-bound workgroup.  n
// independent runs (seed, W walkers).  A half-iteration (seat i updates) is two launches:
//   k_mccfr_walk   grid (workgroups over walkers, run), 256 lanes.  A workgroup stages the run's
//                  sigma (f64), the node table and seat i's half of pay into LDS beside zeroed
//                  int64 dR / dS (Leduc: 45 KB, so three workgroups share a CU's LDS), then each
//                  lane runs WG_WALKERS / 256 traversals in turn.  A traversal is a depth-first
//                  walk of seat i's own-action subtree with chance and the opponent sampled
//                  (Philox keyed by the node, so no draw depends on the order of the visit); its
//                  frames at seat i's decisions -- at most MAX_FRAMES on a path, checked against
//                  the tree at creation -- are the levels of a recursion the compiler unrolls into
//                  registers, and every loop is bounded by the tree's depth.  Lanes add
//                  llrint(x Q) into the LDS tables with 64-bit LDS atomics; after a barrier the
//                  workgroup adds its non-zero entries to the run's dR / dS in device memory with
//                  64-bit atomic adds (relaxed, agent scope).  Integer sums: the bits do not
//                  depend on the grid or on the order of arrival.
//   k_mccfr_apply  R += dR, S += dS, the deltas zeroed, the next sigma (regret matching on R+;
//                  R itself is not floored), the average of S, the counts.
// Outcome sampling (nfsp_mccfr_os_*, the same handle) swaps the walk for
//   k_mccfr_os_walk  the same grid, lane-to-walker mapping, LDS tables and flush.  A traversal is
//                  one sampled hand: a straight path down (seat i samples its own action from
//                  eps uniform + (1 - eps) sigma and carries the product q of what it sampled with),
//                  one terminal, then the path's frames back, deepest first, with importance
//                  weights 1 / q.  The frames are 16 bits each in one 64-bit scalar, sigma is
//                  re-read from LDS by row, and the one pay entry comes from device memory, so pay
//                  is not staged (Leduc: 36,824 B of LDS, four workgroups to a CU).
// Baseline-corrected outcome sampling (nfsp_mccfr_vr_*, VR-MCCFR, the same handle) swaps it for
//   k_mccfr_vr_walk  outcome sampling's grid, mapping, path down and flush.  Both seats' decisions
//                  are frames (8 of 16 bits in two scalars); the terminal's pay is carried back up
//                  them, corrected at each by the frozen baseline B (f64, staged beside sigma), and
//                  every frame adds its sample to dBs / dBn beside dR / dS (Leduc: 64,904 B of LDS,
//                  two workgroups to a CU).
//   k_mccfr_vr_apply  after k_mccfr_apply: Bs += dBs, Bn += dBn, the deltas zeroed, the next B.
// Regret matching+ and linear averaging (nfsp_mccfr_x_*, the same handle, any of the three walks)
// swap both applies for
//   k_mccfr_x_apply  one launch: R += dR and, per run, its floor at 0; S += dS; the f64 linear sum
//                  Sw += (t + 1) dS; the next sigma, both averages, the counts, and with baselines
//                  k_mccfr_vr_apply's part for the thread's three entries.
// Regret nets (nfsp_mccfr_net_*, the same handle, any of the three walks) add after it
//   k_mccfr_net_apply  grid (2 seats, n runs), 512 lanes, one workgroup per (run, seat) with the
//                  seat's 30-64-3 net, its momentum state and the seat's rows in LDS as
//                  k_fit_tables holds them (fit_step.h).  A handle of nfsp_mccfr_net_create_h with
//                  another width H launches k_mccfr_net_apply_w<H>: the same kernel text
//                  (mccfr_net_apply_kernel.inc) at that width, one width per handle.  The workgroup of the seat that walked
//                  turns R into targets and runs the run's K full-batch steps; every workgroup
//                  then takes one forward and writes the heads z and the sigma the next walk
//                  reads for its seat's rows.  k_mccfr_x_apply's regret matching on R goes to a
//                  table beside (sigma_tab).
// No workgroup waits for another -- no flags, no tickets, no spinning: the stream orders the
// launches, and nfsp_mccfr_run synchronises once at its end.
// All f64 arithmetic is in tree_walk.h's style (no FMA contraction, the sums ascending).
#include <stdio.h>

#include <vector>

#include "fit_step.h"
#include "tree_walk.h"

struct nfsp_mccfr {
  nfsp_ctx* ctx = nullptr;
  int ndec = 0, nterm = 0, n = 0, max_walkers = 0;
  int64_t iterations = 0;
  std::vector<nfsp_mccfr_cfg> cfgs;
  long long* state = nullptr;             // per run R | S | dR | dS, [ndec][3][3] each
  double* tabs = nullptr;                 // per run sigma | average, [ndec][3][3] each
  unsigned long long* counts = nullptr;   // per run traversals, terminals, terminals of the walk in flight
  nfsp_mccfr_cfg* dev_cfg = nullptr;      // [n]
  int sampling = 0;                       // 0 external, 1 outcome, 2 outcome with baselines
  std::vector<nfsp_mccfr_os_cfg> os_cfgs; // outcome sampling: the cfgs as given (cfgs holds their seed and walkers)
  std::vector<double> eps;                // outcome sampling: [n][3] epsilon, epsilon / 2.0, epsilon / 3.0
  double* dev_eps = nullptr;              // eps on the device
  std::vector<nfsp_mccfr_vr_cfg> vr_cfgs; // with baselines: the cfgs as given (os_cfgs holds the same fields)
  long long* bstate = nullptr;            // with baselines: per run Bs | Bn | dBs | dBn, [ndec][3][3] each
  double* btab = nullptr;                 // with baselines: per run B, [ndec][3][3]
  double maxpay = 0.0;                    // with baselines: P, the game's max|pay|
  std::vector<nfsp_mccfr_x_cfg> x_cfgs;   // nfsp_mccfr_x_create: the cfgs as given (empty for the other kinds)
  int32_t* dev_rule = nullptr;            // that kind: per run regret, average
  double* sw = nullptr;                   // that kind: per run Sw, [ndec][3][3]
  double* avg2 = nullptr;                 // that kind: per run the average cfg.average does not name
  std::vector<nfsp_mccfr_net_cfg> net_cfgs;   // nfsp_mccfr_net_create: the cfgs as given (x_cfgs holds their rule)
  void* dev_net = nullptr;                // that kind: per run target, K, loss, lr, momentum (NetDevCfg)
  int32_t* net_rows = nullptr;            // that kind: [2][FIT_SEAT_ROWS], a seat's decision rows, ascending
  int net_nrows[2] = {0, 0};
  int net_hidden = nfsp::nn::H;           // that kind: the nets' width, one per handle (fit_step.h FIT_WIDTHS)
  float* net_w = nullptr;                 // that kind: per run and seat the net, NP f32
  float* net_v = nullptr;                 // that kind: per run and seat its momentum state
  float* net_z = nullptr;                 // that kind: per run the heads, [ndec][3][3]
  double* sigma_tab = nullptr;            // that kind: per run regret matching on R (tabs holds the nets' sigma)
  double* net_loss = nullptr;             // that kind: per run and seat the loss before and after the last fit
  bool timing = false;                    // nfsp_mccfr_set_timing: events around the walks and the applies
  double ms_walk = 0.0, ms_apply = 0.0;   // summed over the half-iterations timed
  int64_t timed = 0;                      // iterations timed
};

namespace {

using namespace nfsp::ex;

constexpr int WALK_THREADS = 256;
constexpr int MAX_FRAMES = 4;             // seat i's decisions on one path (Leduc: 4, Kuhn: 2)
constexpr double Q = (double)NFSP_MCCFR_Q;
static_assert(NFSP_MCCFR_WG_WALKERS % WALK_THREADS == 0, "a lane runs a whole number of traversals");

struct WalkArgs {
  ExTables T;
  const nfsp_mccfr_cfg* cfg;              // [n]
  const double* tabs;                     // [n][2][ndec][3][3]: sigma first
  long long* state;                       // [n][4][ndec][3][3]: dR, dS are the last two
  unsigned long long* counts;             // [n][3]
  uint32_t h_lo, h_hi;                    // the half-iteration index
  int seat, nterm;
};

struct ApplyArgs {
  const uint8_t* legal;
  const nfsp_mccfr_cfg* cfg;
  long long* state;
  double* tabs;
  unsigned long long* counts;
  int ndec;
  int walked;                             // 1: a walk went before (0: the tables of creation)
};

// dynamic LDS: sigma f64, dR and dS int64, the terminal count, then the node table and pay
__host__ __device__ inline size_t walk_lds(int nn, int ndec, int nterm) {
  return 8 * ((size_t)ndec * 27 + 1) + sizeof(DevNode) * (size_t)nn + 4 * 9 * (size_t)nterm;
}

struct Walker {
  const double* sg;                       // LDS
  const DevNode* nodes;
  const float* pay;                       // [nterm][r_i][r_o], seat i's
  unsigned long long *dR, *dS;
  uint32_t h_lo, h_hi, w, k0, k1;
  int i, ri, ro, nlev;
  uint32_t terminals;
};

__device__ __forceinline__ double draw(const Walker& X, int node) {
  const uint32_t x = nfsp::philox4x32({X.h_lo, X.h_hi, X.w, (uint32_t)node}, X.k0, X.k1).x;
  return (double)(x >> 8) * 5.9604644775390625e-08;
}

// One step of the rule's choice: c is the running sum, pick the first j with u < c_j and p_j > 0,
// last the last j with p_j > 0.
__device__ __forceinline__ void choice_step(double p, int j, double u, double& c, int& pick, int& last) {
#pragma clang fp contract(off)
  c = c + p;
  if (p > 0.0) {
    last = j;
    if (pick < 0 && u < c) pick = j;
  }
}

__device__ __forceinline__ int choose3(double p0, double p1, double p2, double u) {
  double c = 0.0;
  int pick = -1, last = -1;
  choice_step(p0, 0, u, c, pick, last);
  choice_step(p1, 1, u, c, pick, last);
  choice_step(p2, 2, u, c, pick, last);
  return pick >= 0 ? pick : last;
}

__device__ __forceinline__ void add_fixed(unsigned long long* p, double x) {
  const long long v = (long long)__builtin_rint(x);    // llrint: |x| <= 2 max|pay| Q (omega max|pay| Q), far inside int64
  if (v != 0) atomicAdd(p, (unsigned long long)v);
}

// Traverse(n) with D of seat i's decisions above it.  The node is read where it lies in LDS (a
// copy indexed by the action would go to scratch).
template <int D>
__device__ __forceinline__ double traverse(Walker& X, int n) {
#pragma clang fp contract(off)
  for (int d = 0; d < X.nlev; ++d) {
    const DevNode& N = X.nodes[n];
    if (N.kind == TNode::TERMINAL) {
      ++X.terminals;
      return (double)X.pay[(size_t)N.row * 9 + X.ri * 3 + X.ro];
    }
    if (N.kind == TNode::DECISION && N.p == X.i) {
      if constexpr (D < MAX_FRAMES) {
        double v0 = 0.0, v1 = 0.0, v2 = 0.0;
#pragma nounroll
        for (int a = 0; a < 3; ++a) {
          const int c = N.child[a];
          if (c < 0) continue;
          const double x = traverse<D + 1>(X, c);
          if (a == 0) v0 = x;
          else if (a == 1) v1 = x;
          else v2 = x;
        }
        const size_t row = (size_t)N.row * 9 + X.ri * 3;
        const bool l0 = N.child[0] >= 0, l1 = N.child[1] >= 0, l2 = N.child[2] >= 0;
        double v = 0.0;
        if (l0) v = v + X.sg[row + 0] * v0;
        if (l1) v = v + X.sg[row + 1] * v1;
        if (l2) v = v + X.sg[row + 2] * v2;
        if (l0) add_fixed(X.dR + row + 0, (v0 - v) * Q);
        if (l1) add_fixed(X.dR + row + 1, (v1 - v) * Q);
        if (l2) add_fixed(X.dR + row + 2, (v2 - v) * Q);
        return v;
      } else {
        return 0.0;                       // unreachable: nfsp_mccfr_create counted the frames
      }
    }
    const double u = draw(X, n);
    double p0, p1, p2;
    if (N.kind == TNode::CHANCE) {
      const int r0 = X.i == 0 ? X.ri : X.ro, r1 = X.i == 0 ? X.ro : X.ri;
      p0 = p_public(0, r0, r1);
      p1 = p_public(1, r0, r1);
      p2 = p_public(2, r0, r1);
    } else {
      const size_t row = (size_t)N.row * 9 + X.ro * 3;
      p0 = X.sg[row + 0];
      p1 = X.sg[row + 1];
      p2 = X.sg[row + 2];
      add_fixed(X.dS + row + 0, p0 * Q);
      add_fixed(X.dS + row + 1, p1 * Q);
      add_fixed(X.dS + row + 2, p2 * Q);
    }
    const int a = choose3(p0, p1, p2, u);
    if (a < 0) return 0.0;                // no positive probability: not a strategy
    n = N.child[a];
    if (n < 0) return 0.0;
  }
  return 0.0;
}

__global__ void __launch_bounds__(WALK_THREADS) k_mccfr_walk(WalkArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const ExTables& T = A.T;
  const int run = blockIdx.y;
  const int W = A.cfg[run].walkers;
  const int w0 = blockIdx.x * NFSP_MCCFR_WG_WALKERS;
  if (w0 >= W) return;                    // the grid is sized for the run with the most walkers
  const int nn = T.nn, n9 = T.ndec * 9;
  double* sg = reinterpret_cast<double*>(smem_raw);
  unsigned long long* dR = reinterpret_cast<unsigned long long*>(sg + n9);
  unsigned long long* dS = dR + n9;
  unsigned long long* terms = dS + n9;
  DevNode* nodes = reinterpret_cast<DevNode*>(terms + 1);
  float* pay = reinterpret_cast<float*>(nodes + nn);
  const int tid = threadIdx.x;
  const double* gsg = A.tabs + (size_t)run * 2 * n9;
  for (int k = tid; k < n9; k += WALK_THREADS) {
    sg[k] = gsg[k];
    dR[k] = 0;
    dS[k] = 0;
  }
  if (tid == 0) *terms = 0;
  for (int k = tid; k < nn; k += WALK_THREADS) nodes[k] = T.nodes[k];
  for (int k = tid; k < A.nterm * 9; k += WALK_THREADS) pay[k] = T.pay[(size_t)(k / 9) * 18 + A.seat * 9 + k % 9];
  __syncthreads();

  Walker X;
  X.sg = sg;
  X.nodes = nodes;
  X.pay = pay;
  X.dR = dR;
  X.dS = dS;
  X.h_lo = A.h_lo;
  X.h_hi = A.h_hi;
  X.k0 = (uint32_t)A.cfg[run].seed;
  X.k1 = (uint32_t)(A.cfg[run].seed >> 32);
  X.i = A.seat;
  X.nlev = T.nlev;
  X.terminals = 0;
  for (int k = 0; k < NFSP_MCCFR_WG_WALKERS / WALK_THREADS; ++k) {
    const int w = w0 + k * WALK_THREADS + tid;
    if (w >= W) continue;
    X.w = (uint32_t)w;
    // the deal, at the pseudo-node nn over deal[a][b] in row-major order
    const double u = draw(X, nn);
    double c = 0.0;
    int pick = -1, last = -1;
#pragma unroll
    for (int j = 0; j < 9; ++j) choice_step(T.deal[j / 3][j % 3], j, u, c, pick, last);
    const int j = pick >= 0 ? pick : last;
    if (j < 0) continue;                  // no deal has a positive probability: not a game
    X.ri = j / 3;
    X.ro = j % 3;
    (void)traverse<0>(X, T.root[w & 1]);
  }
  if (X.terminals) atomicAdd(terms, (unsigned long long)X.terminals);
  __syncthreads();

  long long* gd = A.state + ((size_t)run * 4 + 2) * n9;    // dR | dS, as in LDS
  for (int k = tid; k < 2 * n9; k += WALK_THREADS) {
    const unsigned long long v = dR[k];
    if (v)
      __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(gd) + k, v, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid == 0 && *terms)
    __hip_atomic_fetch_add(A.counts + (size_t)run * 3 + 2, *terms, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct OsArgs {
  ExTables T;
  const nfsp_mccfr_cfg* cfg;              // [n]
  const double* eps;                      // [n][3]: epsilon, epsilon / 2.0, epsilon / 3.0 (divided on the host)
  const double* tabs;
  long long* state;
  unsigned long long* counts;
  uint32_t h_lo, h_hi;
  int seat;
};

// dynamic LDS of the outcome-sampling walk: as walk_lds without pay
__host__ __device__ inline size_t os_lds(int nn, int ndec) {
  return 8 * ((size_t)ndec * 27 + 1) + sizeof(DevNode) * (size_t)nn;
}

// A frame of the path, 16 bits: row << 3 | raise legal << 2 | a*.  MAX_FRAMES of them are one
// 64-bit scalar, the deepest in the low bits (nfsp_mccfr_os_create checks the rows fit).
constexpr int FRAME_BITS = 16;
constexpr int FRAME_MAX_ROWS = 1 << (FRAME_BITS - 3);
static_assert(MAX_FRAMES * FRAME_BITS <= 64, "the frames of a path are one scalar");

// Outcome sampling: the grid, the lane-to-walker mapping, the LDS tables and the flush are
// k_mccfr_walk's; a traversal is one path down (nlev steps at most) and its frames back
// (MAX_FRAMES at most).  Two kinds of division: Q / q at an opponent's node, pay / q at the end.
// The staging, the deal and the flush are written out again here: shared with k_mccfr_walk as
// inlined helpers they moved that kernel's registers (91 -> 94 VGPRs), and its code is to stay
// the parent's, instruction for instruction (profiles/mccfr/resources_os.txt).
__global__ void __launch_bounds__(WALK_THREADS) k_mccfr_os_walk(OsArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const ExTables& T = A.T;
  const int run = blockIdx.y;
  const int W = A.cfg[run].walkers;
  const int w0 = blockIdx.x * NFSP_MCCFR_WG_WALKERS;
  if (w0 >= W) return;
  const int nn = T.nn, n9 = T.ndec * 9;
  double* sg = reinterpret_cast<double*>(smem_raw);
  unsigned long long* dR = reinterpret_cast<unsigned long long*>(sg + n9);
  unsigned long long* dS = dR + n9;
  unsigned long long* terms = dS + n9;
  DevNode* nodes = reinterpret_cast<DevNode*>(terms + 1);
  const int tid = threadIdx.x;
  const double* gsg = A.tabs + (size_t)run * 2 * n9;
  for (int k = tid; k < n9; k += WALK_THREADS) {
    sg[k] = gsg[k];
    dR[k] = 0;
    dS[k] = 0;
  }
  if (tid == 0) *terms = 0;
  for (int k = tid; k < nn; k += WALK_THREADS) nodes[k] = T.nodes[k];
  __syncthreads();

  Walker X;
  X.sg = sg;
  X.nodes = nodes;
  X.pay = T.pay + A.seat * 9;             // device memory: a traversal reads one entry
  X.dR = dR;
  X.dS = dS;
  X.h_lo = A.h_lo;
  X.h_hi = A.h_hi;
  X.k0 = (uint32_t)A.cfg[run].seed;
  X.k1 = (uint32_t)(A.cfg[run].seed >> 32);
  X.i = A.seat;
  X.nlev = T.nlev;
  X.terminals = 0;
  const double eps = A.eps[run * 3], eps2 = A.eps[run * 3 + 1], eps3 = A.eps[run * 3 + 2];
  const double keep = 1.0 - eps;
  for (int k = 0; k < NFSP_MCCFR_WG_WALKERS / WALK_THREADS; ++k) {
    const int w = w0 + k * WALK_THREADS + tid;
    if (w >= W) continue;
    X.w = (uint32_t)w;
    const double ud = draw(X, nn);
    double cd = 0.0;
    int pick = -1, last = -1;
#pragma unroll
    for (int j = 0; j < 9; ++j) choice_step(T.deal[j / 3][j % 3], j, ud, cd, pick, last);
    const int j = pick >= 0 ? pick : last;
    if (j < 0) continue;
    X.ri = j / 3;
    X.ro = j % 3;
    // the path down
    int n = T.root[w & 1], nf = 0, end = -1;
    double q = 1.0;
    uint64_t frames = 0;
    for (int d = 0; d < X.nlev; ++d) {
      const DevNode& N = X.nodes[n];
      if (N.kind == TNode::TERMINAL) {
        end = N.row;
        break;
      }
      const double u = draw(X, n);
      const bool own = N.kind == TNode::DECISION && N.p == X.i;
      const bool l2 = N.child[2] >= 0;
      double p0, p1, p2;
      if (N.kind == TNode::CHANCE) {
        const int r0 = X.i == 0 ? X.ri : X.ro, r1 = X.i == 0 ? X.ro : X.ri;
        p0 = p_public(0, r0, r1);
        p1 = p_public(1, r0, r1);
        p2 = p_public(2, r0, r1);
      } else {
        const size_t row = (size_t)N.row * 9 + (own ? X.ri : X.ro) * 3;
        p0 = X.sg[row + 0];
        p1 = X.sg[row + 1];
        p2 = X.sg[row + 2];
        if (own) {
          const double e = l2 ? eps3 : eps2;
          p0 = e + keep * p0;
          p1 = e + keep * p1;
          p2 = l2 ? e + keep * p2 : 0.0;
        } else {
          const double winv = Q / q;
          add_fixed(X.dS + row + 0, p0 * winv);
          add_fixed(X.dS + row + 1, p1 * winv);
          add_fixed(X.dS + row + 2, p2 * winv);
        }
      }
      const int a = choose3(p0, p1, p2, u);
      if (a < 0) break;                   // no positive probability: not a strategy
      if (own) {
        if (nf >= MAX_FRAMES) break;      // unreachable: nfsp_mccfr_os_create counted the frames
        frames = frames << FRAME_BITS | (uint64_t)(N.row << 3 | (l2 ? 4 : 0) | a);
        ++nf;
        q = q * (a == 0 ? p0 : a == 1 ? p1 : p2);
      }
      n = N.child[a];
      if (n < 0) break;
    }
    if (end < 0) continue;
    ++X.terminals;
    // the frames back, deepest first
    const double c = (double)X.pay[(size_t)end * 18 + X.ri * 3 + X.ro] / q;
    double x = 1.0;
    for (int f = 0; f < MAX_FRAMES; ++f) {
      if (f >= nf) break;
      const uint32_t fr = (uint32_t)frames & ((1u << FRAME_BITS) - 1);
      frames >>= FRAME_BITS;
      const int a = fr & 3;
      const size_t row = (size_t)(fr >> 3) * 9 + X.ri * 3;
      const double s = X.sg[row + a], g = c * x;
      const double hit = (g * (1.0 - s)) * Q, miss = (-(g * s)) * Q;
      add_fixed(X.dR + row + 0, a == 0 ? hit : miss);
      add_fixed(X.dR + row + 1, a == 1 ? hit : miss);
      if (fr & 4) add_fixed(X.dR + row + 2, a == 2 ? hit : miss);
      x = x * s;
    }
  }
  if (X.terminals) atomicAdd(terms, (unsigned long long)X.terminals);
  __syncthreads();

  long long* gd = A.state + ((size_t)run * 4 + 2) * n9;    // dR | dS, as in LDS
  for (int k = tid; k < 2 * n9; k += WALK_THREADS) {
    const unsigned long long v = dR[k];
    if (v)
      __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(gd) + k, v, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid == 0 && *terms)
    __hip_atomic_fetch_add(A.counts + (size_t)run * 3 + 2, *terms, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct VrArgs {
  ExTables T;
  const nfsp_mccfr_cfg* cfg;              // [n]
  const double* eps;                      // [n][3], as OsArgs
  const double* tabs;
  const double* btab;                     // [n][ndec][3][3]: B, frozen for the half-iteration
  long long* state;
  long long* bstate;                      // [n][4][ndec][3][3]: dBs, dBn are the last two
  unsigned long long* counts;
  uint32_t h_lo, h_hi;
  int seat;
};

// dynamic LDS of the baseline-corrected walk: sigma and B f64, dR, dS, dBs and dBn int64, the
// terminal count, the node table
__host__ __device__ inline size_t vr_lds(int nn, int ndec) {
  return 8 * ((size_t)ndec * 54 + 1) + sizeof(DevNode) * (size_t)nn;
}

// A frame of the baseline-corrected path, 16 bits: row << 4 | seat i's << 3 | raise legal << 2 | a*.
// Both seats' decisions are frames, 2 MAX_FRAMES of them at most: two 64-bit scalars, the deepest
// in the low bits of the first (nfsp_mccfr_vr_create checks the rows fit).
constexpr int VR_FRAME_MAX_ROWS = 1 << (FRAME_BITS - 4);
static_assert(2 * MAX_FRAMES * FRAME_BITS <= 128, "the frames of a path are two scalars");

// Baseline-corrected outcome sampling: the grid, the lane-to-walker mapping, the staging, the path
// down with its dS and the flush are k_mccfr_os_walk's (written out again, as that kernel's are);
// B is staged beside sigma and dBs / dBn lie beside dR / dS.  The way down pushes a frame at both
// seats' decisions and keeps q before seat i's second, third and fourth factor (before the first
// it is 1.0) in three registers chosen by compares, never by an index; xi_{a*} is formed again on
// the way back from the same sigma and eps by the same two operations, so its bits are the
// rule's.  Divisions: Q / q at an opponent's node on the way down; on the way back one by
// xi_{a*} and one by qk per legal action at seat i's frames, none at the opponent's or the end.
__global__ void __launch_bounds__(WALK_THREADS) k_mccfr_vr_walk(VrArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const ExTables& T = A.T;
  const int run = blockIdx.y;
  const int W = A.cfg[run].walkers;
  const int w0 = blockIdx.x * NFSP_MCCFR_WG_WALKERS;
  if (w0 >= W) return;
  const int nn = T.nn, n9 = T.ndec * 9;
  double* sg = reinterpret_cast<double*>(smem_raw);
  double* B = sg + n9;
  unsigned long long* dR = reinterpret_cast<unsigned long long*>(B + n9);
  unsigned long long* dS = dR + n9;
  unsigned long long* dBs = dS + n9;
  unsigned long long* dBn = dBs + n9;
  unsigned long long* terms = dBn + n9;
  DevNode* nodes = reinterpret_cast<DevNode*>(terms + 1);
  const int tid = threadIdx.x;
  const double* gsg = A.tabs + (size_t)run * 2 * n9;
  const double* gB = A.btab + (size_t)run * n9;
  for (int k = tid; k < n9; k += WALK_THREADS) {
    sg[k] = gsg[k];
    B[k] = gB[k];
    dR[k] = 0;
    dS[k] = 0;
    dBs[k] = 0;
    dBn[k] = 0;
  }
  if (tid == 0) *terms = 0;
  for (int k = tid; k < nn; k += WALK_THREADS) nodes[k] = T.nodes[k];
  __syncthreads();

  Walker X;
  X.sg = sg;
  X.nodes = nodes;
  X.pay = T.pay + A.seat * 9;             // device memory: a traversal reads one entry
  X.dR = dR;
  X.dS = dS;
  X.h_lo = A.h_lo;
  X.h_hi = A.h_hi;
  X.k0 = (uint32_t)A.cfg[run].seed;
  X.k1 = (uint32_t)(A.cfg[run].seed >> 32);
  X.i = A.seat;
  X.nlev = T.nlev;
  X.terminals = 0;
  const double eps = A.eps[run * 3], eps2 = A.eps[run * 3 + 1], eps3 = A.eps[run * 3 + 2];
  const double keep = 1.0 - eps;
  for (int k = 0; k < NFSP_MCCFR_WG_WALKERS / WALK_THREADS; ++k) {
    const int w = w0 + k * WALK_THREADS + tid;
    if (w >= W) continue;
    X.w = (uint32_t)w;
    const double ud = draw(X, nn);
    double cd = 0.0;
    int pick = -1, last = -1;
#pragma unroll
    for (int j = 0; j < 9; ++j) choice_step(T.deal[j / 3][j % 3], j, ud, cd, pick, last);
    const int j = pick >= 0 ? pick : last;
    if (j < 0) continue;
    X.ri = j / 3;
    X.ro = j % 3;
    // the path down: outcome sampling's, with a frame at every decision
    int n = T.root[w & 1], nf = 0, no = 0, end = -1;
    double q = 1.0, qk1 = 1.0, qk2 = 1.0, qk3 = 1.0;
    uint64_t flo = 0, fhi = 0;
    for (int d = 0; d < X.nlev; ++d) {
      const DevNode& N = X.nodes[n];
      if (N.kind == TNode::TERMINAL) {
        end = N.row;
        break;
      }
      const double u = draw(X, n);
      const bool dec = N.kind == TNode::DECISION;
      const bool own = dec && N.p == X.i;
      const bool l2 = N.child[2] >= 0;
      double p0, p1, p2;
      if (!dec) {
        const int r0 = X.i == 0 ? X.ri : X.ro, r1 = X.i == 0 ? X.ro : X.ri;
        p0 = p_public(0, r0, r1);
        p1 = p_public(1, r0, r1);
        p2 = p_public(2, r0, r1);
      } else {
        const size_t row = (size_t)N.row * 9 + (own ? X.ri : X.ro) * 3;
        p0 = X.sg[row + 0];
        p1 = X.sg[row + 1];
        p2 = X.sg[row + 2];
        if (own) {
          const double e = l2 ? eps3 : eps2;
          p0 = e + keep * p0;
          p1 = e + keep * p1;
          p2 = l2 ? e + keep * p2 : 0.0;
        } else {
          const double winv = Q / q;
          add_fixed(X.dS + row + 0, p0 * winv);
          add_fixed(X.dS + row + 1, p1 * winv);
          add_fixed(X.dS + row + 2, p2 * winv);
        }
      }
      const int a = choose3(p0, p1, p2, u);
      if (a < 0) break;                   // no positive probability: not a strategy
      if (dec) {
        if (nf >= 2 * MAX_FRAMES || (own && no >= MAX_FRAMES)) break;    // unreachable: creation counted the frames
        fhi = fhi << FRAME_BITS | flo >> (64 - FRAME_BITS);
        flo = flo << FRAME_BITS | (uint64_t)(N.row << 4 | (own ? 8 : 0) | (l2 ? 4 : 0) | a);
        ++nf;
        if (own) {
          qk1 = no == 1 ? q : qk1;        // qk of seat i's frame `no`; frame 0's is 1.0
          qk2 = no == 2 ? q : qk2;
          qk3 = no == 3 ? q : qk3;
          ++no;
          q = q * (a == 0 ? p0 : a == 1 ? p1 : p2);
        }
      }
      n = N.child[a];
      if (n < 0) break;
    }
    if (end < 0) continue;
    ++X.terminals;
    // the frames back, deepest first
    double v = (double)X.pay[(size_t)end * 18 + X.ri * 3 + X.ro];
    for (int f = 0; f < 2 * MAX_FRAMES; ++f) {
      if (f >= nf) break;
      const uint32_t fr = (uint32_t)flo & ((1u << FRAME_BITS) - 1);
      flo = flo >> FRAME_BITS | fhi << (64 - FRAME_BITS);
      fhi >>= FRAME_BITS;
      const int a = fr & 3;
      const bool own = fr & 8, l2 = fr & 4;
      const size_t row = (size_t)(fr >> 4) * 9 + (own ? X.ri : X.ro) * 3;
      const double s0 = X.sg[row + 0], s1 = X.sg[row + 1], s2 = X.sg[row + 2];
      atomicAdd(dBn + row + a, 1ull);
      if (!own) {
        const double b0 = -B[row + 0], b1 = -B[row + 1], b2 = l2 ? -B[row + 2] : 0.0;
        const double ba = a == 0 ? b0 : a == 1 ? b1 : b2;
        add_fixed(dBs + row + a, (-v) * Q);
        v = ((s0 * b0 + s1 * b1) + s2 * b2) + (v - ba);
      } else {
        const double b0 = B[row + 0], b1 = B[row + 1], b2 = B[row + 2];
        const double ba = a == 0 ? b0 : a == 1 ? b1 : b2;
        add_fixed(dBs + row + a, v * Q);
        --no;
        const double qk = no == 0 ? 1.0 : no == 1 ? qk1 : no == 2 ? qk2 : qk3;
        const double xi = (l2 ? eps3 : eps2) + keep * (a == 0 ? s0 : a == 1 ? s1 : s2);
        const double hit = ba + (v - ba) / xi;
        const double u0 = a == 0 ? hit : b0, u1 = a == 1 ? hit : b1, u2 = a == 2 ? hit : b2;
        double vbar = 0.0;
        vbar = vbar + s0 * u0;
        vbar = vbar + s1 * u1;
        if (l2) vbar = vbar + s2 * u2;
        add_fixed(X.dR + row + 0, ((u0 - vbar) / qk) * Q);
        add_fixed(X.dR + row + 1, ((u1 - vbar) / qk) * Q);
        if (l2) add_fixed(X.dR + row + 2, ((u2 - vbar) / qk) * Q);
        v = vbar;
      }
    }
  }
  if (X.terminals) atomicAdd(terms, (unsigned long long)X.terminals);
  __syncthreads();

  long long* gd = A.state + ((size_t)run * 4 + 2) * n9;    // dR | dS, as in LDS
  long long* gb = A.bstate + ((size_t)run * 4 + 2) * n9;   // dBs | dBn, as in LDS
  for (int k = tid; k < 2 * n9; k += WALK_THREADS) {
    const unsigned long long v = dR[k], b = dBs[k];
    if (v)
      __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(gd) + k, v, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    if (b)
      __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(gb) + k, b, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid == 0 && *terms)
    __hip_atomic_fetch_add(A.counts + (size_t)run * 3 + 2, *terms, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct VrApplyArgs {
  long long* bstate;
  double* btab;
  int ndec;
  double maxpay;                          // P
};

// The baseline's step 3, one thread per entry of a run: Bs += dBs, Bn += dBn, the deltas zeroed,
// and the next B = clamp((double)Bs / ((double)Bn * Q), -P, P), 0 where Bn is 0.
__global__ void __launch_bounds__(256) k_mccfr_vr_apply(VrApplyArgs A) {
#pragma clang fp contract(off)
  const int run = blockIdx.y;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n9 = (size_t)A.ndec * 9;
  if (k >= (int)n9) return;
  long long* Bs = A.bstate + (size_t)run * 4 * n9 + k;
  long long* Bn = Bs + n9;
  long long* dBs = Bn + n9;
  long long* dBn = dBs + n9;
  const long long s = *Bs + *dBs, c = *Bn + *dBn;
  *Bs = s;
  *Bn = c;
  *dBs = 0;
  *dBn = 0;
  double b = 0.0;
  if (c > 0) {
    b = (double)s / ((double)c * Q);
    b = b < -A.maxpay ? -A.maxpay : b > A.maxpay ? A.maxpay : b;
  }
  A.btab[(size_t)run * n9 + k] = b;
}

// One thread per (row, rank) of a run.
__global__ void __launch_bounds__(256) k_mccfr_apply(ApplyArgs A) {
#pragma clang fp contract(off)
  const int run = blockIdx.y;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n9 = (size_t)A.ndec * 9;
  if (k == 0 && A.walked) {
    unsigned long long* c = A.counts + (size_t)run * 3;
    c[0] += (unsigned long long)A.cfg[run].walkers;
    c[1] += c[2];
    c[2] = 0;
  }
  if (k >= A.ndec * 3) return;
  long long* R = A.state + (size_t)run * 4 * n9 + 3 * (size_t)k;
  long long* S = R + n9;
  long long* dR = S + n9;
  long long* dS = dR + n9;
  const bool legal_raise = A.legal[k / 3] & 1;
  double rp[3], s[3];
  for (int a = 0; a < 3; ++a) {
    const long long r = R[a] + dR[a], t = S[a] + dS[a];
    R[a] = r;
    S[a] = t;
    dR[a] = 0;
    dS[a] = 0;
    rp[a] = (double)(r > 0 ? r : 0);
    s[a] = (double)t;
  }
  if (!legal_raise) rp[2] = 0.0;
  double* sg = A.tabs + (size_t)run * 2 * n9 + 3 * (size_t)k;
  average_row(rp, legal_raise, sg);
  average_row(s, legal_raise, sg + n9);
}

struct XApplyArgs {
  const uint8_t* legal;
  const nfsp_mccfr_cfg* cfg;
  const int32_t* rule;                    // [n][2]: regret, average
  long long* state;
  double* tabs;                           // slot 1: the average the run's cfg names
  double* sw;                             // [n][ndec][3][3]
  double* avg2;                           // [n][ndec][3][3]: the other average
  double* sigma_tab;                      // [n][ndec][3][3]: where regret matching on R goes instead of tabs'
                                          // slot 0, which then holds the nets' sigma; null without nets
  unsigned long long* counts;
  long long* bstate;                      // null without baselines
  double* btab;
  double maxpay;                          // P
  double tw;                              // (double)(t + 1), t the iterations completed before this one
  int ndec;
  int walked;
};

// Step 3 of the kind nfsp_mccfr_x_create makes, one thread per (row, rank) of a run: what
// k_mccfr_apply does, with the run's floor on R, the linear sum Sw beside S and both averages;
// then, with baselines, what k_mccfr_vr_apply does for this thread's three entries.
__global__ void __launch_bounds__(256) k_mccfr_x_apply(XApplyArgs A) {
#pragma clang fp contract(off)
  const int run = blockIdx.y;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n9 = (size_t)A.ndec * 9;
  if (k == 0 && A.walked) {
    unsigned long long* c = A.counts + (size_t)run * 3;
    c[0] += (unsigned long long)A.cfg[run].walkers;
    c[1] += c[2];
    c[2] = 0;
  }
  if (k >= A.ndec * 3) return;
  const bool plus = A.rule[2 * run] == NFSP_MCCFR_REGRET_PLUS;
  const bool linear = A.rule[2 * run + 1] == NFSP_MCCFR_AVG_LINEAR;
  long long* R = A.state + (size_t)run * 4 * n9 + 3 * (size_t)k;
  long long* S = R + n9;
  long long* dR = S + n9;
  long long* dS = dR + n9;
  double* Sw = A.sw + (size_t)run * n9 + 3 * (size_t)k;
  const bool legal_raise = A.legal[k / 3] & 1;
  double rp[3], s[3], sl[3];
  for (int a = 0; a < 3; ++a) {
    long long r = R[a] + dR[a];
    if (plus && r < 0) r = 0;
    const long long t = S[a] + dS[a];
    const double w = Sw[a] + A.tw * (double)dS[a];
    R[a] = r;
    S[a] = t;
    Sw[a] = w;
    dR[a] = 0;
    dS[a] = 0;
    rp[a] = (double)(r > 0 ? r : 0);
    s[a] = (double)t;
    sl[a] = w;
  }
  if (!legal_raise) rp[2] = 0.0;
  double* sg = A.tabs + (size_t)run * 2 * n9 + 3 * (size_t)k;
  double* other = A.avg2 + (size_t)run * n9 + 3 * (size_t)k;
  average_row(rp, legal_raise, A.sigma_tab ? A.sigma_tab + (size_t)run * n9 + 3 * (size_t)k : sg);
  average_row(s, legal_raise, linear ? other : sg + n9);
  average_row(sl, legal_raise, linear ? sg + n9 : other);
  if (!A.bstate) return;
  long long* Bs = A.bstate + (size_t)run * 4 * n9 + 3 * (size_t)k;
  long long* Bn = Bs + n9;
  long long* dBs = Bn + n9;
  long long* dBn = dBs + n9;
  double* B = A.btab + (size_t)run * n9 + 3 * (size_t)k;
  for (int a = 0; a < 3; ++a) {
    const long long bs = Bs[a] + dBs[a], c = Bn[a] + dBn[a];
    Bs[a] = bs;
    Bn[a] = c;
    dBs[a] = 0;
    dBn[a] = 0;
    double b = 0.0;
    if (c > 0) {
      b = (double)bs / ((double)c * Q);
      b = b < -A.maxpay ? -A.maxpay : b > A.maxpay ? A.maxpay : b;
    }
    B[a] = b;
  }
}

struct NetDevCfg {
  int32_t target, steps, loss;
  float lr, mu;
};

struct NetApplyArgs {
  const NetDevCfg* net;                   // [n]
  const nfsp_mccfr_cfg* cfg;              // [n]: W
  const int32_t* rows;                    // [2][FIT_SEAT_ROWS]
  const uint32_t* obs;                    // [ndec][3]
  const uint8_t* legal;                   // [ndec]
  const long long* state;                 // R is the first of a run's four tables
  double* tabs;                           // slot 0: the nets' sigma
  float* z;                               // [n][ndec][3][3]
  float* w;                               // [n][2][NP]
  float* v;                               // [n][2][NP]
  double* loss;                           // [n][2][2]
  double tw;                              // (double)(t + 1); 1.0 at creation
  int32_t nrows[2];
  int ndec;
  int fitseat;                            // the seat that walked; 2: both (creation)
};

// The nets' step of a half-iteration, one workgroup per (seat, run): k_fit_tables with the targets
// made here from R and the head turned into sigma.  `fits`, the step count and every row count are
// uniform over the workgroup; the two single-thread regions (the loss sums) lie outside the step
// loop.
__global__ void __launch_bounds__(nfsp::fit::FIT_WG) k_mccfr_net_apply(NetApplyArgs A) {
#include "mccfr_net_apply_kernel.inc"
}

// the same text at another width: one instantiation per entry of fit::FIT_WIDTHS but 64
template <int HH>
__global__ void __launch_bounds__(nfsp::fit::FIT_WG) k_mccfr_net_apply_w(NetApplyArgs A) {
  FIT_WIDTH_NAMES(HH);
  {
#include "mccfr_net_apply_kernel.inc"
  }
}

using NetApplyKernel = void (*)(NetApplyArgs);
NetApplyKernel net_apply_kernel(int hidden) {
  switch (hidden) {
    case 16: return k_mccfr_net_apply_w<16>;
    case 32: return k_mccfr_net_apply_w<32>;
    case 64: return k_mccfr_net_apply;
    case 128: return k_mccfr_net_apply_w<128>;
  }
  return nullptr;
}

int frames_below(const HostTables& H, int n, int i) {
  if (n < 0) return 0;
  const DevNode& N = H.nodes[n];
  int m = 0;
  for (int a = 0; a < 3; ++a) m = std::max(m, frames_below(H, N.child[a], i));
  return m + (N.kind == TNode::DECISION && N.p == i);
}

// The rule's omega: the largest product of L_k / eps over seat i's decisions on a path from n
// down, w the product above n.  Every factor is >= 1, so the largest is at a terminal.
double omega_below(const HostTables& H, int n, int i, double eps, double w) {
  if (n < 0) return 0.0;
  const DevNode& N = H.nodes[n];
  if (N.kind == TNode::DECISION && N.p == i) w = w * ((double)N.nchild / eps);
  double m = w;
  for (int a = 0; a < 3; ++a) m = std::max(m, omega_below(H, N.child[a], i, eps, w));
  return m;
}

// The rule's overflow recursion of the baseline-corrected walk, |B| <= P, for seat i (the node
// table is in depth order, parents first).  Vmax(n) bounds |v| at n:
//   terminal P; chance the most of its children; the opponent's 2 P + the most of its children;
//   seat i's with L legal actions P + (the most of its children + P) * ((double)L / eps).
// rmax: the most of (2 Vmax(n)) * (the product of L_k / eps over seat i's decisions above n) over
// seat i's decisions, what one traversal moves an R entry by; bmax: the most Vmax of a
// decision's child (either seat's), what it moves a Bs entry by.  Both in chips, both only raised.
void vr_bounds(const HostTables& H, int i, double P, double eps, double& rmax, double& bmax) {
  const int nn = (int)H.nodes.size();
  std::vector<double> vmax(nn, 0.0), w(nn, 1.0);
  for (int n = nn - 1; n >= 0; --n) {
    const DevNode& N = H.nodes[n];
    double m = 0.0;
    for (int a = 0; a < 3; ++a)
      if (N.child[a] >= 0) m = std::max(m, vmax[N.child[a]]);
    if (N.kind == TNode::TERMINAL) vmax[n] = P;
    else if (N.kind == TNode::CHANCE) vmax[n] = m;
    else if (N.p != i) vmax[n] = 2.0 * P + m;
    else vmax[n] = P + (m + P) * ((double)N.nchild / eps);
    if (N.kind == TNode::DECISION) bmax = std::max(bmax, m);
  }
  for (int n = 0; n < nn; ++n) {
    const DevNode& N = H.nodes[n];
    if (N.parent >= 0) {
      const DevNode& U = H.nodes[N.parent];
      w[n] = w[N.parent];
      if (U.kind == TNode::DECISION && U.p == i) w[n] = w[N.parent] * ((double)U.nchild / eps);
    }
    if (N.kind == TNode::DECISION && N.p == i) rmax = std::max(rmax, (2.0 * vmax[n]) * w[n]);
  }
}

int launch_vr_apply(nfsp_mccfr* h) {
  VrApplyArgs A{};
  A.bstate = h->bstate;
  A.btab = h->btab;
  A.ndec = h->ndec;
  A.maxpay = h->maxpay;
  k_mccfr_vr_apply<<<dim3(nfsp_blocks(9 * (int64_t)h->ndec, 256), h->n), 256, 0, h->ctx->stream>>>(A);
  NFSP_LAUNCHED("k_mccfr_vr_apply");
  return NFSP_OK;
}

// t: the iterations completed before the one in progress
int launch_x_apply(nfsp_mccfr* h, const ExTables& T, int walked, int64_t t) {
  XApplyArgs A{};
  A.legal = T.legal;
  A.cfg = h->dev_cfg;
  A.rule = h->dev_rule;
  A.state = h->state;
  A.tabs = h->tabs;
  A.sw = h->sw;
  A.avg2 = h->avg2;
  A.sigma_tab = h->sigma_tab;
  A.counts = h->counts;
  A.bstate = h->bstate;
  A.btab = h->btab;
  A.maxpay = h->maxpay;
  A.tw = (double)(t + 1);
  A.ndec = h->ndec;
  A.walked = walked;
  k_mccfr_x_apply<<<dim3(nfsp_blocks(3 * (int64_t)h->ndec, 256), h->n), 256, 0, h->ctx->stream>>>(A);
  NFSP_LAUNCHED("k_mccfr_x_apply");
  return NFSP_OK;
}

size_t net_lds(const nfsp_mccfr* h) {
  const int nm = (std::max(h->net_nrows[0], h->net_nrows[1]) * 3 + 3) & ~3;
  return sizeof(float) * nfsp::fit::fit_lds_floats_h(h->net_hidden, nm);
}

// fitseat: the seat that walked, 2 at creation; t as launch_x_apply's
int launch_net_apply(nfsp_mccfr* h, const ExTables& T, int fitseat, int64_t t) {
  NetApplyArgs A{};
  A.net = (const NetDevCfg*)h->dev_net;
  A.cfg = h->dev_cfg;
  A.rows = h->net_rows;
  A.obs = T.obs;
  A.legal = T.legal;
  A.state = h->state;
  A.tabs = h->tabs;
  A.z = h->net_z;
  A.w = h->net_w;
  A.v = h->net_v;
  A.loss = h->net_loss;
  A.tw = (double)(t + 1);
  A.nrows[0] = h->net_nrows[0];
  A.nrows[1] = h->net_nrows[1];
  A.ndec = h->ndec;
  A.fitseat = fitseat;
  net_apply_kernel(h->net_hidden)<<<dim3(2, h->n), nfsp::fit::FIT_WG, net_lds(h), h->ctx->stream>>>(A);
  NFSP_LAUNCHED("k_mccfr_net_apply");
  return NFSP_OK;
}

int launch_apply(nfsp_mccfr* h, const ExTables& T, int walked) {
  ApplyArgs A{};
  A.legal = T.legal;
  A.cfg = h->dev_cfg;
  A.state = h->state;
  A.tabs = h->tabs;
  A.counts = h->counts;
  A.ndec = h->ndec;
  A.walked = walked;
  k_mccfr_apply<<<dim3(nfsp_blocks(3 * (int64_t)h->ndec, 256), h->n), 256, 0, h->ctx->stream>>>(A);
  NFSP_LAUNCHED("k_mccfr_apply");
  return NFSP_OK;
}

}  // namespace

extern "C" int nfsp_mccfr_cfgs_check(int game, const nfsp_mccfr_cfg* cfgs, int n, int64_t iters) {
  NFSP_REQUIRE(cfgs, "null argument");
  NFSP_REQUIRE(n >= 1 && n <= NFSP_MCCFR_MAX_RUNS, "n must be in 1 .. NFSP_MCCFR_MAX_RUNS");
  NFSP_REQUIRE(iters >= 0, "iters must be >= 0");
  const HostTables* H = nullptr;
  const int rc = host_tables(game, &H);
  if (rc != NFSP_OK) return rc;
  float maxpay = 1.f;                     // max|pay| of the game's table (taken as at least a chip)
  for (float p : H->pay) maxpay = std::max(maxpay, p < 0 ? -p : p);
  // an entry moves by at most 2 max|pay| Q per traversal: keep W x iterations x that <= 2^62
  const int64_t bound = (int64_t)((double)(1ll << 62) / (Q * 2.0 * (double)maxpay));
  for (int k = 0; k < n; ++k) {
    const nfsp_mccfr_cfg& c = cfgs[k];
    NFSP_REQUIRE(c.walkers >= 2 && c.walkers <= NFSP_MCCFR_MAX_WALKERS,
                 "nfsp_mccfr_cfg.walkers must be in 2 .. NFSP_MCCFR_MAX_WALKERS");
    NFSP_REQUIRE(c.walkers % 2 == 0, "nfsp_mccfr_cfg.walkers must be even (one dealer each in turn)");
    NFSP_REQUIRE(c.reserved == 0, "nfsp_mccfr_cfg.reserved must be 0");
    if (iters > bound / c.walkers) {
      char msg[200];
      snprintf(msg, sizeof msg,
               "overflow: walkers x iterations = %d x %lld would pass the bound %lld (2^62 / (2^24 x 2 max|pay|), "
               "max|pay| = %g chips)", c.walkers, (long long)iters, (long long)bound, (double)maxpay);
      return nfsp::fail(NFSP_EINVAL, msg);
    }
  }
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_os_cfgs_check(int game, const nfsp_mccfr_os_cfg* cfgs, int n, int64_t iters) {
  NFSP_REQUIRE(cfgs, "null argument");
  NFSP_REQUIRE(n >= 1 && n <= NFSP_MCCFR_MAX_RUNS, "n must be in 1 .. NFSP_MCCFR_MAX_RUNS");
  NFSP_REQUIRE(iters >= 0, "iters must be >= 0");
  const HostTables* H = nullptr;
  const int rc = host_tables(game, &H);
  if (rc != NFSP_OK) return rc;
  float maxpay = 1.f;
  for (float p : H->pay) maxpay = std::max(maxpay, p < 0 ? -p : p);
  for (int k = 0; k < n; ++k) {
    const nfsp_mccfr_os_cfg& c = cfgs[k];
    NFSP_REQUIRE(c.walkers >= 2 && c.walkers <= NFSP_MCCFR_MAX_WALKERS,
                 "nfsp_mccfr_os_cfg.walkers must be in 2 .. NFSP_MCCFR_MAX_WALKERS");
    NFSP_REQUIRE(c.walkers % 2 == 0, "nfsp_mccfr_os_cfg.walkers must be even (one dealer each in turn)");
    NFSP_REQUIRE(c.reserved == 0, "nfsp_mccfr_os_cfg.reserved must be 0");
    NFSP_REQUIRE(c.epsilon >= NFSP_MCCFR_OS_EPS_MIN && c.epsilon <= 1.0,       // false for a NaN
                 "nfsp_mccfr_os_cfg.epsilon must be in NFSP_MCCFR_OS_EPS_MIN .. 1");
    double omega = 1.0;
    for (int d = 0; d < 2; ++d)
      for (int i = 0; i < 2; ++i) omega = std::max(omega, omega_below(*H, H->root[d], i, c.epsilon, 1.0));
    // per traversal an R entry moves by at most max|pay| omega Q, an S entry by at most omega Q
    const int64_t bound = (int64_t)((double)(1ll << 62) / ((Q * (double)maxpay) * omega));
    if (iters > bound / c.walkers) {
      char msg[256];
      snprintf(msg, sizeof msg,
               "overflow: walkers x iterations = %d x %lld would pass the bound %lld (2^62 / (2^24 x max|pay| x omega), "
               "max|pay| = %g chips, omega = %g at epsilon = %g)", c.walkers, (long long)iters, (long long)bound,
               (double)maxpay, omega, c.epsilon);
      return nfsp::fail(NFSP_EINVAL, msg);
    }
  }
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_vr_cfgs_check(int game, const nfsp_mccfr_vr_cfg* cfgs, int n, int64_t iters) {
  NFSP_REQUIRE(cfgs, "null argument");
  NFSP_REQUIRE(n >= 1 && n <= NFSP_MCCFR_MAX_RUNS, "n must be in 1 .. NFSP_MCCFR_MAX_RUNS");
  NFSP_REQUIRE(iters >= 0, "iters must be >= 0");
  const HostTables* H = nullptr;
  const int rc = host_tables(game, &H);
  if (rc != NFSP_OK) return rc;
  float maxpay = 0.f;                     // P: the clamp of B, so the table's own max|pay|
  for (float p : H->pay) maxpay = std::max(maxpay, p < 0 ? -p : p);
  for (int k = 0; k < n; ++k) {
    const nfsp_mccfr_vr_cfg& c = cfgs[k];
    NFSP_REQUIRE(c.walkers >= 2 && c.walkers <= NFSP_MCCFR_MAX_WALKERS,
                 "nfsp_mccfr_vr_cfg.walkers must be in 2 .. NFSP_MCCFR_MAX_WALKERS");
    NFSP_REQUIRE(c.walkers % 2 == 0, "nfsp_mccfr_vr_cfg.walkers must be even (one dealer each in turn)");
    NFSP_REQUIRE(c.reserved == 0, "nfsp_mccfr_vr_cfg.reserved must be 0");
    NFSP_REQUIRE(c.epsilon >= NFSP_MCCFR_OS_EPS_MIN && c.epsilon <= 1.0,       // false for a NaN
                 "nfsp_mccfr_vr_cfg.epsilon must be in NFSP_MCCFR_OS_EPS_MIN .. 1");
    double omega = 1.0, rmax = 0.0, bmax = 0.0;
    for (int d = 0; d < 2; ++d)
      for (int i = 0; i < 2; ++i) omega = std::max(omega, omega_below(*H, H->root[d], i, c.epsilon, 1.0));
    for (int i = 0; i < 2; ++i) vr_bounds(*H, i, (double)maxpay, c.epsilon, rmax, bmax);
    // per traversal an R entry moves by at most Rmax Q, a Bs entry by Bmax Q, an S entry by omega Q
    const double most = std::max(std::max(rmax, bmax), omega);
    const int64_t bound = (int64_t)((double)(1ll << 62) / (Q * most));
    if (iters > bound / c.walkers) {
      char msg[320];
      snprintf(msg, sizeof msg,
               "overflow: walkers x iterations = %d x %lld would pass the bound %lld (2^62 / (2^24 x max(Rmax, Bmax, "
               "omega)), Rmax = %g and Bmax = %g chips, omega = %g at epsilon = %g, max|pay| = %g chips)", c.walkers,
               (long long)iters, (long long)bound, rmax, bmax, omega, c.epsilon, (double)maxpay);
      return nfsp::fail(NFSP_EINVAL, msg);
    }
  }
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_x_cfgs_check(int game, const nfsp_mccfr_x_cfg* cfgs, int n, int64_t iters) {
  NFSP_REQUIRE(cfgs, "null argument");
  NFSP_REQUIRE(n >= 1 && n <= NFSP_MCCFR_MAX_RUNS, "n must be in 1 .. NFSP_MCCFR_MAX_RUNS");
  NFSP_REQUIRE(iters >= 0, "iters must be >= 0");
  NFSP_REQUIRE(game == NFSP_GAME_LEDUC || game == NFSP_GAME_KUHN, "unknown game");
  for (int k = 0; k < n; ++k) {
    const nfsp_mccfr_x_cfg& c = cfgs[k];
    NFSP_REQUIRE(c.walkers >= 2 && c.walkers <= NFSP_MCCFR_MAX_WALKERS,
                 "nfsp_mccfr_x_cfg.walkers must be in 2 .. NFSP_MCCFR_MAX_WALKERS");
    NFSP_REQUIRE(c.walkers % 2 == 0, "nfsp_mccfr_x_cfg.walkers must be even (one dealer each in turn)");
    NFSP_REQUIRE(c.sampling >= 0 && c.sampling <= 2,
                 "nfsp_mccfr_x_cfg.sampling must be 0 (external), 1 (outcome) or 2 (outcome with baselines)");
    if (c.sampling != cfgs[0].sampling) {
      char msg[200];
      snprintf(msg, sizeof msg,
               "nfsp_mccfr_x_cfg.sampling of run %d is %d, run 0's is %d: one walk kernel serves a launch, so a handle "
               "has one sampling kind", k, c.sampling, cfgs[0].sampling);
      return nfsp::fail(NFSP_EINVAL, msg);
    }
    if (c.sampling == 0)
      NFSP_REQUIRE(c.epsilon == 0.0, "nfsp_mccfr_x_cfg.epsilon must be 0.0 under sampling 0 (external sampling has none)");
    else
      NFSP_REQUIRE(c.epsilon >= NFSP_MCCFR_OS_EPS_MIN && c.epsilon <= 1.0,       // false for a NaN
                   "nfsp_mccfr_x_cfg.epsilon must be in NFSP_MCCFR_OS_EPS_MIN .. 1");
    NFSP_REQUIRE(c.regret == NFSP_MCCFR_REGRET_PLAIN || c.regret == NFSP_MCCFR_REGRET_PLUS,
                 "nfsp_mccfr_x_cfg.regret must be NFSP_MCCFR_REGRET_PLAIN or NFSP_MCCFR_REGRET_PLUS");
    NFSP_REQUIRE(c.average == NFSP_MCCFR_AVG_UNIFORM || c.average == NFSP_MCCFR_AVG_LINEAR,
                 "nfsp_mccfr_x_cfg.average must be NFSP_MCCFR_AVG_UNIFORM or NFSP_MCCFR_AVG_LINEAR");
  }
  // the fields hold: what is left of the sampling kind's own check is its overflow bound (the floor
  // only shrinks |R + dR|, so the bound on the sum of |dR| still bounds R; Sw is f64)
  if (cfgs[0].sampling == 0) {
    std::vector<nfsp_mccfr_cfg> es(n);
    for (int k = 0; k < n; ++k) es[k] = nfsp_mccfr_cfg{cfgs[k].seed, cfgs[k].walkers, 0};
    return nfsp_mccfr_cfgs_check(game, es.data(), n, iters);
  }
  if (cfgs[0].sampling == 1) {
    std::vector<nfsp_mccfr_os_cfg> os(n);
    for (int k = 0; k < n; ++k) os[k] = nfsp_mccfr_os_cfg{cfgs[k].seed, cfgs[k].walkers, 0, cfgs[k].epsilon};
    return nfsp_mccfr_os_cfgs_check(game, os.data(), n, iters);
  }
  std::vector<nfsp_mccfr_vr_cfg> vr(n);
  for (int k = 0; k < n; ++k) vr[k] = nfsp_mccfr_vr_cfg{cfgs[k].seed, cfgs[k].walkers, 0, cfgs[k].epsilon};
  return nfsp_mccfr_vr_cfgs_check(game, vr.data(), n, iters);
}

extern "C" int nfsp_mccfr_net_cfgs_check(int game, const nfsp_mccfr_net_cfg* cfgs, int n, int64_t iters) {
  NFSP_REQUIRE(cfgs, "null argument");
  NFSP_REQUIRE(n >= 1 && n <= NFSP_MCCFR_MAX_RUNS, "n must be in 1 .. NFSP_MCCFR_MAX_RUNS");
  NFSP_REQUIRE(iters >= 0, "iters must be >= 0");
  NFSP_REQUIRE(game == NFSP_GAME_LEDUC || game == NFSP_GAME_KUHN, "unknown game");
  std::vector<nfsp_mccfr_x_cfg> x(n);
  for (int k = 0; k < n; ++k) {
    const nfsp_mccfr_net_cfg& c = cfgs[k];
    const auto bad = [k](const char* what) {
      char msg[256];
      snprintf(msg, sizeof msg, "nfsp_mccfr_net_cfg.%s (run %d)", what, k);
      return nfsp::fail(NFSP_EINVAL, msg);
    };
    if (!(c.walkers >= 2 && c.walkers <= NFSP_MCCFR_MAX_WALKERS))
      return bad("walkers must be in 2 .. NFSP_MCCFR_MAX_WALKERS");
    if (c.walkers % 2 != 0) return bad("walkers must be even (one dealer each in turn)");
    if (!(c.sampling >= 0 && c.sampling <= 2))
      return bad("sampling must be 0 (external), 1 (outcome) or 2 (outcome with baselines)");
    if (c.sampling != cfgs[0].sampling)
      return bad("sampling differs from run 0's: one walk kernel serves a launch, so a handle has one sampling kind");
    if (c.sampling == 0) {
      if (!(c.epsilon == 0.0)) return bad("epsilon must be 0.0 under sampling 0 (external sampling has none)");
    } else if (!(c.epsilon >= NFSP_MCCFR_OS_EPS_MIN && c.epsilon <= 1.0)) {      // true for a NaN
      return bad("epsilon must be in NFSP_MCCFR_OS_EPS_MIN .. 1");
    }
    if (c.regret != NFSP_MCCFR_REGRET_PLAIN && c.regret != NFSP_MCCFR_REGRET_PLUS)
      return bad("regret must be NFSP_MCCFR_REGRET_PLAIN or NFSP_MCCFR_REGRET_PLUS");
    if (c.average != NFSP_MCCFR_AVG_UNIFORM && c.average != NFSP_MCCFR_AVG_LINEAR)
      return bad("average must be NFSP_MCCFR_AVG_UNIFORM or NFSP_MCCFR_AVG_LINEAR");
    if (c.target != NFSP_MCCFR_NET_TARGET_AVG && c.target != NFSP_MCCFR_NET_TARGET_ROWMAX)
      return bad("target must be NFSP_MCCFR_NET_TARGET_AVG or NFSP_MCCFR_NET_TARGET_ROWMAX");
    if (!(c.fit_steps >= 0 && c.fit_steps <= NFSP_MCCFR_NET_MAX_STEPS))
      return bad("fit_steps must be in 0 .. NFSP_MCCFR_NET_MAX_STEPS");
    if (c.loss != NFSP_FIT_MSE && c.loss != NFSP_FIT_HUBER)
      return bad("loss must be NFSP_FIT_MSE or NFSP_FIT_HUBER (the heads are linear)");
    if (!(std::isfinite(c.lr) && c.lr >= 0.f)) return bad("lr must be finite and >= 0");
    if (!(c.momentum >= 0.f && c.momentum < 1.f)) return bad("momentum must be in [0, 1)");
    if (c.reserved != 0) return bad("reserved must be 0");
    x[k] = nfsp_mccfr_x_cfg{c.seed, c.walkers, c.sampling, c.epsilon, c.regret, c.average};
  }
  // the fields hold: what is left is the sampling kind's own overflow bound, which does not depend
  // on sigma and so not on the nets
  return nfsp_mccfr_x_cfgs_check(game, x.data(), n, iters);
}

namespace {

// What every kind of handle is made of, after its checks: cfgs holds every run's seed and
// walkers; os is null for external sampling; sampling 2 adds the baseline's tables, all 0; x (the
// cfgs of nfsp_mccfr_x_create) adds the per-run rule, Sw and the second average, and its own apply;
// net (the cfgs of nfsp_mccfr_net_create, with x) adds the nets from dev_w0, their tables and their apply.
int create_handle(nfsp_ctx* ctx, const nfsp_mccfr_cfg* cfgs, const nfsp_mccfr_os_cfg* os, int n, nfsp_mccfr** out,
                  int sampling = -1, const nfsp_mccfr_x_cfg* x = nullptr, const nfsp_mccfr_net_cfg* net = nullptr,
                  const float* const* dev_w0 = nullptr, int hidden = nfsp::nn::H) {
  const HostTables* H = nullptr;
  int rc = host_tables(ctx->game, &H);
  if (rc != NFSP_OK) return rc;
  for (int d = 0; d < 2; ++d)
    for (int i = 0; i < 2; ++i)
      NFSP_REQUIRE(frames_below(*H, H->root[d], i) <= MAX_FRAMES, "a seat decides more than 4 times on a path");
  const ExTables* T = nullptr;
  rc = device_tables(ctx, &T);
  if (rc != NFSP_OK) return rc;
  const int nterm = (int)(H->pay.size() / 18);
  if (sampling < 0) sampling = os ? 1 : 0;
  const bool vr = sampling == 2;
  if (vr) {
    NFSP_REQUIRE(vr_lds(T->nn, T->ndec) <= 64 * 1024, "MCCFR tables exceed 64 KB of LDS");
    NFSP_REQUIRE(T->ndec <= VR_FRAME_MAX_ROWS, "a decision row does not fit a frame");
  } else if (os) {
    NFSP_REQUIRE(os_lds(T->nn, T->ndec) <= 64 * 1024, "MCCFR tables exceed 64 KB of LDS");
    NFSP_REQUIRE(T->ndec <= FRAME_MAX_ROWS, "a decision row does not fit a frame");
  } else {
    NFSP_REQUIRE(walk_lds(T->nn, T->ndec, nterm) <= 64 * 1024, "MCCFR tables exceed 64 KB of LDS");
  }
  // the nets: the seats' rows as nfsp_fit_tables takes them, and the initial nets to the host once,
  // refused unless finite -- before anything is allocated or launched
  std::vector<int32_t> rows;
  std::vector<float> w0;
  int nrows[2] = {0, 0};
  if (net) {
    using namespace nfsp::fit;
    int64_t lds_need = 0;
    rc = nfsp_fit_width_check(ctx->game, hidden, &lds_need);
    if (rc != NFSP_OK) return rc;
    const size_t NP = fit_np(hidden);               // the width's, not nn's
    rows.assign(2 * FIT_SEAT_ROWS, 0);
    for (int d = 0; d < T->ndec; ++d) {
      const int s = H->legal[d] >> 1;
      NFSP_REQUIRE(s <= 1 && nrows[s] < FIT_SEAT_ROWS,
                   "nfsp_mccfr_net_create: the seat has more rows than the kernel holds");
      rows[s * FIT_SEAT_ROWS + nrows[s]++] = d;
    }
    const int nm = (std::max(nrows[0], nrows[1]) * 3 + 3) & ~3;
    NFSP_REQUIRE(sizeof(float) * fit_lds_floats_h(hidden, nm) == (size_t)lds_need && lds_need <= EX_MAX_LDS,
                 "nfsp_mccfr_net_create: the rows do not fit in LDS");
    w0.resize((size_t)n * 2 * NP);
    for (int k = 0; k < 2 * n; ++k)
      NFSP_HIP(hipMemcpyAsync(w0.data() + (size_t)k * NP, dev_w0[k], sizeof(float) * NP, hipMemcpyDeviceToHost,
                              ctx->stream));
    NFSP_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t e = 0; e < w0.size(); ++e)
      if (!std::isfinite(w0[e])) {
        char msg[160];
        snprintf(msg, sizeof msg, "nfsp_mccfr_net_create: run %d seat %d: dev_w0 is not finite at parameter %d",
                 (int)(e / NP / 2), (int)(e / NP % 2), (int)(e % NP));
        return nfsp::fail(NFSP_EINVAL, msg);
      }
  }
  nfsp_mccfr* h = new nfsp_mccfr;
  h->ctx = ctx;
  h->ndec = T->ndec;
  h->nterm = nterm;
  h->n = n;
  h->cfgs.assign(cfgs, cfgs + n);
  for (int k = 0; k < n; ++k) h->max_walkers = std::max(h->max_walkers, (int)cfgs[k].walkers);
  std::vector<double>& eps = h->eps;
  if (os) {
    h->sampling = sampling;
    h->os_cfgs.assign(os, os + n);
    for (int k = 0; k < n; ++k) eps.insert(eps.end(), {os[k].epsilon, os[k].epsilon / 2.0, os[k].epsilon / 3.0});
  }
  const size_t n9 = 9 * (size_t)h->ndec;
  const size_t b_state = sizeof(long long) * 4 * n9 * n, b_counts = sizeof(unsigned long long) * 3 * n;
  hipError_t e = hipMalloc(&h->state, b_state);
  if (e == hipSuccess) e = hipMalloc(&h->tabs, sizeof(double) * 2 * n9 * n);
  if (e == hipSuccess) e = hipMalloc(&h->counts, b_counts);
  if (e == hipSuccess) e = hipMalloc(&h->dev_cfg, sizeof(nfsp_mccfr_cfg) * n);
  if (e == hipSuccess && os) e = hipMalloc(&h->dev_eps, sizeof(double) * eps.size());
  if (vr) {
    for (float p : H->pay) h->maxpay = std::max(h->maxpay, (double)(p < 0 ? -p : p));
    if (e == hipSuccess) e = hipMalloc(&h->bstate, b_state);
    if (e == hipSuccess) e = hipMalloc(&h->btab, sizeof(double) * n9 * n);
    if (e == hipSuccess) e = hipMemsetAsync(h->bstate, 0, b_state, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->btab, 0, sizeof(double) * n9 * n, ctx->stream);   // B = 0.0
  }
  std::vector<int32_t> rule;
  if (x) {
    h->x_cfgs.assign(x, x + n);
    for (int k = 0; k < n; ++k) rule.insert(rule.end(), {x[k].regret, x[k].average});
    if (e == hipSuccess) e = hipMalloc(&h->dev_rule, sizeof(int32_t) * rule.size());
    if (e == hipSuccess) e = hipMalloc(&h->sw, sizeof(double) * n9 * n);
    if (e == hipSuccess) e = hipMalloc(&h->avg2, sizeof(double) * n9 * n);
    if (e == hipSuccess) e = hipMemsetAsync(h->sw, 0, sizeof(double) * n9 * n, ctx->stream);   // Sw = 0.0
    if (e == hipSuccess)
      e = hipMemcpyAsync(h->dev_rule, rule.data(), sizeof(int32_t) * rule.size(), hipMemcpyHostToDevice, ctx->stream);
  }
  std::vector<NetDevCfg> ncfg;
  if (net) {
    h->net_cfgs.assign(net, net + n);
    h->net_nrows[0] = nrows[0];
    h->net_nrows[1] = nrows[1];
    h->net_hidden = hidden;
    for (int k = 0; k < n; ++k)
      ncfg.push_back(NetDevCfg{net[k].target, net[k].fit_steps, net[k].loss, net[k].lr, net[k].momentum});
    const size_t b_net = sizeof(float) * 2 * nfsp::fit::fit_np(hidden) * n;
    if (e == hipSuccess) e = hipMalloc(&h->dev_net, sizeof(NetDevCfg) * n);
    if (e == hipSuccess) e = hipMalloc(&h->net_rows, sizeof(int32_t) * rows.size());
    if (e == hipSuccess) e = hipMalloc(&h->net_w, b_net);
    if (e == hipSuccess) e = hipMalloc(&h->net_v, b_net);
    if (e == hipSuccess) e = hipMalloc(&h->net_z, sizeof(float) * n9 * n);
    if (e == hipSuccess) e = hipMalloc(&h->sigma_tab, sizeof(double) * n9 * n);
    if (e == hipSuccess) e = hipMalloc(&h->net_loss, sizeof(double) * 4 * n);
    if (e == hipSuccess)
      e = hipMemcpyAsync(h->dev_net, ncfg.data(), sizeof(NetDevCfg) * n, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(h->net_rows, rows.data(), sizeof(int32_t) * rows.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->net_w, w0.data(), b_net, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->net_v, 0, b_net, ctx->stream);                    // v = 0.0
    if (e == hipSuccess) e = hipMemsetAsync(h->net_z, 0, sizeof(float) * n9 * n, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->net_loss, 0, sizeof(double) * 4 * n, ctx->stream);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)net_apply_kernel(hidden), hipFuncAttributeMaxDynamicSharedMemorySize,
                              EX_MAX_LDS);
  }
  if (e == hipSuccess) e = hipMemsetAsync(h->state, 0, b_state, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->counts, 0, b_counts, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h->dev_cfg, h->cfgs.data(), sizeof(nfsp_mccfr_cfg) * n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && os)
    e = hipMemcpyAsync(h->dev_eps, eps.data(), sizeof(double) * eps.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) {
    (void)nfsp_mccfr_destroy(h);
    return nfsp::hip_fail(e, "nfsp_mccfr_create");
  }
  // sigma and the average before any iteration: uniform; with nets sigma is theirs, after both
  // seats' K steps toward R = 0
  rc = x ? launch_x_apply(h, *T, 0, 0) : launch_apply(h, *T, 0);
  if (rc == NFSP_OK && net) rc = launch_net_apply(h, *T, 2, 0);
  if (rc == NFSP_OK && (e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
    rc = nfsp::hip_fail(e, "nfsp_mccfr_create");
  if (rc != NFSP_OK) {
    (void)nfsp_mccfr_destroy(h);
    return rc;
  }
  *out = h;
  return NFSP_OK;
}

}  // namespace

// Checks that need no handle or device come first, so that every rule answers without a GPU.
extern "C" int nfsp_mccfr_create(nfsp_ctx* ctx, const nfsp_mccfr_cfg* cfgs, int n, nfsp_mccfr** out) {
  NFSP_REQUIRE(cfgs && out, "null argument");
  NFSP_REQUIRE(n >= 1 && n <= NFSP_MCCFR_MAX_RUNS, "n must be in 1 .. NFSP_MCCFR_MAX_RUNS");
  NFSP_REQUIRE(ctx, "null argument");
  const int rc = nfsp_mccfr_cfgs_check(ctx->game, cfgs, n, 0);
  if (rc != NFSP_OK) return rc;
  return create_handle(ctx, cfgs, nullptr, n, out);
}

extern "C" int nfsp_mccfr_os_create(nfsp_ctx* ctx, const nfsp_mccfr_os_cfg* cfgs, int n, nfsp_mccfr** out) {
  NFSP_REQUIRE(cfgs && out, "null argument");
  NFSP_REQUIRE(n >= 1 && n <= NFSP_MCCFR_MAX_RUNS, "n must be in 1 .. NFSP_MCCFR_MAX_RUNS");
  NFSP_REQUIRE(ctx, "null argument");
  const int rc = nfsp_mccfr_os_cfgs_check(ctx->game, cfgs, n, 0);
  if (rc != NFSP_OK) return rc;
  std::vector<nfsp_mccfr_cfg> plain(n);
  for (int k = 0; k < n; ++k) plain[k] = nfsp_mccfr_cfg{cfgs[k].seed, cfgs[k].walkers, 0};
  return create_handle(ctx, plain.data(), cfgs, n, out);
}

extern "C" int nfsp_mccfr_vr_create(nfsp_ctx* ctx, const nfsp_mccfr_vr_cfg* cfgs, int n, nfsp_mccfr** out) {
  NFSP_REQUIRE(cfgs && out, "null argument");
  NFSP_REQUIRE(n >= 1 && n <= NFSP_MCCFR_MAX_RUNS, "n must be in 1 .. NFSP_MCCFR_MAX_RUNS");
  NFSP_REQUIRE(ctx, "null argument");
  int rc = nfsp_mccfr_vr_cfgs_check(ctx->game, cfgs, n, 0);
  if (rc != NFSP_OK) return rc;
  std::vector<nfsp_mccfr_cfg> plain(n);
  std::vector<nfsp_mccfr_os_cfg> os(n);
  for (int k = 0; k < n; ++k) {
    plain[k] = nfsp_mccfr_cfg{cfgs[k].seed, cfgs[k].walkers, 0};
    os[k] = nfsp_mccfr_os_cfg{cfgs[k].seed, cfgs[k].walkers, 0, cfgs[k].epsilon};
  }
  rc = create_handle(ctx, plain.data(), os.data(), n, out, 2);
  if (rc == NFSP_OK) (*out)->vr_cfgs.assign(cfgs, cfgs + n);
  return rc;
}

extern "C" int nfsp_mccfr_x_create(nfsp_ctx* ctx, const nfsp_mccfr_x_cfg* cfgs, int n, nfsp_mccfr** out) {
  NFSP_REQUIRE(cfgs && out, "null argument");
  NFSP_REQUIRE(n >= 1 && n <= NFSP_MCCFR_MAX_RUNS, "n must be in 1 .. NFSP_MCCFR_MAX_RUNS");
  NFSP_REQUIRE(ctx, "null argument");
  int rc = nfsp_mccfr_x_cfgs_check(ctx->game, cfgs, n, 0);
  if (rc != NFSP_OK) return rc;
  const int sampling = cfgs[0].sampling;
  std::vector<nfsp_mccfr_cfg> plain(n);
  std::vector<nfsp_mccfr_os_cfg> os(n);
  std::vector<nfsp_mccfr_vr_cfg> vr(n);
  for (int k = 0; k < n; ++k) {
    plain[k] = nfsp_mccfr_cfg{cfgs[k].seed, cfgs[k].walkers, 0};
    os[k] = nfsp_mccfr_os_cfg{cfgs[k].seed, cfgs[k].walkers, 0, cfgs[k].epsilon};
    vr[k] = nfsp_mccfr_vr_cfg{cfgs[k].seed, cfgs[k].walkers, 0, cfgs[k].epsilon};
  }
  rc = create_handle(ctx, plain.data(), sampling ? os.data() : nullptr, n, out, sampling, cfgs);
  if (rc == NFSP_OK && sampling == 2) (*out)->vr_cfgs = vr;
  return rc;
}

extern "C" int nfsp_mccfr_net_create(nfsp_ctx* ctx, const nfsp_mccfr_net_cfg* cfgs, int n, const float* const* dev_w0,
                                     nfsp_mccfr** out) {
  return nfsp_mccfr_net_create_h(ctx, nfsp::nn::H, cfgs, n, dev_w0, out);
}

extern "C" int nfsp_mccfr_net_create_h(nfsp_ctx* ctx, int hidden, const nfsp_mccfr_net_cfg* cfgs, int n,
                                       const float* const* dev_w0, nfsp_mccfr** out) {
  NFSP_REQUIRE(cfgs && out && dev_w0, "null argument");
  NFSP_REQUIRE(n >= 1 && n <= NFSP_MCCFR_MAX_RUNS, "n must be in 1 .. NFSP_MCCFR_MAX_RUNS");
  NFSP_REQUIRE(ctx, "null argument");
  int rc = nfsp_mccfr_net_cfgs_check(ctx->game, cfgs, n, 0);
  if (rc != NFSP_OK) return rc;
  rc = nfsp_fit_width_check(ctx->game, hidden, nullptr);
  if (rc != NFSP_OK) return rc;
  for (int k = 0; k < 2 * n; ++k) NFSP_REQUIRE(dev_w0[k], "nfsp_mccfr_net_create: a null initial net");
  const int sampling = cfgs[0].sampling;
  std::vector<nfsp_mccfr_cfg> plain(n);
  std::vector<nfsp_mccfr_os_cfg> os(n);
  std::vector<nfsp_mccfr_vr_cfg> vr(n);
  std::vector<nfsp_mccfr_x_cfg> x(n);
  for (int k = 0; k < n; ++k) {
    plain[k] = nfsp_mccfr_cfg{cfgs[k].seed, cfgs[k].walkers, 0};
    os[k] = nfsp_mccfr_os_cfg{cfgs[k].seed, cfgs[k].walkers, 0, cfgs[k].epsilon};
    vr[k] = nfsp_mccfr_vr_cfg{cfgs[k].seed, cfgs[k].walkers, 0, cfgs[k].epsilon};
    x[k] = nfsp_mccfr_x_cfg{cfgs[k].seed, cfgs[k].walkers, sampling, cfgs[k].epsilon, cfgs[k].regret, cfgs[k].average};
  }
  rc = create_handle(ctx, plain.data(), sampling ? os.data() : nullptr, n, out, sampling, x.data(), cfgs, dev_w0, hidden);
  if (rc == NFSP_OK && sampling == 2) (*out)->vr_cfgs = vr;
  return rc;
}

#define NFSP_NET_HANDLE(h) \
  NFSP_REQUIRE(!(h)->net_cfgs.empty(), "not a handle of nfsp_mccfr_net_create: the other kinds hold no nets")

extern "C" int nfsp_mccfr_net_tables(nfsp_mccfr* h, int run, const double** dev_sigma, const double** dev_sigma_tab,
                                     const float** dev_z) {
  NFSP_REQUIRE(run >= 0, "run out of range");
  NFSP_REQUIRE(h, "null argument");
  NFSP_NET_HANDLE(h);
  NFSP_REQUIRE(run < h->n, "run out of range");
  const size_t n9 = 9 * (size_t)h->ndec;
  if (dev_sigma) *dev_sigma = h->tabs + (size_t)run * 2 * n9;
  if (dev_sigma_tab) *dev_sigma_tab = h->sigma_tab + (size_t)run * n9;
  if (dev_z) *dev_z = h->net_z + (size_t)run * n9;
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_net_weights(nfsp_mccfr* h, int run, int seat, float** dev_w, float** dev_v) {
  NFSP_REQUIRE(run >= 0, "run out of range");
  NFSP_REQUIRE(h, "null argument");
  NFSP_NET_HANDLE(h);
  NFSP_REQUIRE(run < h->n, "run out of range");
  NFSP_REQUIRE(seat == 0 || seat == 1, "seat must be 0 or 1");
  const size_t at = ((size_t)run * 2 + seat) * nfsp::fit::fit_np(h->net_hidden);
  if (dev_w) *dev_w = h->net_w + at;
  if (dev_v) *dev_v = h->net_v + at;
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_net_hidden(nfsp_mccfr* h, int* out) {
  NFSP_REQUIRE(h && out, "null argument");
  NFSP_NET_HANDLE(h);
  *out = h->net_hidden;
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_net_loss(nfsp_mccfr* h, int run, double out[2][2]) {
  NFSP_REQUIRE(run >= 0, "run out of range");
  NFSP_REQUIRE(h && out, "null argument");
  NFSP_NET_HANDLE(h);
  NFSP_REQUIRE(run < h->n, "run out of range");
  NFSP_HIP(hipMemcpyAsync(out, h->net_loss + 4 * (size_t)run, sizeof(double) * 4, hipMemcpyDeviceToHost,
                          h->ctx->stream));
  NFSP_HIP(hipStreamSynchronize(h->ctx->stream));
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_rule(nfsp_mccfr* h, int run, int32_t out[2]) {
  NFSP_REQUIRE(run >= 0, "run out of range");
  NFSP_REQUIRE(h && out, "null argument");
  NFSP_REQUIRE(run < h->n, "run out of range");
  const bool x = !h->x_cfgs.empty();
  out[0] = x ? h->x_cfgs[run].regret : NFSP_MCCFR_REGRET_PLAIN;
  out[1] = x ? h->x_cfgs[run].average : NFSP_MCCFR_AVG_UNIFORM;
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_average_of(nfsp_mccfr* h, int run, int average, const double** dev_table) {
  NFSP_REQUIRE(run >= 0, "run out of range");
  NFSP_REQUIRE(h && dev_table, "null argument");
  NFSP_REQUIRE(!h->x_cfgs.empty(), "not a handle of nfsp_mccfr_x_create: the other kinds keep no linear sum Sw");
  NFSP_REQUIRE(run < h->n, "run out of range");
  NFSP_REQUIRE(average == NFSP_MCCFR_AVG_UNIFORM || average == NFSP_MCCFR_AVG_LINEAR,
               "average must be NFSP_MCCFR_AVG_UNIFORM or NFSP_MCCFR_AVG_LINEAR");
  const size_t n9 = 9 * (size_t)h->ndec;
  *dev_table = average == h->x_cfgs[run].average ? h->tabs + ((size_t)run * 2 + 1) * n9 : h->avg2 + (size_t)run * n9;
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_weighted(nfsp_mccfr* h, int run, double* host_Sw) {
  NFSP_REQUIRE(run >= 0, "run out of range");
  NFSP_REQUIRE(h && host_Sw, "null argument");
  NFSP_REQUIRE(!h->x_cfgs.empty(), "not a handle of nfsp_mccfr_x_create: the other kinds keep no linear sum Sw");
  NFSP_REQUIRE(run < h->n, "run out of range");
  const size_t n9 = 9 * (size_t)h->ndec;
  NFSP_HIP(hipMemcpyAsync(host_Sw, h->sw + (size_t)run * n9, sizeof(double) * n9, hipMemcpyDeviceToHost,
                          h->ctx->stream));
  NFSP_HIP(hipStreamSynchronize(h->ctx->stream));
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_sampling(nfsp_mccfr* h, int* out) {
  NFSP_REQUIRE(h && out, "null argument");
  *out = h->sampling;
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_run(nfsp_mccfr* h, int64_t iters) {
  NFSP_REQUIRE(iters >= 0, "iters must be >= 0");
  NFSP_REQUIRE(h, "null argument");
  NFSP_REQUIRE(iters <= INT64_MAX - h->iterations, "overflow: iters too large");
  NFSP_REQUIRE(!h->timing || iters <= NFSP_MCCFR_TIMED_ITERS, "with timing on, iters must be <= NFSP_MCCFR_TIMED_ITERS");
  int rc = h->sampling == 2   ? nfsp_mccfr_vr_cfgs_check(h->ctx->game, h->vr_cfgs.data(), h->n, h->iterations + iters)
           : h->sampling == 1 ? nfsp_mccfr_os_cfgs_check(h->ctx->game, h->os_cfgs.data(), h->n, h->iterations + iters)
                              : nfsp_mccfr_cfgs_check(h->ctx->game, h->cfgs.data(), h->n, h->iterations + iters);
  if (rc != NFSP_OK) return rc;
  const ExTables* T = nullptr;
  rc = device_tables(h->ctx, &T);
  if (rc != NFSP_OK) return rc;
  const dim3 grid(nfsp_blocks(h->max_walkers, NFSP_MCCFR_WG_WALKERS), h->n);
  const size_t lds = h->sampling == 2   ? vr_lds(T->nn, T->ndec)
                     : h->sampling == 1 ? os_lds(T->nn, T->ndec)
                                        : walk_lds(T->nn, T->ndec, h->nterm);
  // with timing on: three events per half-iteration, before the walk, after it and after the applies
  std::vector<hipEvent_t> ev;
  struct EvFree {
    std::vector<hipEvent_t>& v;
    ~EvFree() {
      for (hipEvent_t e : v) (void)hipEventDestroy(e);
    }
  } ev_free{ev};
  const auto stamp = [&]() -> int {
    if (!h->timing) return NFSP_OK;
    hipEvent_t e;
    NFSP_HIP(hipEventCreate(&e));
    ev.push_back(e);
    NFSP_HIP(hipEventRecord(e, h->ctx->stream));
    return NFSP_OK;
  };
  for (int64_t it = 0; it < iters; ++it) {
    for (int i = 0; i < 2; ++i) {
      const uint64_t hh = 2 * (uint64_t)h->iterations + i;
      if ((rc = stamp()) != NFSP_OK) return rc;
      if (h->sampling == 2) {
        VrArgs A{};
        A.T = *T;
        A.cfg = h->dev_cfg;
        A.eps = h->dev_eps;
        A.tabs = h->tabs;
        A.btab = h->btab;
        A.state = h->state;
        A.bstate = h->bstate;
        A.counts = h->counts;
        A.h_lo = (uint32_t)hh;
        A.h_hi = (uint32_t)(hh >> 32);
        A.seat = i;
        k_mccfr_vr_walk<<<grid, WALK_THREADS, lds, h->ctx->stream>>>(A);
        NFSP_LAUNCHED("k_mccfr_vr_walk");
      } else if (h->sampling == 1) {
        OsArgs A{};
        A.T = *T;
        A.cfg = h->dev_cfg;
        A.eps = h->dev_eps;
        A.tabs = h->tabs;
        A.state = h->state;
        A.counts = h->counts;
        A.h_lo = (uint32_t)hh;
        A.h_hi = (uint32_t)(hh >> 32);
        A.seat = i;
        k_mccfr_os_walk<<<grid, WALK_THREADS, lds, h->ctx->stream>>>(A);
        NFSP_LAUNCHED("k_mccfr_os_walk");
      } else {
        WalkArgs A{};
        A.T = *T;
        A.cfg = h->dev_cfg;
        A.tabs = h->tabs;
        A.state = h->state;
        A.counts = h->counts;
        A.h_lo = (uint32_t)hh;
        A.h_hi = (uint32_t)(hh >> 32);
        A.seat = i;
        A.nterm = h->nterm;
        k_mccfr_walk<<<grid, WALK_THREADS, lds, h->ctx->stream>>>(A);
        NFSP_LAUNCHED("k_mccfr_walk");
      }
      if ((rc = stamp()) != NFSP_OK) return rc;
      if (!h->x_cfgs.empty()) {
        rc = launch_x_apply(h, *T, 1, h->iterations);
        if (rc == NFSP_OK && !h->net_cfgs.empty()) rc = launch_net_apply(h, *T, i, h->iterations);
      } else {
        rc = launch_apply(h, *T, 1);
        if (rc == NFSP_OK && h->sampling == 2) rc = launch_vr_apply(h);
      }
      if (rc != NFSP_OK) return rc;
      if ((rc = stamp()) != NFSP_OK) return rc;
    }
    h->iterations += 1;
  }
  NFSP_HIP(hipStreamSynchronize(h->ctx->stream));
  for (size_t k = 0; k + 2 < ev.size(); k += 3) {
    float walk = 0.f, apply = 0.f;
    NFSP_HIP(hipEventElapsedTime(&walk, ev[k], ev[k + 1]));
    NFSP_HIP(hipEventElapsedTime(&apply, ev[k + 1], ev[k + 2]));
    h->ms_walk += (double)walk;
    h->ms_apply += (double)apply;
  }
  if (h->timing) h->timed += iters;
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_set_timing(nfsp_mccfr* h, int enable) {
  NFSP_REQUIRE(h, "null argument");
  h->timing = enable != 0;
  h->ms_walk = h->ms_apply = 0.0;
  h->timed = 0;
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_get_timings(nfsp_mccfr* h, double out_ms[2], int64_t* iterations) {
  NFSP_REQUIRE(h && out_ms && iterations, "null argument");
  out_ms[0] = h->ms_walk;
  out_ms[1] = h->ms_apply;
  *iterations = h->timed;
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_iterations(nfsp_mccfr* h, int64_t* out) {
  NFSP_REQUIRE(h && out, "null argument");
  *out = h->iterations;
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_counts(nfsp_mccfr* h, int run, int64_t* out) {
  NFSP_REQUIRE(run >= 0, "run out of range");
  NFSP_REQUIRE(h && out, "null argument");
  NFSP_REQUIRE(run < h->n, "run out of range");
  NFSP_HIP(hipMemcpyAsync(out, h->counts + 3 * (size_t)run, 2 * sizeof(int64_t), hipMemcpyDeviceToHost,
                          h->ctx->stream));
  NFSP_HIP(hipStreamSynchronize(h->ctx->stream));
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_average(nfsp_mccfr* h, int run, const double** dev_table) {
  NFSP_REQUIRE(run >= 0, "run out of range");
  NFSP_REQUIRE(h && dev_table, "null argument");
  NFSP_REQUIRE(run < h->n, "run out of range");
  *dev_table = h->tabs + ((size_t)run * 2 + 1) * 9 * (size_t)h->ndec;
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_state(nfsp_mccfr* h, int run, int64_t* host_R, int64_t* host_S) {
  NFSP_REQUIRE(run >= 0, "run out of range");
  NFSP_REQUIRE(h && host_R && host_S, "null argument");
  NFSP_REQUIRE(run < h->n, "run out of range");
  const size_t n9 = 9 * (size_t)h->ndec;
  const long long* s = h->state + (size_t)run * 4 * n9;
  NFSP_HIP(hipMemcpyAsync(host_R, s, sizeof(int64_t) * n9, hipMemcpyDeviceToHost, h->ctx->stream));
  NFSP_HIP(hipMemcpyAsync(host_S, s + n9, sizeof(int64_t) * n9, hipMemcpyDeviceToHost, h->ctx->stream));
  NFSP_HIP(hipStreamSynchronize(h->ctx->stream));
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_baseline(nfsp_mccfr* h, int run, int64_t* host_Bs, int64_t* host_Bn) {
  NFSP_REQUIRE(run >= 0, "run out of range");
  NFSP_REQUIRE(h && host_Bs && host_Bn, "null argument");
  NFSP_REQUIRE(h->sampling == 2, "not a baseline-corrected handle (nfsp_mccfr_vr_create)");
  NFSP_REQUIRE(run < h->n, "run out of range");
  const size_t n9 = 9 * (size_t)h->ndec;
  const long long* s = h->bstate + (size_t)run * 4 * n9;
  NFSP_HIP(hipMemcpyAsync(host_Bs, s, sizeof(int64_t) * n9, hipMemcpyDeviceToHost, h->ctx->stream));
  NFSP_HIP(hipMemcpyAsync(host_Bn, s + n9, sizeof(int64_t) * n9, hipMemcpyDeviceToHost, h->ctx->stream));
  NFSP_HIP(hipStreamSynchronize(h->ctx->stream));
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_set_baseline(nfsp_mccfr* h, int run, const int64_t* host_Bs, const int64_t* host_Bn) {
  NFSP_REQUIRE(run >= 0, "run out of range");
  NFSP_REQUIRE(h && host_Bs && host_Bn, "null argument");
  NFSP_REQUIRE(h->sampling == 2, "not a baseline-corrected handle (nfsp_mccfr_vr_create)");
  NFSP_REQUIRE(run < h->n, "run out of range");
  const size_t n9 = 9 * (size_t)h->ndec;
  const int64_t most = (int64_t)1 << 61;  // half of what the run's budget keeps an entry within
  for (size_t k = 0; k < n9; ++k) {
    NFSP_REQUIRE(host_Bn[k] >= 0, "a baseline count is negative");
    NFSP_REQUIRE(host_Bn[k] != 0 || host_Bs[k] == 0, "a baseline sum is not 0 where its count is 0");
    NFSP_REQUIRE(host_Bn[k] <= most && host_Bs[k] <= most && host_Bs[k] >= -most,
                 "a baseline sum or count is beyond 2^61");
  }
  // the deltas are 0 between runs: the apply adds nothing, and writes the B of the new tables
  long long* s = h->bstate + (size_t)run * 4 * n9;
  NFSP_HIP(hipMemcpyAsync(s, host_Bs, sizeof(int64_t) * n9, hipMemcpyHostToDevice, h->ctx->stream));
  NFSP_HIP(hipMemcpyAsync(s + n9, host_Bn, sizeof(int64_t) * n9, hipMemcpyHostToDevice, h->ctx->stream));
  const int rc = launch_vr_apply(h);
  if (rc != NFSP_OK) return rc;
  NFSP_HIP(hipStreamSynchronize(h->ctx->stream));
  return NFSP_OK;
}

extern "C" int nfsp_mccfr_destroy(nfsp_mccfr* h) {
  NFSP_REQUIRE(h, "null argument");
  if (h->state) (void)hipFree(h->state);
  if (h->tabs) (void)hipFree(h->tabs);
  if (h->counts) (void)hipFree(h->counts);
  if (h->dev_cfg) (void)hipFree(h->dev_cfg);
  if (h->dev_eps) (void)hipFree(h->dev_eps);
  if (h->bstate) (void)hipFree(h->bstate);
  if (h->btab) (void)hipFree(h->btab);
  if (h->dev_rule) (void)hipFree(h->dev_rule);
  if (h->sw) (void)hipFree(h->sw);
  if (h->avg2) (void)hipFree(h->avg2);
  if (h->dev_net) (void)hipFree(h->dev_net);
  if (h->net_rows) (void)hipFree(h->net_rows);
  if (h->net_w) (void)hipFree(h->net_w);
  if (h->net_v) (void)hipFree(h->net_v);
  if (h->net_z) (void)hipFree(h->net_z);
  if (h->sigma_tab) (void)hipFree(h->sigma_tab);
  if (h->net_loss) (void)hipFree(h->net_loss);
  delete h;
  return NFSP_OK;
}

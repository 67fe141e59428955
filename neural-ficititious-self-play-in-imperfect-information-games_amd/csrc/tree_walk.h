// The walk of the evaluator's public tree (exploit_tree.h), as the four kernels that do it share
// it: k_evaluate and k_best_response (evaluate.hip), k_cfr_plus (cfr.hip), k_xfp (xfp.hip).  Each
// sweeps the tree a depth level at a time, a barrier per level:
//   * top-down, the reach of an item (node, responding seat i, its rank ri, the opponent's rank
//     ro): chance x the opponent's policy (reach_step).  k_cfr_plus carries seat i's own reach
//     beside it and keeps the two in one chain of branches of its own: apart, each walks the
//     parent's fields, one dependent LDS read after another, and its iteration measured 12% slower;
//   * bottom-up, the value per (node, seat i, ri): a terminal sums reach x payoff over the
//     opponent's rank; seat i's decision takes the max over its actions (its information set is
//     its rank + the public history) or its strategy's expectation; every other node sums.
// All in double, no FMA contraction, the sums in the order of the recursive definition (actions,
// public ranks, opponent ranks ascending): the kernels agree with each other, and with the numpy
// restatements in tests/, to the bit.  `#pragma clang fp contract(off)` is scoped to the body it
// stands in, so every helper carries its own.
//
// Device inlines only.  The loops that hand items to threads, the arrays' layouts and the
// barriers stay in the kernels; an array is passed as `item`, the slot of this (seat, ranks) in
// node 0, with the per-node stride.  `nodes` is the node table wherever the kernel keeps it
// (T.nodes, or a copy in LDS).
#pragma once
#include "exploit_tree.h"

namespace nfsp {
namespace ex {

__device__ inline double sum3(const double* v) {
#pragma clang fp contract(off)
  return (v[0] + v[1]) + v[2];
}

// The reach of (N, seat i, ri, ro) from its parent's: the deal at a root; x p_public below chance;
// x pol[row][ro][via] below the opponent's decision; below seat i's own decision unchanged (the
// counterfactual reach a best response or a regret is taken against) or, with own_too,
// x pol[row][ri][via] (the on-policy value).  pol: [ndec][3 ranks][3].
__device__ inline double reach_step(const ExTables& T, const DevNode* nodes, const DevNode& N, int i, int ri, int ro,
                                    const double* pol, const double* item, int stride, bool own_too) {
#pragma clang fp contract(off)
  if (N.parent < 0) return T.deal[ri][ro];
  const DevNode& P = nodes[N.parent];
  const double r0 = item[(size_t)N.parent * stride];
  if (P.kind == TNode::CHANCE) return r0 * p_public(N.via, ri, ro);
  if (P.p == i) return own_too ? r0 * pol[(size_t)P.row * 9 + ri * 3 + N.via] : r0;
  return r0 * pol[(size_t)P.row * 9 + ro * 3 + N.via];
}

// Seat i's value at terminal N with rank ri; reach: [3 ranks of the opponent].
__device__ inline double terminal_value(const ExTables& T, const DevNode& N, int i, int ri, const double* reach) {
#pragma clang fp contract(off)
  const float* py = T.pay + (size_t)N.row * 18 + i * 9 + ri * 3;
  double v = 0.0;
  for (int ro = 0; ro < 3; ++ro) v = v + reach[ro] * (double)py[ro];
  return v;
}

__device__ inline double sum_children(const DevNode& N, const double* item, int stride) {
#pragma clang fp contract(off)
  double v = 0.0;
  for (int a = 0; a < 3; ++a)
    if (N.child[a] >= 0) v = v + item[(size_t)N.child[a] * stride];
  return v;
}

// The expectation under the strategy row s[3].
__device__ inline double weighted_children(const DevNode& N, const double* item, int stride, const double* s) {
#pragma clang fp contract(off)
  double v = 0.0;
  for (int a = 0; a < 3; ++a)
    if (N.child[a] >= 0) v = v + s[a] * item[(size_t)N.child[a] * stride];
  return v;
}

// The best response at a decision: the first maximum among the legal children (a later action
// wins only if strictly greater) and its action.
__device__ inline double first_max_child(const DevNode& N, const double* item, int stride, int& best) {
  double v = 0.0;
  best = -1;
  for (int a = 0; a < 3; ++a) {
    if (N.child[a] < 0) continue;
    const double c = item[(size_t)N.child[a] * stride];
    if (best < 0 || c > v) {
      v = c;
      best = a;
    }
  }
  return v;
}

// A seat's value of the game from its values at the two dealers' roots.
__device__ inline double root_value(const ExTables& T, const double* item, int stride) {
#pragma clang fp contract(off)
  return 0.5 * sum3(item + (size_t)T.root[0] * stride) + 0.5 * sum3(item + (size_t)T.root[1] * stride);
}

// Uniform over the legal actions.
__device__ inline void uniform_row(bool legal_raise, double* out) {
#pragma clang fp contract(off)
  const double u = 1.0 / (legal_raise ? 3.0 : 2.0);
  out[0] = u;
  out[1] = u;
  out[2] = legal_raise ? u : 0.0;
}

// The non-negative row S normalised; uniform where its sum is 0.  An illegal raise gets 0.
__device__ inline void average_row(const double* S, bool legal_raise, double* out) {
#pragma clang fp contract(off)
  const double sum = sum3(S);
  if (sum > 0.0) {
    out[0] = S[0] / sum;
    out[1] = S[1] / sum;
    out[2] = legal_raise ? S[2] / sum : 0.0;
  } else {
    uniform_row(legal_raise, out);
  }
}

}  // namespace ex
}  // namespace nfsp

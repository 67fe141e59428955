"""TEST INFRASTRUCTURE ONLY -- numpy restatements over the *exported* tree tables
(``evaluation.GameTree``) of the exact best-response table (csrc/evaluate.hip k_best_response)
and of full-width extensive-form fictitious play (csrc/xfp.hip k_xfp): the same operations in
the same order, the way policy_ref.CfrRef restates k_cfr_plus.
"""
import numpy as np

import policy_ref as pr

DECISION, CHANCE, TERMINAL = pr.DECISION, pr.CHANCE, pr.TERMINAL
WEIGHT_UNIFORM, WEIGHT_LINEAR = 0, 1


def first_max(vals):
    """[(action, [3] values)] of the legal children in ascending action order -> (best value,
    best action) per rank: a later action wins only where it is strictly greater."""
    a0, v = vals[0]
    v = v.copy()
    best = np.full(3, a0, int)
    for a, c in vals[1:]:
        gt = c > v
        v = np.where(gt, c, v)
        best = np.where(gt, a, best)
    return v, best


def best_response(tree, table0, table1):
    """k_best_response: (beta [ndec, 3, 3] one-hot, q [ndec, 3, 3], reach [ndec, 3]).  Rows where
    seat i acts hold seat i's best response against the other seat's table."""
    T = pr.NodeTable(tree)
    pol = (tree.remap(table0), tree.remap(table1))
    nn = T.nn
    reach = np.zeros((nn, 2, 3, 3))       # [node][e = responding seat][ri][ro]
    val = np.zeros((nn, 2, 3))
    for n in range(nn):
        par = T.par[n]
        if par < 0:
            reach[n, :] = tree.deal
            continue
        for e in (0, 1):
            r0 = reach[par, e]
            if T.kind[par] == CHANCE:
                r = r0 * pr.P_PUBLIC[T.via[n]]
            elif T.p[par] == e:
                r = r0
            else:
                r = r0 * pol[1 - e][T.row[par]][:, T.via[n]][None, :]
            reach[n, e] = r
    beta = np.zeros((tree.ndec, 3, 3))
    q = np.zeros((tree.ndec, 3, 3))
    rch = np.zeros((tree.ndec, 3))
    for n in range(nn - 1, -1, -1):
        for e in (0, 1):
            if T.kind[n] == TERMINAL:
                rp = reach[n, e] * T.pay[T.row[n], e]
                v = (rp[:, 0] + rp[:, 1]) + rp[:, 2]
            elif T.kind[n] == DECISION and T.p[n] == e:
                v, best = first_max([(a, val[c, e]) for a, c in T.kids[n]])
                row = T.row[n]
                for a, c in T.kids[n]:
                    q[row, :, a] = val[c, e]
                beta[row, np.arange(3), best] = 1.0
                rch[row] = (reach[n, e][:, 0] + reach[n, e][:, 1]) + reach[n, e][:, 2]
            else:
                v = np.zeros(3)
                for _, c in T.kids[n]:
                    v = v + val[c, e]
            val[n, e] = v
    return beta, q, rch


class XfpRef:
    """k_xfp in numpy: one run of full-width fictitious play with simultaneous updates."""

    def __init__(self, tree, eta=0.0, weight=WEIGHT_UNIFORM):
        self.T = pr.NodeTable(tree)
        self.tree = tree
        self.eta = float(eta)
        self.weight = int(weight)
        self.S = np.zeros((tree.ndec, 3, 3))
        self.B = np.zeros((tree.ndec, 3, 3))
        self.W = 0.0
        self.t = 0
        self.gaps = []

    def uniform(self):
        return self.tree.uniform()

    def sigma(self):
        """Step 1: the strategy both seats respond to."""
        if self.W == 0.0:
            return self.uniform()
        if self.eta == 0.0:
            P = self.S
        else:
            P = (1.0 - self.eta) * (self.S / self.W) + self.eta * self.B
        den = (P[..., 0] + P[..., 1]) + P[..., 2]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where((den > 0.0)[..., None], P / den[..., None], self.uniform())

    def run(self, iters):
        T, tree = self.T, self.tree
        nn = T.nn
        cf = np.zeros((nn, 3, 3))
        val = np.zeros((nn, 3))
        for _ in range(iters):
            self.t += 1
            w = 1.0 if self.weight == WEIGHT_UNIFORM else float(self.t)
            sg = self.sigma()
            beta = np.zeros((tree.ndec, 3, 3))
            br = [0.0, 0.0]
            for i in (0, 1):
                for n in range(nn):
                    par = T.par[n]
                    if par < 0:
                        cf[n] = tree.deal
                    elif T.kind[par] == CHANCE:
                        cf[n] = cf[par] * pr.P_PUBLIC[T.via[n]]
                    elif T.p[par] == i:
                        cf[n] = cf[par]
                    else:
                        cf[n] = cf[par] * sg[T.row[par], :, T.via[n]][None, :]
                for n in range(nn - 1, -1, -1):
                    v = np.zeros(3)
                    if T.kind[n] == TERMINAL:
                        rp = cf[n] * T.pay[T.row[n], i]
                        for ro in range(3):
                            v = v + rp[:, ro]
                    elif T.kind[n] == DECISION and T.p[n] == i:
                        v, best = first_max([(a, val[c]) for a, c in T.kids[n]])
                        beta[T.row[n], np.arange(3), best] = 1.0
                    else:
                        for _, c in T.kids[n]:
                            v = v + val[c]
                    val[n] = v
                s = [(val[r][0] + val[r][1]) + val[r][2] for r in T.root]
                br[i] = 0.5 * s[0] + 0.5 * s[1]
            self.gaps.append(br[0] + br[1])
            x = np.ones((nn, 2, 3))                # own reach of beta: [node][seat][its rank]
            for n in range(nn):
                par = T.par[n]
                if par < 0:
                    continue
                x[n] = x[par]
                if T.kind[par] == DECISION:
                    x[n, T.p[par]] = x[par, T.p[par]] * beta[T.row[par], :, T.via[n]]
            for n in range(nn):
                if T.kind[n] == DECISION:
                    self.B[T.row[n]] = x[n, T.p[n]][:, None] * beta[T.row[n]]
            self.S = self.S + w * self.B
            self.W = self.W + w
        return self

    def average(self):
        return pr.average_rows(self.tree, self.S)

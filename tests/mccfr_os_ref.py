"""TEST INFRASTRUCTURE ONLY -- the numpy restatement over the *exported* tree tables
(``evaluation.GameTree``) of outcome-sampling MCCFR (csrc/mccfr.hip k_mccfr_os_walk, k_mccfr_apply),
built on mccfr_ref.py.  The rule (include/nfsp.h, "outcome-sampling MCCFR"):

A run has a seed, W walkers (even) and an exploration rate eps.  R, S, t and Q, step 1 (sigma from
R, frozen for the half-iteration), step 3, the draw u(node), the choice rule, the dealer w & 1 and
the deal at the pseudo-node nn are external sampling's (mccfr_ref.py).  Step 2 for walker w of
half-iteration h = 2 t + i is one path; all f64, the operations in the order written:

  start with q = 1.0
  chance              the child chosen by u(n) over p_public(c, r_0, r_1), c ascending
  the opponent's      winv = Q / q; dS[row][r_o][a] += llrint(sigma_a * winv) for each a; the
                      child chosen by u(n) over sigma[row][r_o]
  seat i's, L legal   xi_a = eps / (double)L + (1.0 - eps) * sigma_a for the legal a, 0 at an illegal
                      raise; a* = choice(xi, u(n)); push the frame (row, a*); q = q * xi_{a*}; go
                      to child a*
  terminal            c = (double)pay[row][i][r_i][r_o] / q and x = 1.0
  the frames, deepest first
                      s = sigma[row][r_i][a*] and g = c * x; for the legal a ascending
                      dR[row][r_i][a] += llrint((g * (1.0 - s)) * Q) if a == a*, else
                      llrint((-(g * s)) * Q); then x = x * s

A walker is on one node per level, so all walkers go down the node table together (depth order:
parents first), each node keeping the walkers that reached it, and come back up it in reverse,
which is deepest first for each of them.  Each walker's arithmetic is the rule's, operation for
operation.
"""
import numpy as np

import mccfr_ref as mr
import policy_ref as pr

DECISION, CHANCE, TERMINAL = mr.DECISION, mr.CHANCE, mr.TERMINAL
Q = mr.Q


def omega(tree, eps):
    """The rule's omega: the largest, over both seats and all root-to-terminal paths, of the product
    of L_k / eps over that seat's decisions on the path (from 1.0, the root's factor first)."""
    T = pr.NodeTable(tree)
    best = 1.0
    for i in (0, 1):
        w = np.ones(T.nn)
        for n in range(T.nn):                                # parents first
            if T.par[n] >= 0:
                w[n] = w[T.par[n]]
            if T.kind[n] == DECISION and T.p[n] == i:
                w[n] = w[n] * (float(len(T.kids[n])) / eps)
            if T.kind[n] == TERMINAL:
                best = max(best, float(w[n]))
    return best


def bound(tree, eps):
    """The most walkers x iterations of a run: floor(2^62 / ((Q max(max|pay|, 1)) omega))."""
    maxpay = max(float(np.abs(tree.pay).max()), 1.0)
    return int(2.0 ** 62 / ((Q * maxpay) * omega(tree, eps)))


class OsRef(mr.MccfrRef):
    """One run.  ``moments`` as MccfrRef's."""

    EPS_MIN = 0.0625                                         # NFSP_MCCFR_OS_EPS_MIN

    def __init__(self, tree, seed, walkers, eps, moments=False):
        super().__init__(tree, seed, walkers, moments)
        self.eps = float(eps)
        assert self.EPS_MIN <= self.eps <= 1.0

    def half(self, i):
        T, W, nn, eps = self.tree, self.W, self.nn, self.eps
        h = 2 * self.t + i
        sg = self.sigma()
        w = np.arange(W)
        k = mr.choose([np.full(W, T.deal[a, b]) for a in range(3) for b in range(3)], mr.draws(self.seed, h, w, nn))
        ri, ro = k // 3, k % 3
        r0, r1 = (ri, ro) if i == 0 else (ro, ri)
        at = [None] * nn                                     # the walkers on each node, and what they chose
        pick = [None] * nn
        for d in (0, 1):
            at[self.root[d]] = w[(w & 1) == d]
        dR = np.zeros_like(self.R)
        dS = np.zeros_like(self.S)
        q = np.ones(W)
        c = np.zeros(W)
        for n in range(nn):                                  # the paths down: parents first
            ix = at[n]
            if ix is None or ix.size == 0:
                continue
            row = self.row[n]
            if self.kind[n] == TERMINAL:
                c[ix] = self.pay[row, i][ri[ix], ro[ix]] / q[ix]
                self.terminals += int(ix.size)
                continue
            own = self.kind[n] == DECISION and self.p[n] == i
            if self.kind[n] == CHANCE:
                ps = [pr.P_PUBLIC[a][r0[ix], r1[ix]] for a in range(3)]
            elif not own:
                ps = [sg[row, ro[ix], a] for a in range(3)]
                winv = Q / q[ix]
                for a in range(3):
                    np.add.at(dS[row, :, a], ro[ix], mr.llrint(ps[a] * winv))
            else:
                L = float(len(self.kids[n]))
                legal = [a for a, _ in self.kids[n]]
                ps = [eps / L + (1.0 - eps) * sg[row, ri[ix], a] if a in legal else np.zeros(ix.size)
                      for a in range(3)]
            pk = mr.choose(ps, mr.draws(self.seed, h, ix, n))
            pick[n] = pk
            if own:
                q[ix] = q[ix] * np.choose(pk, ps)
            for a, ch in self.kids[n]:
                at[ch] = ix[pk == a]
        if self.moments:
            self.m1 = np.zeros((T.ndec, 3, 3))
            self.m2 = np.zeros((T.ndec, 3, 3))
        x = np.ones(W)
        for n in range(nn - 1, -1, -1):                      # the frames back: deepest first
            ix = at[n]
            if ix is None or ix.size == 0 or self.kind[n] != DECISION or self.p[n] != i:
                continue
            row, pk = self.row[n], pick[n]
            s = sg[row, ri[ix], pk]
            g = c[ix] * x[ix]
            hit, miss = mr.llrint((g * (1.0 - s)) * Q), mr.llrint((-(g * s)) * Q)
            for a, _ in self.kids[n]:
                inc = np.where(pk == a, hit, miss)
                np.add.at(dR[row, :, a], ri[ix], inc)
                if self.moments:
                    y = inc.astype(np.float64) / Q
                    np.add.at(self.m1[row, :, a], ri[ix], y)
                    np.add.at(self.m2[row, :, a], ri[ix], y * y)
            x[ix] = x[ix] * s
        self.R += dR
        self.S += dS

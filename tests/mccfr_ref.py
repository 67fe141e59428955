"""TEST INFRASTRUCTURE ONLY -- the numpy restatement over the *exported* tree tables
(``evaluation.GameTree``) of external-sampling MCCFR (csrc/mccfr.hip k_mccfr_walk, k_mccfr_apply),
the way policy_ref.CfrRef restates k_cfr_plus.  The rule (include/nfsp.h, "external-sampling
MCCFR"):

A run has a seed and W walkers (even).  R and S [ndec, 3, 3] are int64 fixed point, Q = 2^24 per
chip (R) or per unit of probability (S); t counts completed iterations; all 0 at the start.
Iteration t + 1 is seat i = 0, then seat 1; the half-iteration index is h = 2 t + i.

1. sigma from R, every row and rank: rp_a = (double)max(R_a, 0), 0 at an illegal raise;
   s = (rp_0 + rp_1) + rp_2; sigma_a = rp_a / s, uniform over the legal actions where s = 0.
   R itself is not floored.  sigma is frozen for the half-iteration and all W walkers share it.
2. Walker w = 0 .. W - 1 has dealer w & 1 and starts at root[dealer].
   u(node) = (x >> 8) 2^-24, x the first word of philox4x32(counter = (h low, h high, w, node),
   key = (seed low, seed high)): a draw belongs to the node, not to the order of the visit.
   A choice among p_0 .. p_k with a draw u is the first j with u < c_j and p_j > 0, c the running
   double sum from 0 in ascending order; the last j with p_j > 0 if there is none.
   The deal is drawn at the pseudo-node nn over deal[a][b] in row-major order: seat i holds rank
   a, the other seat b.  Then Traverse(n):
     terminal            (double)pay[row][i][r_i][r_o]
     chance              the child chosen by u(n) over p_public(c, r_0, r_1), c ascending
     the opponent's      dS[row][r_o][a] += llrint(sigma_a Q) for each a; the child chosen by u(n)
                         over sigma[row][r_o]
     seat i's            v_a = Traverse(child_a), legal a ascending; v = 0, then v = v + sigma_a v_a
                         ascending (no contraction); dR[row][r_i][a] += llrint((v_a - v) Q);
                         returns v
3. R += dR, S += dS.

The walkers are independent and the tables are integer sums, so they are restated here for all
walkers at once: a top-down sweep marks the nodes each walker visits, a bottom-up sweep carries
its values.  Each walker's arithmetic is the rule's, operation for operation.
"""
import numpy as np

import policy_ref as pr

DECISION, CHANCE, TERMINAL = pr.DECISION, pr.CHANCE, pr.TERMINAL
Q = float(1 << 24)
M32 = np.uint64(0xFFFFFFFF)


def philox_x(c0, c1, c2, c3, k0, k1):
    """The first word of Philox4x32-10 (csrc/nfsp_device.h philox4x32); uint64 arrays that hold
    32-bit words, broadcast against each other."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    A, B = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = A * c0, B * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> s32) ^ c3 ^ k1) & M32, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0


def draws(seed, h, w, node):
    """u(node) of walkers ``w`` in half-iteration h."""
    x = philox_x(h & 0xFFFFFFFF, (h >> 32) & 0xFFFFFFFF, w, node, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return (x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def choose(ps, u):
    """The rule's choice among the probabilities ps (a list of [W] arrays) with the draws u."""
    c = np.zeros_like(u)
    pick = np.full(u.shape, -1, int)
    last = np.full(u.shape, -1, int)
    for j, p in enumerate(ps):
        c = c + p
        pos = p > 0.0
        last = np.where(pos, j, last)
        pick = np.where((pick < 0) & pos & (u < c), j, pick)
    return np.where(pick >= 0, pick, last)


def match(tree, R):
    """Step 1: sigma [ndec, 3, 3] from the int64 regrets."""
    rp = np.maximum(R, 0).astype(np.float64)
    rp[~tree.legal, :, 2] = 0.0
    return pr.average_rows(tree, rp)


def llrint(x):
    return np.rint(x).astype(np.int64)


class MccfrRef(pr.NodeTable):
    """One run.  ``moments=True`` keeps, for the last half-iteration, the per-entry sums of the
    increments in chips and of their squares over the walkers (``m1``, ``m2``: [ndec, 3, 3])."""

    def __init__(self, tree, seed, walkers, moments=False):
        super().__init__(tree)
        assert walkers >= 2 and walkers % 2 == 0
        self.seed, self.W = int(seed), int(walkers)
        self.R = np.zeros((tree.ndec, 3, 3), np.int64)
        self.S = np.zeros((tree.ndec, 3, 3), np.int64)
        self.t = 0
        self.terminals = 0
        self.moments = moments
        self.m1 = self.m2 = None

    @property
    def traversals(self):
        return 2 * self.W * self.t

    def sigma(self):
        return match(self.tree, self.R)

    def half(self, i):
        T, W, nn = self.tree, self.W, self.nn
        h = 2 * self.t + i
        sg = self.sigma()
        w = np.arange(W)
        u = draws(self.seed, h, w[:, None], np.arange(nn + 1)[None, :])       # [W, nn + 1]
        k = choose([np.full(W, T.deal[a, b]) for a in range(3) for b in range(3)], u[:, nn])
        ri, ro = k // 3, k % 3
        r0, r1 = (ri, ro) if i == 0 else (ro, ri)
        visit = np.zeros((nn, W), bool)
        pick = np.full((nn, W), -1, int)
        for d in (0, 1):
            visit[self.root[d]] = (w & 1) == d
        dR = np.zeros_like(self.R)
        dS = np.zeros_like(self.S)
        for n in range(nn):                                  # depth order: parents first
            m = visit[n]
            if not m.any() or self.kind[n] == TERMINAL:
                continue
            row = self.row[n]
            if self.kind[n] == DECISION and self.p[n] == i:
                for _, c in self.kids[n]:
                    visit[c] = m
                continue
            if self.kind[n] == CHANCE:
                ps = [pr.P_PUBLIC[c][r0, r1] for c in range(3)]
            else:
                ps = [sg[row, ro, a] for a in range(3)]
                for a in range(3):
                    np.add.at(dS[row, :, a], ro[m], llrint(ps[a][m] * Q))
            pick[n] = choose(ps, u[:, n])
            for a, c in self.kids[n]:
                visit[c] = m & (pick[n] == a)
        val = np.zeros((nn, W))
        if self.moments:
            self.m1 = np.zeros((T.ndec, 3, 3))
            self.m2 = np.zeros((T.ndec, 3, 3))
        for n in range(nn - 1, -1, -1):
            m = visit[n]
            if not m.any():
                continue
            row = self.row[n]
            if self.kind[n] == TERMINAL:
                val[n] = self.pay[row, i][ri, ro]
                self.terminals += int(m.sum())
            elif self.kind[n] == DECISION and self.p[n] == i:
                v = np.zeros(W)
                for a, c in self.kids[n]:
                    v = v + sg[row, ri, a] * val[c]
                for a, c in self.kids[n]:
                    inc = llrint((val[c] - v) * Q)
                    np.add.at(dR[row, :, a], ri[m], inc[m])
                    if self.moments:
                        x = inc[m].astype(np.float64) / Q
                        np.add.at(self.m1[row, :, a], ri[m], x)
                        np.add.at(self.m2[row, :, a], ri[m], x * x)
                val[n] = v
            else:
                v = np.zeros(W)
                for a, c in self.kids[n]:
                    v = np.where(pick[n] == a, val[c], v)
                val[n] = v
        self.R += dR
        self.S += dS

    def run(self, iters):
        for _ in range(iters):
            self.half(0)
            self.half(1)
            self.t += 1
        return self

    def average(self):
        return pr.average_rows(self.tree, self.S.astype(np.float64))


def exact_increments(tree, sigma, i):
    """The exact counterpart of a traversal's regret increments for seat i under ``sigma``:
    [ndec, 3, 3] of val[child] - val[node], the counterfactual values of policy_ref.CfrRef's walk
    (the opponent's and chance's reach from the deal, times seat i's value below).  0 where the
    other seat acts and at an illegal raise."""
    T = pr.NodeTable(tree)
    nn = T.nn
    cf = np.zeros((nn, 3, 3))
    val = np.zeros((nn, 3))
    for n in range(nn):
        par = T.par[n]
        if par < 0:
            cf[n] = tree.deal
        elif T.kind[par] == CHANCE:
            cf[n] = cf[par] * pr.P_PUBLIC[T.via[n]]
        elif T.p[par] == i:
            cf[n] = cf[par]
        else:
            cf[n] = cf[par] * sigma[T.row[par], :, T.via[n]][None, :]
    for n in range(nn - 1, -1, -1):
        v = np.zeros(3)
        if T.kind[n] == TERMINAL:
            rp = cf[n] * T.pay[T.row[n], i]
            for ro in range(3):
                v = v + rp[:, ro]
        elif T.kind[n] == DECISION and T.p[n] == i:
            for a, c in T.kids[n]:
                v = v + sigma[T.row[n], :, a] * val[c]
        else:
            for _, c in T.kids[n]:
                v = v + val[c]
        val[n] = v
    out = np.zeros((tree.ndec, 3, 3))
    for n in range(nn):
        if T.kind[n] == DECISION and T.p[n] == i:
            for a, c in T.kids[n]:
                out[T.row[n], :, a] = val[c] - val[n]
    return out

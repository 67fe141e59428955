"""TEST INFRASTRUCTURE ONLY -- the numpy restatement over the *exported* tree tables
(``evaluation.GameTree``) of baseline-corrected outcome sampling, VR-MCCFR (Schmid et al. 2019;
Davis, Schmid and Bowling 2020; csrc/mccfr.hip k_mccfr_vr_walk, k_mccfr_apply, k_mccfr_vr_apply),
built on mccfr_os_ref.py.  The rule (include/nfsp.h, "baseline-corrected outcome sampling"):

A run has a seed, W walkers (even) and an exploration rate eps, and beside R and S the baseline
sums Bs (int64, Q per chip) and counts Bn (int64), [ndec, 3, 3], all 0 at the start.  The baseline
of a half-iteration is frozen as sigma is: B = clamp((double)Bs / ((double)Bn * Q), -P, P), 0 where
Bn = 0, P = max|pay|; B[row][r][a] is in the perspective of the seat that acts at row, r its rank.
The path of walker w -- the deal, every draw and choice, q, and the dS increments -- is outcome
sampling's (mccfr_os_ref.py), bit for bit.  What changes is the pass back; all f64, the operations
in the order written:

  on the way down     push a frame at every decision, both seats'; at seat i's keep xi_{a*} and qk,
                      q before it is multiplied by xi_{a*}
  terminal            v = (double)pay[row][i][r_i][r_o]
  the frames, deepest first
    the opponent's    b_a = -B[row][r_o][a], 0 at an illegal raise;
                      dBs[row][r_o][a*] += llrint((-v) * Q) and dBn[row][r_o][a*] += 1;
                      v = ((sigma_0 * b_0 + sigma_1 * b_1) + sigma_2 * b_2) + (v - b_{a*})
    seat i's          b_a = B[row][r_i][a];
                      dBs[row][r_i][a*] += llrint(v * Q) and dBn[row][r_i][a*] += 1;
                      u_a = b_a for the legal a != a*, u_{a*} = b_{a*} + (v - b_{a*}) / xi_{a*};
                      vbar = 0, then vbar = vbar + sigma_a * u_a for the legal a ascending;
                      dR[row][r_i][a] += llrint(((u_a - vbar) / qk) * Q) for the legal a; v = vbar
  then R += dR, S += dS, Bs += dBs, Bn += dBn.

As in mccfr_os_ref.py all walkers go down the node table together and come back up it in reverse.
"""
import numpy as np

import mccfr_os_ref as osr
import mccfr_ref as mr
import policy_ref as pr

DECISION, CHANCE, TERMINAL = mr.DECISION, mr.CHANCE, mr.TERMINAL
Q = mr.Q


def maxpay(tree):
    """P: the game's largest |pay|, in chips."""
    return float(np.abs(tree.pay).max())


def baseline_table(tree, Bs, Bn):
    """B [ndec, 3, 3] f64 from the sums and the counts."""
    P = maxpay(tree)
    den = np.where(Bn > 0, Bn, 1).astype(np.float64) * Q
    return np.where(Bn > 0, np.clip(Bs.astype(np.float64) / den, -P, P), 0.0)


def bound_parts(tree, eps):
    """The rule's overflow recursion with |B| <= P: (Rmax, Bmax, omega) in chips / as a factor --
    the most one traversal moves an R entry, a Bs entry, and (x 1) an S entry, over both seats."""
    T = pr.NodeTable(tree)
    P = maxpay(tree)
    rmax = bmax = 0.0
    for i in (0, 1):
        vmax = np.zeros(T.nn)
        for n in range(T.nn - 1, -1, -1):                    # children first
            m = max([vmax[c] for _, c in T.kids[n]], default=0.0)
            if T.kind[n] == TERMINAL:
                vmax[n] = P
            elif T.kind[n] == CHANCE:
                vmax[n] = m
            elif T.p[n] != i:
                vmax[n] = 2.0 * P + m
            else:
                vmax[n] = P + (m + P) * (float(len(T.kids[n])) / eps)
            if T.kind[n] == DECISION:
                bmax = max(bmax, float(m))
        w = np.ones(T.nn)                                    # the product of L_k / eps above n
        for n in range(T.nn):                                # parents first
            par = T.par[n]
            if par >= 0:
                w[n] = w[par]
                if T.kind[par] == DECISION and T.p[par] == i:
                    w[n] = w[par] * (float(len(T.kids[par])) / eps)
            if T.kind[n] == DECISION and T.p[n] == i:
                rmax = max(rmax, float((2.0 * vmax[n]) * w[n]))
    return rmax, bmax, osr.omega(tree, eps)


def bound(tree, eps):
    """The most walkers x iterations of a run: floor(2^62 / (Q max(Rmax, Bmax, omega)))."""
    return int(2.0 ** 62 / (Q * max(bound_parts(tree, eps))))


class VrRef(osr.OsRef):
    """One run.  ``moments`` as MccfrRef's, over seat i's R increments.  ``picks`` holds, after a
    half-iteration, what the walkers on each node chose."""

    def __init__(self, tree, seed, walkers, eps, moments=False):
        super().__init__(tree, seed, walkers, eps, moments)
        self.Bs = np.zeros((tree.ndec, 3, 3), np.int64)
        self.Bn = np.zeros((tree.ndec, 3, 3), np.int64)
        self.picks = None

    def baseline(self):
        return baseline_table(self.tree, self.Bs, self.Bn)

    def half(self, i):
        T, W, nn, eps = self.tree, self.W, self.nn, self.eps
        h = 2 * self.t + i
        sg = self.sigma()
        B = self.baseline()
        w = np.arange(W)
        k = mr.choose([np.full(W, T.deal[a, b]) for a in range(3) for b in range(3)], mr.draws(self.seed, h, w, nn))
        ri, ro = k // 3, k % 3
        r0, r1 = (ri, ro) if i == 0 else (ro, ri)
        at = [None] * nn                                     # the walkers on each node, what they chose,
        pick = [None] * nn                                   # and at seat i's nodes xi_{a*} and qk
        xi = [None] * nn
        qk = [None] * nn
        for d in (0, 1):
            at[self.root[d]] = w[(w & 1) == d]
        dR = np.zeros_like(self.R)
        dS = np.zeros_like(self.S)
        dBs = np.zeros_like(self.Bs)
        dBn = np.zeros_like(self.Bn)
        q = np.ones(W)
        v = np.zeros(W)
        for n in range(nn):                                  # the paths down: outcome sampling's
            ix = at[n]
            if ix is None or ix.size == 0:
                continue
            row = self.row[n]
            if self.kind[n] == TERMINAL:
                v[ix] = self.pay[row, i][ri[ix], ro[ix]]
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
                qk[n] = q[ix].copy()
                xi[n] = np.choose(pk, ps)
                q[ix] = q[ix] * xi[n]
            for a, ch in self.kids[n]:
                at[ch] = ix[pk == a]
        self.picks = pick
        if self.moments:
            self.m1 = np.zeros((T.ndec, 3, 3))
            self.m2 = np.zeros((T.ndec, 3, 3))
        for n in range(nn - 1, -1, -1):                      # the frames back: deepest first
            ix = at[n]
            if ix is None or ix.size == 0 or self.kind[n] != DECISION:
                continue
            row, pk = self.row[n], pick[n]
            legal = [a for a, _ in self.kids[n]]
            vv = v[ix]
            if self.p[n] != i:
                r = ro[ix]
                b = [-B[row, r, a] if a in legal else np.zeros(ix.size) for a in range(3)]
                np.add.at(dBs[row], (r, pk), mr.llrint((-vv) * Q))
                np.add.at(dBn[row], (r, pk), 1)
                s = [sg[row, r, a] for a in range(3)]
                v[ix] = ((s[0] * b[0] + s[1] * b[1]) + s[2] * b[2]) + (vv - np.choose(pk, b))
                continue
            r = ri[ix]
            b = [B[row, r, a] for a in range(3)]
            np.add.at(dBs[row], (r, pk), mr.llrint(vv * Q))
            np.add.at(dBn[row], (r, pk), 1)
            hit = np.choose(pk, b)
            hit = hit + (vv - hit) / xi[n]
            u = {a: np.where(pk == a, hit, b[a]) for a in legal}
            vbar = np.zeros(ix.size)
            for a in legal:
                vbar = vbar + sg[row, r, a] * u[a]
            for a in legal:
                inc = mr.llrint(((u[a] - vbar) / qk[n]) * Q)
                np.add.at(dR[row, :, a], r, inc)
                if self.moments:
                    y = inc.astype(np.float64) / Q
                    np.add.at(self.m1[row, :, a], r, y)
                    np.add.at(self.m2[row, :, a], r, y * y)
            v[ix] = vbar
        self.R += dR
        self.S += dS
        self.Bs += dBs
        self.Bn += dBn

"""TEST INFRASTRUCTURE ONLY -- numpy restatements over the *exported* tree tables
(``evaluation.GameTree``): the evaluator's walk (csrc/evaluate.hip k_evaluate) and CFR+
(csrc/cfr.hip k_cfr_plus), the same operations in the same order, plus the glue that scores a
table with the brute-force oracle (oracle/exploit_oracle.py, which knows nothing of the tree).
"""
import numpy as np

import exploit_oracle as eo

DECISION, CHANCE, TERMINAL = 0, 1, 2
GAME_NAME = {0: "leduc", 1: "kuhn"}
# P(public rank r | ranks ri, ro): [r][ri][ro]
P_PUBLIC = np.array([[[(2.0 - (ri == r) - (ro == r)) / 4.0 for ro in range(3)] for ri in range(3)]
                     for r in range(3)])


def random_table(tree, seed):
    """Dirichlet(1, 1, 1) rows (the raise column is remapped where it is illegal)."""
    rng = np.random.RandomState(seed)
    return tree.remap(rng.dirichlet(np.ones(3), size=(tree.ndec, 3)))


# ---- the walk ---------------------------------------------------------------------------
def walk(tree, table0, table1):
    """What nfsp_evaluate_batch computes for (table at seat 0, table at seat 1)."""
    pol = (tree.remap(table0), tree.remap(table1))
    N = tree.nodes
    nn = tree.nn
    reach = np.zeros((nn, 3, 3, 3))       # [node][evaluation][ri][ro]
    val = np.zeros((nn, 3, 3))
    for n in range(nn):                   # depth order: parents first
        par = int(N["parent"][n])
        if par < 0:
            reach[n, :] = tree.deal
            continue
        via, row, kind, pp = int(N["via"][n]), int(N["row"][par]), int(N["kind"][par]), int(N["p"][par])
        for e in range(3):
            i = 1 if e == 1 else 0
            r0 = reach[par, e]
            if kind == CHANCE:
                r = r0 * P_PUBLIC[via]
            elif pp == i:
                r = r0 if e < 2 else r0 * pol[i][row][:, via][:, None]
            else:
                r = r0 * pol[1 - i][row][:, via][None, :]
            reach[n, e] = r
    for n in range(nn - 1, -1, -1):
        kind, pp, row = int(N["kind"][n]), int(N["p"][n]), int(N["row"][n])
        kids = [int(c) for c in N["child"][n] if c >= 0]
        for e in range(3):
            i = 1 if e == 1 else 0
            if kind == TERMINAL:
                rp = reach[n, e] * tree.pay[row, i].astype(np.float64)
                v = (rp[:, 0] + rp[:, 1]) + rp[:, 2]
            elif kind == DECISION and pp == i and e < 2:
                v = val[kids[0], e]
                for c in kids[1:]:
                    v = np.maximum(v, val[c, e])
            else:
                v = np.zeros(3)
                for c in kids:
                    v = v + val[c, e]
            val[n, e] = v
    per = np.array([[(val[tree.root[d], e, 0] + val[tree.root[d], e, 1]) + val[tree.root[d], e, 2]
                     for d in range(2)] for e in range(3)])
    s = 0.5 * per[:, 0] + 0.5 * per[:, 1]
    return {"br0": s[0], "br1": s[1], "exploitability": s[0] + s[1], "value0": s[2],
            "value0_dealer0": per[2, 0], "value0_dealer1": per[2, 1]}


# ---- the brute-force oracle on a table ------------------------------------------------------
def oracle_policy(tree, table, seat):
    """``table`` played at ``seat`` as an exploit_oracle policy (looked up by observation)."""
    t = np.asarray(table, np.float64).reshape(tree.ndec, 3, 3)
    return eo.TabularPolicy(lambda obs: t[tree.row_of(seat, obs)])


def oracle_scores(tree, p0, p1, keys=("br0", "br1", "value0", "value0_dealer0", "value0_dealer1")):
    """The oracle's numbers for exploit_oracle policies p0 at seat 0 and p1 at seat 1."""
    g = GAME_NAME[tree.game]
    out = {}
    if "br0" in keys:
        out["br0"] = eo.best_response(0, p1, g)
    if "br1" in keys:
        out["br1"] = eo.best_response(1, p0, g)
    if "br0" in out and "br1" in out:
        out["exploitability"] = out["br0"] + out["br1"]
    if "value0" in keys:
        out["value0"] = eo.on_policy_value0(p0, p1, g)
    for d in (0, 1):
        if f"value0_dealer{d}" in keys:
            out[f"value0_dealer{d}"] = eo.on_policy_value0(p0, p1, g, dealers=(d,))
    return out


def oracle_table_scores(tree, table0, table1, **kw):
    return oracle_scores(tree, oracle_policy(tree, table0, 0), oracle_policy(tree, table1, 1), **kw)


# ---- what the solvers' restatements share (xfp_ref.py too) -----------------------------------
class NodeTable:
    """The node table unpacked once (plain ints index faster than numpy scalars)."""

    def __init__(self, tree):
        N = tree.nodes
        self.tree = tree
        self.nn = tree.nn
        self.par = N["parent"].astype(int)
        self.kind = N["kind"].astype(int)
        self.p = N["p"].astype(int)
        self.via = N["via"].astype(int)
        self.row = N["row"].astype(int)
        self.kids = [[(a, int(c)) for a, c in enumerate(N["child"][n]) if c >= 0] for n in range(tree.nn)]
        self.pay = tree.pay.astype(np.float64)
        self.root = [int(r) for r in tree.root]


def average_rows(tree, S):
    """The strategy sums S [ndec, 3, 3] normalised per row; uniform over the legal actions where
    a row's sum is 0: the tail of k_cfr_plus and k_xfp."""
    s = (S[..., 0] + S[..., 1]) + S[..., 2]
    legal = tree.legal[:, None] & np.ones(3, bool)[None, :]
    u = np.where(legal, 1.0 / 3.0, 1.0 / 2.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = np.where((s > 0.0)[..., None], S / s[..., None], u[..., None])
    avg[..., 2] = np.where(legal, avg[..., 2], 0.0)
    return avg


# ---- CFR+ ---------------------------------------------------------------------------------
class CfrRef(NodeTable):
    """k_cfr_plus in numpy: regret-matching+, alternating updates, average weighted by t."""

    def __init__(self, tree):
        super().__init__(tree)
        self.R = np.zeros((tree.ndec, 3, 3))
        self.S = np.zeros((tree.ndec, 3, 3))
        self.t = 0

    def match(self, R, legal):
        """[.., 3] regrets -> strategies; ``legal`` [..]: whether the raise is legal."""
        rp = np.where(R > 0.0, R, 0.0)
        rp[..., 2] = np.where(legal, rp[..., 2], 0.0)
        s = (rp[..., 0] + rp[..., 1]) + rp[..., 2]
        u = np.where(legal, 1.0 / 3.0, 1.0 / 2.0)
        uni = np.stack([u, u, np.where(legal, u, 0.0)], axis=-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where((s > 0.0)[..., None], rp / s[..., None], uni)

    def run(self, iters):
        T = self.tree
        nn = T.nn
        legal = T.legal[:, None] & np.ones(3, bool)[None, :]
        sg = self.match(self.R, legal)
        cf = np.zeros((nn, 3, 3))
        own = np.zeros((nn, 3))
        val = np.zeros((nn, 3))
        for _ in range(iters):
            self.t += 1
            t = float(self.t)
            for i in (0, 1):
                for n in range(nn):
                    par = self.par[n]
                    if par < 0:
                        cf[n] = T.deal
                        own[n] = 1.0
                    elif self.kind[par] == CHANCE:
                        cf[n] = cf[par] * P_PUBLIC[self.via[n]]
                        own[n] = own[par]
                    elif self.p[par] == i:
                        cf[n] = cf[par]
                        own[n] = own[par] * sg[self.row[par], :, self.via[n]]
                    else:
                        cf[n] = cf[par] * sg[self.row[par], :, self.via[n]][None, :]
                        own[n] = own[par]
                for n in range(nn - 1, -1, -1):
                    v = np.zeros(3)
                    if self.kind[n] == TERMINAL:
                        rp = cf[n] * self.pay[self.row[n], i]
                        for ro in range(3):
                            v = v + rp[:, ro]
                    elif self.kind[n] == DECISION and self.p[n] == i:
                        for a, c in self.kids[n]:
                            v = v + sg[self.row[n], :, a] * val[c]
                    else:
                        for _, c in self.kids[n]:
                            v = v + val[c]
                    val[n] = v
                for n in range(nn):
                    if self.kind[n] != DECISION or self.p[n] != i:
                        continue
                    row = self.row[n]
                    w = t * own[n]
                    for a, c in self.kids[n]:
                        r = (self.R[row, :, a] + val[c]) - val[n]
                        self.R[row, :, a] = np.where(r > 0.0, r, 0.0)
                        self.S[row, :, a] = self.S[row, :, a] + w * sg[row, :, a]
                    sg[row] = self.match(self.R[row], legal[row])
        return self

    def average(self):
        return average_rows(self.tree, self.S)

"""TEST INFRASTRUCTURE ONLY -- the exact distribution of one hand of the batched rollout
(``nfsp_rollout``), in float64 numpy, and the statistics that compare a rollout's counts with it.

The oracle replays (oracle/rollout_oracle.py) restate the kernel: they share its Philox counter
layout, its ``below`` / ``u01``, its deal and its dealer rule, so a mistake in any of those is
copied on both sides.  This module shares none of that.  It is built from the exported public
tree (``evaluation.GameTree``: what evaluate.hip, cfr.hip and xfp.hip score) and from
``oracle/nn_oracle.py`` forwards of the six nets, and says with which probability a hand visits
every (information set, action): what the rollout's counts must converge to if the engine
samples the game the evaluators score.  Nothing here comes from the device or from
``rollout_oracle``.

Rules

1. Acting table of seat p: the per-hand mixture of two tables, the BR epsilon-table
   ``(1 - eps_p) * greedy + eps_p * (1/3, 1/3, 1/3)`` and the AR table: one-hot at the argmax
   of the softmax (agent/agent.py:143, newenv.py:135), the softmax itself with
   ``NFSP_EXT_SAMPLE_AR``.  The mixture weights are eta and 1 - eta (one draw per hand and
   agent, main.py:36-45) times ``GameTree.own_reach`` of each table as executed, applied to
   the UN-remapped rows (``evaluation.mix`` returns remapped rows; ``remap`` of this table is
   ``evaluation.mix`` of the two).
2. Reach: the walk of ``policy_ref.walk``'s on-policy evaluation, per dealer: ``tree.deal`` at
   the dealer's root (0.5 x that over both), ``P_PUBLIC`` at chance nodes, the executed
   (remapped) tables at decisions.
3. Before the remap: ``stats()["actions"]`` (agent/agent.py:155) and the stored action rows
   count the argmax BEFORE the env's raise-to-call remap (newenv.py:141-145), and an
   epsilon-random action (agent/agent.py:128) is uniform over three actions even where the
   raise is illegal.
4. No record: a decision leaves no RL record when its action vector is all zero
   (``np.average(a) != 0``, agent/agent.py:132-134): the greedy ReLU head with three
   non-positive outputs.  Such a decision folds (argmax of zeros), and still counts in
   ``actions``.  Which rows those are comes from the ``nn_oracle`` forward (the device's ReLU
   forward is bit-exact with it: test_predict_relu_bit_exact).
5. Alias: with ``NFSP_QUIRK_ALIAS_RL`` the RL rows carry the hand's LAST s and a
   (utils/replay_buffer.py:30-41 + newenv.py:119), so per-information-set RL counts are for
   configs without that bit; with it the number of records, the action counters, the reward
   and the SL records (``pend_x`` holds the observation of every BR-mode decision, random ones
   included) still follow the model.
6. Draws are 24-bit and the comparisons inclusive: the engine draws u in {0, 1, .., 2^24 - 1}
   x 2^-24 and an agent acts with its BR net iff ``not (u > eta)`` (main.py:36-45), at random
   iff ``not (u > eps)`` (agent/agent.py:124-128).  So P(BR mode) = (floor(eta x 2^24) + 1) /
   2^24 (eta as float32, capped at 1) and likewise for eps: eta = 0 is 2^-24, not 0.  With
   262,144 lanes that is 0.06 expected BR-mode seats per rollout, which a model with P = 0
   would report as records in cells of probability 0.

Besides the behavioural tables (rules 1-2: ``p_dec``, ``p_rec``, ``p_sl``, the reward), the model
walks the tree once per pair of modes (BR / AR per seat) carrying the distribution of the per-hand
counters (each action per seat, RL records per seat, SL records per seat).  That gives their
exact means and variances -- a seat makes up to 4 decisions per hand, so those counts are not
binomial -- and, independently of rule 1, the same means as the behavioural tables
(tests/test_rollout_dist.py asserts that they agree).

The bound (a condition, derived and not measured).  A specific (row, rank, action) is visited
at most once per hand, so its count over n hands of the row's dealer is exactly binomial: for an
expectation E in [cut, n - cut], z = (obs - E) / sqrt(E (1 - p)).  Other cells of non-zero
probability are pooled per seat and tested with the conservative variance 4 x E_pool (a seat
makes at most 4 decisions per hand, so a per-hand count Y <= 4 has Var Y <= E Y^2 <= 4 E Y).
Cells of probability exactly 0 must have a count of exactly 0.  A test file asserting K
statistics requires |z| <= z*, with K erfc(z* / sqrt 2) <= 1e-6 (``z_star``).
"""
import math

import numpy as np

import nn_oracle as nn
from policy_ref import CHANCE, P_PUBLIC, TERMINAL

EXT_LINEAR_Q, EXT_SAMPLE_AR = 32, 128                           # include/nfsp.h
DRAW_STEPS = float(1 << 24)
# the per-hand counters of the mode walk, per seat p at index 5 p + ..
ACT0, N_RL, N_SL, NCNT = 0, 3, 4, 5
MAXDEC = 4                                                      # decisions of one seat in a hand


def p_not_above(x) -> float:
    """P(not (u > x)) for the engine's 24-bit uniform u (rule 6)."""
    x = float(x)
    if x < 0.0:
        return 0.0
    return min(1.0, (math.floor(x * DRAW_STEPS) + 1.0) / DRAW_STEPS)


def z_star(k: int, alpha: float = 1e-6) -> float:
    """The smallest z (to 1e-9) with k x erfc(z / sqrt 2) <= alpha: k two-sided normal
    statistics all stay within z with probability >= 1 - alpha."""
    lo, hi = 0.0, 40.0
    while hi - lo > 1e-9:
        mid = 0.5 * (lo + hi)
        if k * math.erfc(mid / math.sqrt(2.0)) <= alpha:
            hi = mid
        else:
            lo = mid
    return hi


def dealer_lanes(lane0: int, n: int, g: int) -> np.ndarray:
    """[2]: how many of the global lanes [lane0, lane0 + n) have dealer 0 / 1 at hand index g
    (the dealer alternates per hand and per lane: include/nfsp.h, nfsp_engine section)."""
    d = (np.arange(lane0, lane0 + n, dtype=np.int64) + int(g)) & 1
    return np.bincount(d, minlength=2).astype(np.int64)


def stats_per_rollout(ndec: int) -> int:
    """An upper bound of the statistics ``check_counts`` asserts for one rollout: every RL cell
    and every SL cell (as a z or as an exact zero), a pool per seat for each, 6 action counters,
    the records per seat of each kind and the reward."""
    return 9 * ndec + 3 * ndec + 4 + 6 + 4 + 1


class Model:
    """The exact per-hand distribution for ``game``'s ``tree`` under the packed ``[2][3][NP]``
    weights ``w_flat``, ``eta``, ``eps = (eps0, eps1)`` and ``quirks``.

    Per dealer d: ``p_dec[d][row, rank, a]`` (the hand visits the decision and the stored
    action vector's argmax is a), ``p_rec[d]`` (.. and leaves an RL record), ``p_sl[d][row,
    rank]`` (.. leaves an SL record), ``reward_mean[d]`` / ``reward_var[d]`` of seat 0,
    ``cnt_mean[d][k]`` / ``cnt_var[d][k]`` of the per-hand counters (5 p + a: actions of seat p,
    5 p + 3: its RL records, 5 p + 4: its SL records).  ``acting_raw`` / ``acting``: the
    behavioural table of rule 1 before / after the remap.

    The keyword arguments build deliberately WRONG models for the tests' teeth: ``rule4=False``
    drops rule 4; against rule 3, ``remap_counters`` counts executed actions in the action
    counters, ``rule3=False`` does that and also takes the stored action rows as remapped, and
    ``remap_random`` puts only the epsilon-random action through the remap before it is
    counted; ``p_public`` replaces the public card's distribution."""

    def __init__(self, tree, w_flat, eta, eps, quirks, rule4=True, rule3=True, remap_counters=False,
                 remap_random=False, p_public=None):
        self.tree = tree
        self.quirks = int(quirks)
        self.p_br = p_not_above(np.float32(eta))                       # cfg.eta is a float
        self.p_rand = np.array([p_not_above(eps[0]), p_not_above(eps[1])])
        self.remap_counters = bool(remap_counters) or not rule3
        self.rule3 = bool(rule3)
        self.p_public = P_PUBLIC if p_public is None else np.asarray(p_public, np.float64)
        nd = tree.ndec
        seat = tree.seat.astype(int)
        self.seat = seat
        self.dealer_of_row = np.array([tree.path(r)[0] for r in range(nd)])
        # ---- the nets at every information set (nn_oracle forwards, float32)
        w = np.asarray(w_flat, np.float32).reshape(2, 3, -1)
        obs = tree.obs.astype(np.int64).reshape(-1)
        x = ((obs[:, None] >> np.arange(30)) & 1).astype(np.float32)
        br_act = nn.ACT_LINEAR if self.quirks & EXT_LINEAR_Q else nn.ACT_RELU
        ar_y = np.zeros((nd, 3, 3))
        br_q = np.zeros((nd, 3, 3))
        for p in (0, 1):
            y = nn.MLP(nn.ACT_SOFTMAX, 64, weights=nn.unpack_weights(w[p, 0])).predict(x).reshape(nd, 3, 3)
            q = nn.MLP(br_act, 64, weights=nn.unpack_weights(w[p, 1])).predict(x).reshape(nd, 3, 3)
            ar_y[seat == p] = y[seat == p]
            br_q[seat == p] = q[seat == p]
        eye = np.eye(3)
        self.greedy = np.argmax(br_q, axis=2)                          # first maximum wins
        self.norec = (br_q.mean(axis=2) == 0.0) if rule4 else np.zeros((nd, 3), bool)
        if self.quirks & EXT_SAMPLE_AR:      # r < y0 -> 0, r < y0 + y1 (float32) -> 1, else 2
            y01 = (ar_y[..., 0].astype(np.float32) + ar_y[..., 1].astype(np.float32)).astype(np.float64)
            t_ar = np.stack([ar_y[..., 0], y01 - ar_y[..., 0], 1.0 - y01], axis=2)
        else:
            t_ar = eye[np.argmax(ar_y, axis=2)]
        rnd = np.full((nd, 3, 3), 1.0 / 3.0)
        if remap_random:
            rnd = tree.remap(rnd)
        pr = self.p_rand[seat][:, None, None]
        t_br = (1.0 - pr) * eye[self.greedy] + pr * rnd
        self.t_ar, self.t_br = t_ar, t_br
        # ---- rule 1: the per-hand mixture, on the un-remapped rows
        w_br = self.p_br * tree.own_reach(t_br)
        w_ar = (1.0 - self.p_br) * tree.own_reach(t_ar)
        den = w_br + w_ar
        nz = den > 0
        self.acting_raw = np.full((nd, 3, 3), 1.0 / 3.0)
        self.acting_raw[nz] = (w_br[nz][:, None] * t_br[nz] + w_ar[nz][:, None] * t_ar[nz]) / den[nz][:, None]
        self.post_br = np.zeros((nd, 3))
        self.post_br[nz] = w_br[nz] / den[nz]
        self.acting = tree.remap(self.acting_raw)
        # ---- rule 2 per dealer, then the records
        self.p_dec = np.zeros((2, nd, 3, 3))
        self.p_rec = np.zeros((2, nd, 3, 3))
        self.p_sl = np.zeros((2, nd, 3))
        self.visit = np.zeros((2, nd, 3))
        self.reach = np.zeros((2, tree.nn, 3, 3))
        self.reward_mean = np.zeros(2)
        self.reward_var = np.zeros(2)
        for d in (0, 1):
            self._walk(d)
        # ---- the per-hand counters, by pairs of modes
        self.cnt_mean = np.zeros((2, 2 * NCNT))
        self.cnt_var = np.zeros((2, 2 * NCNT))
        for d in (0, 1):
            m1 = np.zeros(2 * NCNT)
            m2 = np.zeros(2 * NCNT)
            for br0 in (0, 1):
                for br1 in (0, 1):
                    wgt = (self.p_br if br0 else 1.0 - self.p_br) * (self.p_br if br1 else 1.0 - self.p_br)
                    if wgt > 0.0:
                        a, b = self._count_walk(d, (br0, br1))
                        m1 += wgt * a
                        m2 += wgt * b
            self.cnt_mean[d] = m1
            self.cnt_var[d] = m2 - m1 * m1

    def _walk(self, d):
        tree = self.tree
        N = tree.nodes
        reach = np.zeros((tree.nn, 3, 3))               # [node][seat 0's rank][seat 1's rank]
        reach[tree.root[d]] = tree.deal
        m1 = m2 = 0.0
        for n in range(tree.nn):                        # depth order: parents first
            par = int(N["parent"][n])
            if par >= 0:
                via = int(N["via"][n])
                if N["kind"][par] == CHANCE:
                    reach[n] = reach[par] * self.p_public[via]
                else:
                    col = self.acting[int(N["row"][par])][:, via]
                    reach[n] = reach[par] * (col[:, None] if N["p"][par] == 0 else col[None, :])
            if N["kind"][n] == TERMINAL:
                pay = tree.pay[int(N["row"][n]), 0].astype(np.float64)
                m1 += float((reach[n] * pay).sum())
                m2 += float((reach[n] * pay * pay).sum())
        self.reward_mean[d] = m1
        self.reward_var[d] = m2 - m1 * m1
        self.reach[d] = reach
        at = reach[tree.node_of_row]                    # [ndec, 3, 3]
        visit = np.where((self.seat == 0)[:, None], at.sum(axis=2), at.sum(axis=1))
        self.visit[d] = visit
        self.p_dec[d] = visit[:, :, None] * (self.acting_raw if self.rule3 else self.acting)
        self.p_sl[d] = visit * self.post_br
        none = self.p_sl[d] * (1.0 - self.p_rand[self.seat])[:, None] * self.norec
        self.p_rec[d] = self.p_dec[d] - none[:, :, None] * np.eye(3)[self.greedy]

    def _count_walk(self, d, modes):
        """(E X_k, E X_k^2) of the per-hand counters for dealer d when seat p acts in BR mode
        iff modes[p]: within one mode a seat's decisions are independent draws from one table,
        so the walk can carry each counter's distribution."""
        tree = self.tree
        N = tree.nodes
        K = 2 * NCNT
        dist = np.zeros((tree.nn, K, MAXDEC + 1, 3, 3))  # [node][counter][count][r0][r1]
        dist[tree.root[d], :, 0] = tree.deal
        tot = np.zeros((K, MAXDEC + 1))
        for n in range(tree.nn):
            par = int(N["parent"][n])
            if par >= 0 and dist[par].any():
                via = int(N["via"][n])
                if N["kind"][par] == CHANCE:
                    dist[n] = dist[par] * self.p_public[via]
                else:
                    pp, row = int(N["p"][par]), int(N["row"][par])
                    br = bool(modes[pp])
                    T = (self.t_br if br else self.t_ar)[row]
                    raws = (1, 2) if (via == 1 and not tree.legal[row]) else (via,)
                    shape = (K, 1, 3, 1) if pp == 0 else (K, 1, 1, 3)
                    for a in raws:
                        P = T[:, a]
                        inc = np.zeros((K, 3))
                        inc[NCNT * pp + ACT0 + (via if self.remap_counters else a)] = P
                        inc[NCNT * pp + N_RL] = P
                        if br:
                            inc[NCNT * pp + N_RL] = P - (1.0 - self.p_rand[pp]) * self.norec[row] * (self.greedy[row] == a)
                            inc[NCNT * pp + N_SL] = P
                        move = dist[par] * inc.reshape(shape)
                        assert not move[:, MAXDEC].any()
                        dist[n] += dist[par] * (P[None, :] - inc).reshape(shape)
                        dist[n][:, 1:] += move[:, :-1]
            if N["kind"][n] == TERMINAL:
                tot += dist[n].sum(axis=(2, 3))
        c = np.arange(MAXDEC + 1, dtype=np.float64)
        return tot @ c, tot @ (c * c)


# ---- a rollout's counts against the model -----------------------------------------------------
def _cells(out, name, obs, exp, p, n_cell, seat_cell, cut, zs, label):
    """Per-cell binomial z, exact zeros, and one pool per seat.  obs / exp / p / n_cell /
    seat_cell are flat arrays over the cells."""
    zero = p == 0.0
    big = (exp >= cut) & (exp <= n_cell - cut)
    bad = np.nonzero(zero & (obs != 0))[0]
    for i in bad[:5]:
        out["failures"].append(f"{name}: {int(obs[i])} records in a cell of probability 0: {label(int(i))}")
    z = (obs[big] - exp[big]) / np.sqrt(exp[big] * (1.0 - p[big]))
    out["z_cells"].extend(z.tolist())
    for i, zi in zip(np.nonzero(big)[0], z):
        if not abs(zi) <= zs:
            out["failures"].append(f"{name}: obs {int(obs[i])} exp {exp[i]:.2f} z {zi:.2f}: {label(int(i))}")
    out["n_stats"] += int(big.sum()) + int(zero.sum())
    small = ~big & ~zero
    for s in (0, 1):
        m = small & (seat_cell == s)
        e = float(exp[m].sum())
        o = float(obs[m].sum())
        out["n_stats"] += 1
        if e > 0.0:
            zp = (o - e) / math.sqrt(MAXDEC * e)
            out["z_other"].append(zp)
            if not abs(zp) <= zs:
                out["failures"].append(f"{name}: pool of seat {s} obs {o:.0f} exp {e:.2f} z {zp:.2f}")
        elif o != 0.0:
            out["failures"].append(f"{name}: pool of seat {s} holds {o:.0f} records, expected none")


def check_counts(model, obs, lane0, n, g, zs, cut=100.0, n_by_dealer=None):
    """Compare one rollout's counts with ``model``: global lanes [lane0, lane0 + n) at hand
    index g.  ``obs``: ``rl`` [ndec, 3, 3] (None under the alias quirk), ``sl`` [ndec, 3],
    ``actions`` [2, 3], ``reward0`` (seat 0's summed reward), ``n_rl`` [2], ``n_sl`` [2].
    Returns ``failures`` (empty iff every statistic is within ``zs``), the cell z's
    (``z_cells``), the other z's, and ``n_stats``.  ``n_by_dealer`` overrides the lanes per
    dealer (a wrong model for the teeth)."""
    nb = dealer_lanes(lane0, n, g) if n_by_dealer is None else np.asarray(n_by_dealer, np.int64)
    out = dict(failures=[], z_cells=[], z_other=[], n_stats=0)
    nd = model.tree.ndec
    n_row = nb[model.dealer_of_row].astype(np.float64)
    rows = np.arange(nd)
    if obs.get("rl") is not None:
        p = model.p_rec[model.dealer_of_row, rows]                     # [ndec, 3, 3]
        _cells(out, "RL", np.asarray(obs["rl"], np.float64).reshape(-1), (n_row[:, None, None] * p).reshape(-1),
               p.reshape(-1), np.repeat(n_row, 9), np.repeat(model.seat, 9), cut, zs,
               lambda i: f"{model.tree.describe(i // 9)}, holding rank {i // 3 % 3}, action {i % 3}")
    p = model.p_sl[model.dealer_of_row, rows]                          # [ndec, 3]
    _cells(out, "SL", np.asarray(obs["sl"], np.float64).reshape(-1), (n_row[:, None] * p).reshape(-1),
           p.reshape(-1), np.repeat(n_row, 3), np.repeat(model.seat, 3), cut, zs,
           lambda i: f"{model.tree.describe(i // 3)}, holding rank {i % 3}")
    mean = nb @ model.cnt_mean
    var = nb @ model.cnt_var
    got = np.zeros(2 * NCNT)
    for s in (0, 1):
        got[NCNT * s:NCNT * s + 3] = obs["actions"][s]
        got[NCNT * s + N_RL] = obs["n_rl"][s]
        got[NCNT * s + N_SL] = obs["n_sl"][s]
    names = [f"{what} of seat {s}" for s in (0, 1) for what in ("folds", "calls", "raises", "RL records", "SL records")]
    stats = [(names[k], got[k], mean[k], var[k]) for k in range(2 * NCNT)]
    stats.append(("reward of seat 0", float(obs["reward0"]), float(nb @ model.reward_mean), float(nb @ model.reward_var)))
    for k, (name, o, e, v) in enumerate(stats):
        out["n_stats"] += 1
        if k < 2 * NCNT and e < cut:                   # far from normal: the pool's conservative variance
            v = max(v, MAXDEC * e)
        if v > 0.0:
            z = (o - e) / math.sqrt(v)
            out["z_other"].append(z)
            if not abs(z) <= zs:
                out["failures"].append(f"{name}: obs {o:.1f} exp {e:.2f} z {z:.2f}")
        elif abs(o - e) > 1e-9 * max(1.0, abs(e)):
            out["failures"].append(f"{name}: obs {o:.1f} exp {e:.2f} with variance 0")
    return out


def summary(out) -> str:
    z = np.array(out["z_cells"] if out["z_cells"] else [0.0])
    zo = np.array(out["z_other"] if out["z_other"] else [0.0])
    return (f"cells {len(out['z_cells'])} max|z| {np.abs(z).max():.2f} rms z {np.sqrt((z * z).mean()):.2f}; "
            f"others {len(out['z_other'])} max|z| {np.abs(zo).max():.2f}; statistics {out['n_stats']}")


def rms(out) -> float:
    z = np.array(out["z_cells"])
    return float(np.sqrt((z * z).mean()))


# ---- independence of two sets of lanes -------------------------------------------------------------
def match_z(code_a, code_b, cls):
    """z of the number of pairs with equal fingerprints.  ``code_a[i]`` / ``code_b[i]``: the
    fingerprints of pair i's two hands (disjoint pairs: no hand is in two of them), ``cls[i]``
    the pair's dealer-parity class.  Under independence the matches of a class of n pairs are
    binomial(n, sum_c qA_c qB_c), with qA and qB the two sides' marginals in that class (taken
    from the data)."""
    code_a, code_b, cls = (np.asarray(v, np.int64) for v in (code_a, code_b, cls))
    obs = exp = var = 0.0
    for c in np.unique(cls):
        m = cls == c
        a, b = code_a[m], code_b[m]
        n = int(m.sum())
        k = int(max(a.max(), b.max())) + 1
        pi = float((np.bincount(a, minlength=k) / n) @ (np.bincount(b, minlength=k) / n))
        obs += float((a == b).sum())
        exp += n * pi
        var += n * pi * (1.0 - pi)
    return (obs - exp) / math.sqrt(var), obs, exp

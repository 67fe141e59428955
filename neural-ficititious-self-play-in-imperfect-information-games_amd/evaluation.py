"""Exact evaluation of any policy, and a tabular equilibrium to measure against.

``exploitability`` scores a pair of AR nets.  The rest of this module scores every kind of
policy the project meets, on the same public tree and with the same f64 walk
(``nfsp_evaluate_batch``, csrc/evaluate.hip):

* ``Policy.ar(w, mode)``    an average-policy net, as its softmax (mode 0) or argmax (mode 1);
* ``Policy.br(w, linear)``  a best-response net played greedily, as the rollout executes it
                            when the epsilon draw does not fire (first maximum wins, an illegal
                            raise becomes a call) -- the learned best response of the evaluator
                            the reference left commented out (main.py:82-120);
* ``Policy.table(t)``       a behavioural strategy ``[ndec][3 ranks][3 actions]`` over the rows of
                            ``GameTree``: a net read out with ``policy_table``, a ``mix`` of
                            tables, a ``CfrSolver``, ``XfpSolver`` or ``MccfrSolver`` average, a
                            ``best_response``, anything written by hand.

``best_response`` (``nfsp_best_response_table``) gives the exact best responses the scores
are the values of as a table, with the exact action values at every information set: where a
learned BR net deviates, and by how much.

``GameTree`` (host only, no GPU) is the tree as data; ``CfrSolver`` runs CFR+ on it
(``nfsp_cfr_*``, csrc/cfr.hip), which anchors the Leduc variant the way the analytic Nash
family anchors Kuhn.  ``XfpSolver`` runs full-width fictitious play on it (``nfsp_xfp_*``,
csrc/xfp.hip), n runs over eta and the weighting at once: the curve of the algorithm NFSP
approximates, with an exact best response and exact averaging.  ``MccfrSolver`` runs
external-sampling MCCFR on it (``nfsp_mccfr_*``, csrc/mccfr.hip): the sampled tabular yardstick,
counted in traversals and terminals visited, to set beside the engine's curves in hands;
``MccfrOsSolver`` runs outcome sampling on the same handle (``nfsp_mccfr_os_*``), whose traversal
is one sampled hand, so its cost is in the engine's own unit, and ``MccfrVrSolver`` the same
paths with baseline-corrected values (``nfsp_mccfr_vr_*``, VR-MCCFR).  ``MccfrXSolver`` puts
regret matching+ and linear averaging on any of the three (``nfsp_mccfr_x_*``), and
``MccfrNetSolver`` holds the regrets in two 30-H-3 nets per run (``nfsp_mccfr_net_*``; H is 64, or
16, 32 or 128 through ``hidden`` / ``init_nets``): sampled regression CFR on the same walks.

``MemoryTable`` is a memory counted per information set on the device (``nfsp_memory_table``,
csrc/memtab.hip): M_SL as the tabular average strategy the AR net is a fit of, M_RL as what the
BR net had to learn from; ``diagnostics.memory_reports`` scores the former beside the nets.

``head_tables`` (``nfsp_head_tables``) reads out the Q values a BR net holds where ``policy_table``
only has its one-hot argmax, ``td_table`` (``nfsp_td_table``) counts the TD values the net is
fitted to per (information set, action) over M_RL where it lies, and ``q_report_from`` splits the
BR net's error against ``best_response``'s exact action values in two: what the data say against
the truth, and what the net makes of its data.

``fit_tables`` (``nfsp_fit_tables``, csrc/fit_tables.hip) goes the other way: ``FitJob``s put a
table into a packed net by weighted full-batch gradient descent on the device, and
``visit_weights`` gives the exact visit distribution to weight them with.  The fit, ``head_tables``
and the regret nets take packed nets of hidden width 16, 32, 64 or 128 (``net_width`` reads it from
a net's length); ``net_policy`` turns a net of any of them into the ``Policy.table`` it executes,
which is how ``evaluate`` and ``best_response`` score a width the evaluators' net kinds (64) lack.

Nothing here knows an engine: what needs both an engine and this module is ``diagnostics``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import native

DECISION, CHANCE, TERMINAL = 0, 1, 2
ACTIONS = ("fold", "call", "raise")
NODE_DTYPE = np.dtype([("kind", "i1"), ("p", "i1"), ("via", "i1"), ("nchild", "i1"), ("parent", "<i4"),
                       ("child", "<i4", (3,)), ("row", "<i4")])
RESULT_KEYS = ("br0", "br1", "exploitability", "value0", "value0_dealer0", "value0_dealer1")


class GameTree:
    """The evaluator's public tree of ``game`` (``nfsp_tree_export``), in depth order.

    ``nodes`` (NODE_DTYPE), ``obs[ndec, 3]``, ``legal[ndec]`` (whether a raise is executed as a
    raise), ``seat[ndec]`` (who acts), ``pay[nterm, 2, 3, 3]``, ``lev[nlev + 1]``, ``root[2]``
    (by dealer), ``deal[3, 3]``; ``node_of_row[ndec]`` maps a decision row back to its node.

    ``GameTree.of(game)`` is the one shared tree of a game, its arrays read-only."""
    _shared = {}

    @classmethod
    def of(cls, game: int = native.GAME_LEDUC) -> "GameTree":
        game = int(game)
        if game not in cls._shared:
            tree = cls(game)
            for a in vars(tree).values():
                if isinstance(a, np.ndarray):
                    a.flags.writeable = False
            cls._shared[game] = tree
        return cls._shared[game]

    def __init__(self, game: int = native.GAME_LEDUC):
        L = native.load()
        self.game = int(game)
        n = [C.c_int32(0) for _ in range(4)]
        native.check(L.nfsp_tree_size(self.game, *[C.byref(x) for x in n]), "nfsp_tree_size")
        self.nn, self.ndec, self.nterm, self.nlev = (x.value for x in n)
        self.nodes = np.zeros(self.nn, NODE_DTYPE)
        assert NODE_DTYPE.itemsize == C.sizeof(native.TreeNode) == 24
        self.obs = np.zeros((self.ndec, 3), np.uint32)
        bits = np.zeros(self.ndec, np.uint8)
        self.pay = np.zeros((self.nterm, 2, 3, 3), np.float32)
        self.lev = np.zeros(self.nlev + 1, np.int32)
        self.root = np.zeros(2, np.int32)
        self.deal = np.zeros((3, 3), np.float64)
        native.check(L.nfsp_tree_export(self.game, *[a.ctypes.data_as(native.P) for a in (
            self.nodes, self.obs, bits, self.pay, self.lev, self.root, self.deal)]), "nfsp_tree_export")
        self.legal = (bits & 1).astype(bool)
        self.seat = (bits >> 1).astype(np.int8)
        self.node_of_row = np.full(self.ndec, -1, np.int32)
        dec = np.nonzero(self.nodes["kind"] == DECISION)[0]
        self.node_of_row[self.nodes["row"][dec]] = dec
        self._rows = {(int(self.seat[d]), int(self.obs[d, r])): (d, r)
                      for d in range(self.ndec) for r in range(3)}

    def row_of(self, seat: int, obs: int) -> tuple:
        """(row, rank) of the information set in which ``seat`` observes ``obs`` (30 bits)."""
        return self._rows[(int(seat), int(obs))]

    def path(self, row: int) -> tuple:
        """(dealer, [node ids from the root to the decision of ``row``])."""
        chain = [int(self.node_of_row[row])]
        while self.nodes["parent"][chain[-1]] >= 0:
            chain.append(int(self.nodes["parent"][chain[-1]]))
        chain.reverse()
        return int(np.nonzero(self.root == chain[0])[0][0]), chain

    def describe(self, row: int) -> str:
        """The decision of ``row`` as text: the dealer, the executed actions so far (by seat),
        the public rank once it is dealt, and who acts."""
        dealer, chain = self.path(row)
        parts, public = [], None
        for par, n in zip(chain[:-1], chain[1:]):
            via = int(self.nodes["via"][n])
            if self.nodes["kind"][par] == CHANCE:
                public = via
                parts.append(f"| public {via} |")
            else:
                parts.append(f"{int(self.nodes['p'][par])}:{ACTIONS[via]}")
        hist = " ".join(parts) if parts else "-"
        pub = "none" if public is None else str(public)
        return (f"dealer {dealer}, history {hist}, public rank {pub}, seat {int(self.seat[row])} to act"
                f"{'' if self.legal[row] else ' (raise -> call)'}")

    def uniform(self) -> np.ndarray:
        """The table that is uniform over the legal actions of every row."""
        t = np.zeros((self.ndec, 3, 3))
        t[self.legal] = 1.0 / 3.0
        t[~self.legal, :, :2] = 0.5
        return t

    def remap(self, table) -> np.ndarray:
        """``table`` as executed: an illegal raise's mass goes to call (the env's remap)."""
        t = np.array(table, np.float64).reshape(self.ndec, 3, 3)
        il = ~self.legal
        t[il, :, 1] = t[il, :, 1] + t[il, :, 2]
        t[il, :, 2] = 0.0
        return t

    def own_reach(self, table) -> np.ndarray:
        """[ndec, 3]: the product of the acting seat's own action probabilities (holding rank
        r, under ``table`` as executed) along the path to each decision."""
        t = self.remap(table)
        reach = np.ones((self.nn, 2, 3))          # [node][seat][that seat's rank]
        N = self.nodes
        for n in range(self.nn):                  # depth order: parents first
            par = int(N["parent"][n])
            if par < 0:
                continue
            reach[n] = reach[par]
            if N["kind"][par] == DECISION:
                reach[n, N["p"][par]] = reach[par, N["p"][par]] * t[N["row"][par], :, N["via"][n]]
        return reach[self.node_of_row, self.seat.astype(int)]


def mix(tree: GameTree, parts) -> np.ndarray:
    """The behavioural strategy realisation-equivalent to drawing table k with probability
    w_k once **per hand** and playing it to the end (Kuhn's theorem) -- how self-play mixes
    the BR and AR nets (one eta draw per hand and agent, main.py:36-45), so
    ``mix(tree, [(eta, br_table), (1 - eta, ar_table)])`` is the policy an NFSP agent plays.

    Row (d, r) is the tables' rows weighted by w_k x the own reach of (d, r) under table k
    (``GameTree.own_reach``); where that total is 0 the row is uniform over the legal actions.
    The result serves either seat: each row only uses the reach of the seat acting there.

    A mixture drawn anew at every decision needs none of this, it is plain row arithmetic:
    epsilon-greedy with the reference's random action (agent/agent.py:124-128 draws three
    uniforms and the env takes their argmax, i.e. uniform over the three actions, then the
    remap) is ``(1 - eps) * greedy + eps * tree.remap(np.full_like(greedy, 1 / 3))``."""
    num = np.zeros((tree.ndec, 3, 3))
    den = np.zeros((tree.ndec, 3))
    for w, table in parts:
        t = tree.remap(table)
        wr = float(w) * tree.own_reach(t)
        num = num + wr[:, :, None] * t
        den = den + wr
    out = tree.uniform()
    nz = den > 0
    out[nz] = num[nz] / den[nz][:, None]
    return out


class Policy:
    """A policy spec (``nfsp_policy``): a kind and the device memory it reads, kept alive here."""

    def __init__(self, kind: int, data=None, ptr: int | None = None, owner=None):
        self.kind = int(kind)
        self.data = data            # a torch tensor on the device, or None for a borrowed pointer
        self.owner = owner          # whatever owns a borrowed pointer
        self.ptr = int(data.data_ptr() if ptr is None else ptr)

    @staticmethod
    def _dev(x, dtype, numel=None):
        import torch
        if isinstance(x, int):
            return None, x
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x))
        t = t.to(device="cuda", dtype=dtype).contiguous().reshape(-1)
        if numel is not None and t.numel() != numel:
            raise ValueError(f"expected {numel} values, got {t.numel()}")
        return t, None

    @classmethod
    def ar(cls, weights, mode: int = 0, owner=None) -> "Policy":
        """An AR net (packed f32 weights: array, tensor or device address), softmax or argmax."""
        import torch
        if mode not in (0, 1):
            raise ValueError("mode must be 0 (softmax) or 1 (argmax)")
        t, p = cls._dev(weights, torch.float32, native.NP)
        return cls(native.POL_AR_ARGMAX if mode else native.POL_AR_SOFTMAX, t, p, owner)

    @classmethod
    def br(cls, weights, linear: bool = False, owner=None) -> "Policy":
        """A BR net played greedily; ``linear`` for the Q head of ``EXT_LINEAR_Q``."""
        import torch
        t, p = cls._dev(weights, torch.float32, native.NP)
        return cls(native.POL_BR_GREEDY_LINEAR if linear else native.POL_BR_GREEDY, t, p, owner)

    @classmethod
    def table(cls, table, owner=None) -> "Policy":
        """A table ``[ndec][3][3]`` of doubles (array, tensor or device address)."""
        import torch
        t, p = cls._dev(table, torch.float64)
        return cls(native.POL_TABLE, t, p, owner)

    def spec(self) -> native.PolicySpec:
        return native.PolicySpec(self.kind, 0, native.P(self.ptr))


def exploitability(ctx, dev_w_ar0: int, dev_w_ar1: int, mode: int = 0) -> dict:
    """nfsp_exploitability on two packed AR nets given as device pointers."""
    out = (C.c_double * 4)()
    native.check(ctx.L.nfsp_exploitability(ctx.h, dev_w_ar0, dev_w_ar1, mode, out), "nfsp_exploitability")
    return {"br0": out[0], "br1": out[1], "exploitability": out[2], "value0": out[3]}


def exploitability_batch(ctx, dev_w_ar0: list, dev_w_ar1: list, mode: int = 0) -> list:
    """nfsp_exploitability_batch on n pairs of packed AR nets (lists of device pointers)."""
    n = len(dev_w_ar0)
    assert len(dev_w_ar1) == n
    a0 = (C.c_void_p * max(n, 1))(*dev_w_ar0)
    a1 = (C.c_void_p * max(n, 1))(*dev_w_ar1)
    out = (C.c_double * (4 * max(n, 1)))()
    native.check(ctx.L.nfsp_exploitability_batch(ctx.h, a0, a1, n, mode, out), "nfsp_exploitability_batch")
    return [{"br0": out[4 * k], "br1": out[4 * k + 1], "exploitability": out[4 * k + 2], "value0": out[4 * k + 3]}
            for k in range(n)]


def _result(out, k):
    return {key: out[6 * k + j] for j, key in enumerate(RESULT_KEYS)}


def evaluate_batch(ctx, pairs) -> list:
    """``nfsp_evaluate_batch``: for every (policy at seat 0, policy at seat 1) the best-response
    values br0 / br1 against the other seat's policy, their sum, seat 0's on-policy value and
    that value over dealer-0 / dealer-1 hands only.  One workgroup per pair."""
    n = len(pairs)
    s0 = (native.PolicySpec * max(n, 1))(*[a.spec() for a, _ in pairs])
    s1 = (native.PolicySpec * max(n, 1))(*[b.spec() for _, b in pairs])
    out = (C.c_double * (6 * max(n, 1)))()
    native.check(ctx.L.nfsp_evaluate_batch(ctx.h, s0, s1, n, out), "nfsp_evaluate_batch")
    return [_result(out, k) for k in range(n)]


def evaluate(ctx, seat0: Policy, seat1: Policy) -> dict:
    return evaluate_batch(ctx, [(seat0, seat1)])[0]


def policy_table(ctx, policy: Policy, tree: GameTree | None = None):
    """``nfsp_policy_table``: the policy as executed at every row, a float64 device tensor
    ``[ndec, 3, 3]`` (``Policy.table`` of it scores bit-identically to ``policy``)."""
    import torch
    tree = tree or GameTree.of(ctx.game)
    out = torch.empty((tree.ndec, 3, 3), dtype=torch.float64, device="cuda")
    spec = policy.spec()
    native.check(ctx.L.nfsp_policy_table(ctx.h, C.byref(spec), native.P(out.data_ptr())), "nfsp_policy_table")
    return out


def best_response(ctx, seat0: Policy, seat1: Policy, values: bool = False, tree: GameTree | None = None):
    """``nfsp_best_response_table``: the exact best responses as one joint one-hot table, a
    float64 device tensor ``[ndec, 3, 3]`` -- rows where seat 0 acts hold its best response
    against ``seat1``, rows where seat 1 acts its best response against ``seat0`` (first maximum
    over the legal actions: ties and unreached information sets fold).  ``Policy.table`` of it
    scores ``evaluate``'s br0 at seat 0 and br1 at seat 1.

    With ``values`` returns ``(beta, q, reach)``: ``q[d, r, a]`` the counterfactual value of
    action a (0 for an illegal raise), ``reach[d, r]`` the counterfactual reach of the
    information set, so ``q / reach`` is the exact expected chips per action given that it is
    reached -- what a BR net's Q head is to learn there."""
    import torch
    tree = tree or GameTree.of(ctx.game)
    beta = torch.empty((tree.ndec, 3, 3), dtype=torch.float64, device="cuda")
    q = torch.empty((tree.ndec, 3, 3), dtype=torch.float64, device="cuda") if values else None
    reach = torch.empty((tree.ndec, 3), dtype=torch.float64, device="cuda") if values else None
    s0, s1 = seat0.spec(), seat1.spec()
    native.check(ctx.L.nfsp_best_response_table(
        ctx.h, C.byref(s0), C.byref(s1), native.P(beta.data_ptr()),
        native.P(q.data_ptr()) if values else None, native.P(reach.data_ptr()) if values else None),
        "nfsp_best_response_table")
    return (beta, q, reach) if values else beta


class MemoryTable:
    """A memory counted per information set (``nfsp_memory_table``): ``raw`` is the int64 array
    ``[ndec, 3 ranks, 3 actions, 3 fields]`` over the rows of ``tree``.

    ``kind`` ``native.MEM_SL``: field 0 the records whose argmax is the action, field 1 the sum of
    the stored action vectors' component in 2^-24 units.  ``native.MEM_RL``: field 0 the records
    whose stored argmax is the action, field 1 the sum of their rewards in half chips, field 2
    how many of them are terminal.

    ``native.MEM_TD`` (``td_table``): field 0 as ``MEM_RL``, field 1 the sum of the records' TD
    values v = r + gamma max Q_target(s2) and field 2 the sum of max Q_target(s2) over the records
    that bootstrap, both in 2^-24 units.  ``native.MEM_TDQ`` (``tdq_table``): the same with a Q
    table's row at s2 in Q_target's place.

    ``counts[ndec, 3, 3]`` is field 0 and ``n[ndec, 3]`` the records per information set."""

    def __init__(self, tree: GameTree, kind: int, raw):
        self.tree = tree
        self.kind = int(kind)
        if hasattr(raw, "cpu"):
            raw = raw.cpu().numpy()
        self.raw = np.array(raw, np.int64).reshape(tree.ndec, 3, 3, 3)
        self.counts = self.raw[..., 0]
        self.n = self.counts.sum(axis=2)

    def policy(self, how: str = "argmax") -> np.ndarray:
        """The memory as a behavioural strategy, float64 ``[ndec, 3, 3]`` for ``Policy.table``:
        "argmax" normalises the counts (the textbook NFSP average), "mass" the summed action
        vectors (the exact minimiser of the AR net's cross-entropy).  A row without records (for
        "mass": whose sum is 0) is ``tree.uniform()``'s row."""
        if how not in ("argmax", "mass"):
            raise ValueError('how must be "argmax" or "mass"')
        if self.kind != native.MEM_SL and how == "mass":
            raise ValueError('"mass" is defined for M_SL tables only')
        w = self.raw[..., 0 if how == "argmax" else 1].astype(np.float64)
        tot = w.sum(axis=2)
        out = self.tree.uniform()
        nz = tot != 0
        out[nz] = w[nz] / tot[nz][:, None]
        return out

    def _rl(self):
        if self.kind != native.MEM_RL:
            raise AttributeError("mean_r / terminal belong to M_RL tables")

    @property
    def mean_r(self) -> np.ndarray:
        """M_RL: the mean stored reward in chips per (row, rank, action); NaN without records."""
        self._rl()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.counts > 0, self.raw[..., 1] / (2.0 * self.counts), np.nan)

    @property
    def terminal(self) -> np.ndarray:
        """M_RL: the terminal records per (row, rank, action)."""
        self._rl()
        return self.raw[..., 2]

    def _td_mean(self, field):
        if self.kind not in (native.MEM_TD, native.MEM_TDQ):
            raise AttributeError("mean_v / mean_bootstrap belong to TD tables")
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.where(self.counts > 0, self.raw[..., field] / (2.0**native.MEMTAB_FIX_SHIFT * self.counts), np.nan)
        # a TDQ table's means are the float32 values its rows hold (``table_rows``, ROWS_TD_MEAN)
        return m.astype(np.float32).astype(np.float64) if self.kind == native.MEM_TDQ else m

    @property
    def mean_v(self) -> np.ndarray:
        """TD: the mean TD value in chips per (row, rank, stored action); NaN without records."""
        return self._td_mean(1)

    @property
    def mean_bootstrap(self) -> np.ndarray:
        """TD: the mean of max Q_target(s2) per (row, rank, stored action), a record that does not
        bootstrap counting as 0; NaN without records."""
        return self._td_mean(2)


def _segments(records, size):
    """``records`` of ``memory_table`` / ``td_table`` as (a ``MemSegment`` array, its length)."""
    import torch
    if isinstance(records, torch.Tensor) or (isinstance(records, tuple) and isinstance(records[0], int)):
        records = [records]
    segs = []
    for r in records:
        if isinstance(r, torch.Tensor):
            nbytes = r.numel() * r.element_size()
            if not r.is_contiguous() or nbytes % size:
                raise ValueError("a segment must be a contiguous tensor of whole records")
            segs.append(native.MemSegment(native.P(r.data_ptr()), nbytes // size))
        else:
            segs.append(native.MemSegment(native.P(int(r[0])), int(r[1])))
    return (native.MemSegment * max(len(segs), 1))(*segs), len(segs)


def memory_table(ctx, kind: int, seat: int, records, out=None, tree: GameTree | None = None):
    """``nfsp_memory_table``: packed device records (``SlRec`` 16 B / ``RlRec`` 32 B) of ``seat``
    counted into the seat's rows of ``out``, an int64 device tensor ``[ndec, 3, 3, 3]`` (zeros
    when not given; the other seat's rows are left as they are).  ``records``: one segment or a
    list of them, each a contiguous device tensor of whole records or ``(device address, n)``.
    Returns ``(out, info)``; ``MemoryTable(tree, kind, out)`` reads it."""
    import torch
    tree = tree or GameTree.of(ctx.game)
    arr, nsegs = _segments(records, 16 if kind == native.MEM_SL else 32)
    if out is None:
        out = torch.zeros((tree.ndec, 3, 3, 3), dtype=torch.int64, device="cuda")
    info = native.MemtabInfo()
    native.check(ctx.L.nfsp_memory_table(ctx.h, tree.game, int(kind), int(seat), arr, nsegs,
                                         native.P(out.data_ptr()), C.byref(info)), "nfsp_memory_table")
    return out, info.to_dict()


def td_table(ctx, seat: int, records, target_w, gamma: float, quirks: int, out=None, tree: GameTree | None = None):
    """``nfsp_td_table``: the TD values the BR net is fitted to (agent/agent.py:219-241), counted
    over packed ``RlRec`` device records of ``seat`` into the seat's rows of ``out`` (as
    ``memory_table``).  Per record v = r + gamma max Q_target(s2), or r where the record is terminal
    and ``QUIRK_TERMINAL_BOOTSTRAP`` is off, with ``k_br_targets``' arithmetic; ``target_w`` is the
    packed target net (array, tensor or device address), its head linear with ``EXT_LINEAR_Q`` in
    ``quirks``.  The key is the stored s and the stored argmax: under ``QUIRK_ALIAS_RL`` the hand's
    LAST s.  Returns ``(out, info)``; ``MemoryTable(tree, native.MEM_TD, out)`` reads it."""
    import torch
    tree = tree or GameTree.of(ctx.game)
    arr, nsegs = _segments(records, 32)
    w, addr = Policy._dev(target_w, torch.float32, native.NP)
    if out is None:
        out = torch.zeros((tree.ndec, 3, 3, 3), dtype=torch.int64, device="cuda")
    td = native.TdArgs(native.P(w.data_ptr() if addr is None else addr), float(gamma), int(quirks), 0)
    info = native.MemtabInfo()
    native.check(ctx.L.nfsp_td_table(ctx.h, tree.game, int(seat), arr, nsegs, C.byref(td), native.P(out.data_ptr()),
                                     C.byref(info)), "nfsp_td_table")
    return out, info.to_dict()


def tdq_table(ctx, seat: int, records, q, gamma: float, quirks: int, out=None, tree: GameTree | None = None):
    """``nfsp_tdq_table``: ``td_table`` with a Q table in the target net's place -- one fitted-Q
    sweep's sums.  ``q``: float32 ``[ndec, 3, 3]`` over ``tree``'s rows (array or device tensor); a
    record bootstraps from the largest of the three entries at the information set of its s2, and
    from 0 where s2 is none (a terminal observation).  Only ``QUIRK_TERMINAL_BOOTSTRAP`` of
    ``quirks`` is read.  Returns ``(out, info)``; ``MemoryTable(tree, native.MEM_TDQ, out)`` reads
    it, and ``table_rows(ctx, native.ROWS_TD_MEAN, out, fill)`` is the sweep's Q table."""
    import torch
    tree = tree or GameTree.of(ctx.game)
    arr, nsegs = _segments(records, 32)
    qd, _ = Policy._dev(q, torch.float32, tree.ndec * 9)
    if out is None:
        out = torch.zeros((tree.ndec, 3, 3, 3), dtype=torch.int64, device="cuda")
    info = native.MemtabInfo()
    native.check(ctx.L.nfsp_tdq_table(ctx.h, tree.game, int(seat), arr, nsegs, native.P(qd.data_ptr()), float(gamma),
                                      int(quirks), native.P(out.data_ptr()), C.byref(info)), "nfsp_tdq_table")
    return out, info.to_dict()


def table_rows(ctx, stat: int, tabs, fill=None, prev=None, tree: GameTree | None = None):
    """``nfsp_table_rows``: int64 tables ``[n, ndec, 3, 3, 3]`` (or one, ``[ndec, 3, 3, 3]``; array,
    tensor or ``MemoryTable``) as the float32 rows a slot acts on, on the device.  ``stat``
    ``native.ROWS_TD_MEAN``: field 1 / field 0 in chips per (set, action), of a TD or TDQ table;
    ``ROWS_SL_MASS`` / ``ROWS_SL_ARGMAX``: an M_SL table's summed action vectors / argmax counts
    normalised per set, before the raise-to-call remap.  Where the table has no data -- an entry
    without records, an M_SL set without records or without positive mass -- the value is ``fill``'s
    (float32, the tables' shape with 3 in place of the fields), 0 without ``fill``.  Returns
    ``(rows, changed)``: a float32 device tensor of ``fill``'s shape and per table the entries whose
    bits differ from ``prev``'s (``None`` without ``prev``)."""
    import torch
    tree = tree or GameTree.of(ctx.game)
    raw = tabs.raw if isinstance(tabs, MemoryTable) else tabs
    t = raw if isinstance(raw, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(raw))
    if t.dtype != torch.int64 or t.numel() % (tree.ndec * 27):
        raise ValueError(f"table_rows: int64 tables [n, {tree.ndec}, 3, 3, 3]")
    one = t.dim() == 4
    t = t.cuda().contiguous()
    n = t.numel() // (tree.ndec * 27)

    def rows_like(x, what):
        if x is None:
            return None
        x = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x))
        if x.dtype != torch.float32 or x.numel() != n * tree.ndec * 9:
            raise ValueError(f"table_rows: {what} must be float32 [{n}, {tree.ndec}, 3, 3]")
        return x.cuda().contiguous()
    fill, prev = rows_like(fill, "fill"), rows_like(prev, "prev")
    out = torch.empty((tree.ndec, 3, 3) if one else (n, tree.ndec, 3, 3), dtype=torch.float32, device="cuda")
    changed = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    native.check(ctx.L.nfsp_table_rows(ctx.h, tree.game, int(stat), native.ptr(t), native.ptr(fill), native.ptr(prev), n,
                                       native.ptr(out), native.ptr(changed)), "nfsp_table_rows")
    if prev is None:
        return out, None
    c = changed[:n].cpu().tolist()
    return out, c[0] if one else c


def net_width(w) -> int:
    """The hidden width of a packed net (array or tensor), from its length 34 H + 3; a length that
    is no built width's (``native.FIT_WIDTHS``) is refused.  A device address carries no length: 64."""
    if isinstance(w, int):
        return 64
    n = int(w.numel() if hasattr(w, "numel") else np.asarray(w).size)
    for h in native.FIT_WIDTHS:
        if n == native.net_params(h):
            return h
    raise ValueError(f"a packed net has 34 H + 3 values for H in {native.FIT_WIDTHS}, got {n}")


def _one_width(nets, what: str, hidden=None) -> int:
    """the one width of ``nets`` (``hidden`` for device addresses, 64 without it); mixed widths are refused"""
    ws = {int(hidden) if isinstance(w, int) and hidden is not None else net_width(w) for w in nets}
    if hidden is not None:
        ws.add(int(hidden))
    if len(ws) > 1:
        raise ValueError(f"{what}: nets of widths {sorted(ws)} in one call; one width per call")
    h = ws.pop() if ws else 64
    native.net_params(h)
    return h


def head_tables(ctx, nets, acts, tree: GameTree | None = None, hidden=None):
    """``nfsp_head_tables``: the raw head outputs of packed nets (arrays, tensors or device
    addresses) at every row and rank, a float32 device tensor ``[n, ndec, 3, 3]`` -- for a BR net
    the Q values it holds, with the bits the rollout acts on.  ``acts[k]``: ``native.ACT_RELU``,
    ``ACT_LINEAR`` or ``ACT_SOFTMAX``.  All three outputs are there, an illegal raise's too.
    The width is the nets' (``net_width``; ``hidden`` for device addresses), one per call: other
    than 64, or with ``hidden`` given, the call is ``nfsp_head_tables_h``'s plain kernel."""
    import torch
    tree = tree or GameTree.of(ctx.game)
    n = len(nets)
    if len(acts) != n:
        raise ValueError("one act per net")
    H = _one_width(nets, "head_tables", hidden)
    keep = [Policy._dev(w, torch.float32, native.net_params(H)) for w in nets]
    ptrs = (native.P * max(n, 1))(*[t.data_ptr() if p is None else p for t, p in keep])
    act = (native.I32 * max(n, 1))(*[int(a) for a in acts])
    out = torch.empty((n, tree.ndec, 3, 3), dtype=torch.float32, device="cuda")
    if H == 64 and hidden is None:
        native.check(ctx.L.nfsp_head_tables(ctx.h, tree.game, ptrs, act, n, native.P(out.data_ptr())), "nfsp_head_tables")
    else:
        native.check(ctx.L.nfsp_head_tables_h(ctx.h, tree.game, H, ptrs, act, n, native.P(out.data_ptr())),
                     "nfsp_head_tables_h")
    return out


_KIND_ACT = {native.POL_AR_SOFTMAX: native.ACT_SOFTMAX, native.POL_AR_ARGMAX: native.ACT_SOFTMAX,
             native.POL_BR_GREEDY: native.ACT_RELU, native.POL_BR_GREEDY_LINEAR: native.ACT_LINEAR}


def heads_table(heads, legal, kind: int) -> np.ndarray:
    """Heads ``[ndec, 3, 3]`` (softmax rows for the AR kinds, ReLU / linear Q values for the BR
    kinds) as the float64 table a net of that ``native.POL_*`` kind executes: softmax rows pass
    through, the other kinds are one-hot at the first maximum (an all-zero head folds); a raise
    where ``legal[d]`` is false goes to call."""
    if kind not in _KIND_ACT:
        raise ValueError("heads_table: kind must be one of the four net kinds (native.POL_*)")
    y = np.asarray(heads, np.float32).astype(np.float64).reshape(-1, 3, 3)
    legal = np.asarray(legal, bool).reshape(-1)
    if len(legal) != len(y):
        raise ValueError("heads_table: one legal flag per decision row")
    if kind != native.POL_AR_SOFTMAX:
        y = np.eye(3)[np.argmax(y, axis=2)]        # numpy's argmax: the first maximum
    out = y.copy()
    il = ~legal
    out[il, :, 1] = y[il, :, 1] + y[il, :, 2]
    out[il, :, 2] = 0.0
    return out


def net_policy(ctx, w, kind: int = native.POL_AR_SOFTMAX, tree: GameTree | None = None) -> "Policy":
    """A packed net of any built width as the ``Policy.table`` it executes under ``kind``
    (``native.POL_AR_SOFTMAX``, ``POL_AR_ARGMAX``, ``POL_BR_GREEDY``, ``POL_BR_GREEDY_LINEAR``):
    ``head_tables`` at the net's width, then ``heads_table``.  What ``evaluate``, ``best_response``
    and the solvers score a net of width other than 64 through; the evaluators' own net kinds are
    64 wide."""
    tree = tree or GameTree.of(ctx.game)
    if kind not in _KIND_ACT:
        raise ValueError("net_policy: kind must be one of the four net kinds (native.POL_*)")
    z = head_tables(ctx, [w], [_KIND_ACT[kind]], tree, hidden=net_width(w))[0].cpu().numpy()
    return Policy.table(heads_table(z, tree.legal, kind))


def act_rows(table):
    """A policy table (float64 ``[ndec, 3, 3]``: array or tensor, as ``policy_table``,
    ``best_response``, ``mix`` and the solvers' averages give them) as the float32 rows a slot of
    an engine acts with (``SelfPlayEngine.set_act_table``): one rounding per value, so exact for
    one-hot rows.  A tensor stays on its device.  Values that are not finite, or not after the
    rounding, are refused: a table acts as it stands, nothing downstream would catch them."""
    import torch
    t = table if isinstance(table, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(table))
    if t.numel() % 9:
        raise ValueError(f"a table has 9 values per row, got {t.numel()} values")
    t = t.to(torch.float32).reshape(-1, 3, 3).contiguous()
    if not bool(torch.isfinite(t).all()):
        raise ValueError("act_rows: the table has values that are not finite (as float32)")
    return t


def glorot_net(rng: np.random.RandomState, hidden: int = 64) -> np.ndarray:
    """Keras defaults: glorot_uniform kernels, zero biases; packed like nfsp.h."""
    def g(fi, fo):
        lim = np.sqrt(6.0 / (fi + fo))
        return rng.uniform(-lim, lim, size=(fi, fo)).astype(np.float32)
    return np.concatenate([g(30, hidden).ravel(), np.zeros(hidden, np.float32),
                           g(hidden, 3).ravel(), np.zeros(3, np.float32)])


FIT_LOSSES = {"ce": native.FIT_CE, "mse": native.FIT_MSE, "huber": native.FIT_HUBER}


class FitJob:
    """One job of ``fit_tables`` (``nfsp_fit_job``): the packed net ``w`` fitted to ``seat``'s rows
    of ``target`` (float64 ``[ndec, 3, 3]`` over ``GameTree``'s rows) by full-batch gradient descent
    with momentum.  ``head``: ``native.ACT_SOFTMAX`` with ``loss`` "ce", ``ACT_RELU`` or
    ``ACT_LINEAR`` with "mse" or "huber".  ``weight``: float64 ``[ndec, 3]`` >= 0 per information
    set (None: 1); ``mask``: ``[ndec, 3, 3]``, nonzero where an entry has a target (None: the legal
    actions; not with "ce"); ``v``: the momentum state, float32 like ``w`` (None: zero at the
    call's start, dropped at its end).  The hidden width is ``w``'s (``net_width``; ``hidden`` where
    ``w`` is a device address, 64 without it) and is kept as ``.hidden``.  Every input is an array, a device tensor or a device
    address, in the style of ``Policy``; ``w`` and ``v`` are updated in place where they are device
    tensors or addresses, and ``self.w`` / ``self.v`` are the device tensors otherwise."""

    def __init__(self, w, target, seat: int, head: int, loss, lr: float, momentum: float = 0.0, weight=None,
                 mask=None, v=None, hidden=None):
        import torch

        def dev(x, dtype, numel=None):
            if x is None:
                return None, None
            t, p = Policy._dev(x, dtype, numel)
            return t, int(t.data_ptr() if p is None else p)
        self.hidden = _one_width([w] + ([] if v is None else [v]), "FitJob (w and v)", hidden)
        self.w, self._w = dev(w, torch.float32, native.net_params(self.hidden))
        self.v, self._v = dev(v, torch.float32, native.net_params(self.hidden))
        self.target, self._t = dev(target, torch.float64)
        self.weight, self._wt = dev(weight, torch.float64)
        self.mask, self._m = dev(mask, torch.uint8)
        self.seat, self.head = int(seat), int(head)
        self.loss = int(FIT_LOSSES.get(loss, loss))
        self.lr, self.momentum = float(lr), float(momentum)

    def spec(self) -> native.FitJob:
        return native.FitJob(self._w, self._v, self._t, self._wt, self._m, self.seat, self.head, self.loss,
                             self.lr, self.momentum)


def fit_tables(ctx, jobs, steps: int, tree: GameTree | None = None) -> np.ndarray:
    """``nfsp_fit_tables``: every job's net takes ``steps`` full-batch steps on its seat's rows, one
    workgroup per job (64 per launch), deterministic: a job's result depends on the job alone, and
    ``steps`` split over calls with ``v`` carried gives the bits of one call.  All jobs of a call
    have one hidden width (16, 32, 64 or 128: ``nfsp_fit_tables_h`` where it is not 64).  Returns the
    weighted losses ``[n, 2]``: at the weights before step 1 and at the final weights."""
    tree = tree or GameTree.of(ctx.game)
    for k, j in enumerate(jobs):
        for name, t, numel in (("target", j.target, tree.ndec * 9), ("weight", j.weight, tree.ndec * 3),
                               ("mask", j.mask, tree.ndec * 9)):
            if t is not None and t.numel() != numel:
                raise ValueError(f"fit_tables: job {k}: {name} has {t.numel()} values, expected {numel}")
    n = len(jobs)
    widths = sorted({j.hidden for j in jobs})
    if len(widths) > 1:
        raise ValueError(f"fit_tables: jobs of widths {widths} in one call; one width per call")
    arr = (native.FitJob * max(n, 1))(*[j.spec() for j in jobs])
    out = np.zeros((n, 2))
    if widths in ([], [64]):
        native.check(ctx.L.nfsp_fit_tables(ctx.h, tree.game, arr, n, int(steps), out.ctypes.data_as(native.P)),
                     "nfsp_fit_tables")
    else:
        native.check(ctx.L.nfsp_fit_tables_h(ctx.h, tree.game, widths[0], arr, n, int(steps),
                                             out.ctypes.data_as(native.P)), "nfsp_fit_tables_h")
    return out


def joint_table(ctx, seat0, seat1, tree: GameTree | None = None) -> np.ndarray:
    """The two seats' policies (``Policy`` or table) as one executed table: seat i's rows from
    seat i's."""
    tree = tree or GameTree.of(ctx.game)

    def host(p):
        return policy_table(ctx, p, tree).cpu().numpy() if isinstance(p, Policy) else tree.remap(p)
    t0 = host(seat0)
    t1 = t0 if seat1 is seat0 else host(seat1)
    return np.where((tree.seat == 0)[:, None, None], t0, t1)


def visit_weights(ctx, seat0, seat1, tree: GameTree | None = None) -> np.ndarray:
    """``[ndec, 3]``: the probability that a hand reaches each information set when ``seat0``
    plays seat 0 and ``seat1`` seat 1 (``Policy`` or table each): ``best_response(values=True)``'s
    ``reach`` (chance and the other seat) times the acting seat's own reach
    (``GameTree.own_reach``).  The exact visit distribution of the two policies' self-play: the
    weights under which a net fitted to a table is fitted where the table is played."""
    tree = tree or GameTree.of(ctx.game)
    p0 = seat0 if isinstance(seat0, Policy) else Policy.table(tree.remap(seat0))
    p1 = p0 if seat1 is seat0 else seat1 if isinstance(seat1, Policy) else Policy.table(tree.remap(seat1))
    _, _, reach = best_response(ctx, p0, p1, values=True, tree=tree)
    return reach.cpu().numpy() * tree.own_reach(joint_table(ctx, p0, p1, tree))


def _rms(err, weight):
    den = float(weight.sum())
    return float(np.sqrt((weight * err**2).sum() / den)) if den > 0 else float("nan")


def q_report_from(tree: GameTree, seat: int, beta, q, reach, head, td, linear: bool, gamma: float = 1.0,
                  info=None) -> dict:
    """The BR half of ``memory_report`` for agent ``seat``, pure host arithmetic.

    ``beta``, ``q``, ``reach``: ``best_response(values=True)`` against the opponent the agent
    faces; ``head[ndec, 3, 3]``: the agent's BR net's raw outputs (``head_tables``); ``td``: its TD
    table (a ``MemoryTable`` of kind ``MEM_TD`` or the raw array); ``linear``: whether the head is
    linear (echoed); ``gamma``: the TD table's.  Over the rows where the seat acts, with
    qx = q / reach (the exact expected chips of each legal action where reach > 0: what the Q net is
    to learn) and w = reach / sum reach:

    * ``q_rmse_exact``   sqrt(sum_sets w sum_legal (Q_net - qx)^2 / sum_sets w nlegal);
    * ``greedy_mismatch_share``  the w-share of reached sets where the head's executed action
      (first maximum, an illegal raise becomes call) is not ``beta``'s;
    * ``neg_value_actions``  reached (set, legal action) pairs with qx < 0;
    * ``relu_blind_share``  the w-share of reached sets whose best exact action is not fold and has
      qx <= 0: a ReLU head can at best tie there, and the first maximum folds (reported for a
      linear head too);
    * ``td_pairs`` / ``td_empty_actions``  legal pairs with / without records;
    * ``td_rmse_exact``  the count-weighted RMS of mean_v - qx over pairs with records and
      reach > 0: the data against the truth;
    * ``fit_rmse_td``    the count-weighted RMS of Q_net - mean_v over pairs with records: the net
      against its data;
    * ``mean_bootstrap_share``  sum field 2 x gamma / sum |field 1| over the legal pairs (NaN
      without TD mass);
    * ``linear``, and ``info`` when given.

    RMS values without a pair to average are NaN.  Records stored at an illegal raise are in the
    table but in none of these figures.  Two caveats: under ``QUIRK_ALIAS_RL`` a record's key is its
    hand's LAST s, and under ``QUIRK_ROW0_TARGET`` the net is fitted to one TD value per 128 sampled
    rows; the report states what is stored and what the net holds, whatever the quirks."""
    def host(x):
        return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    beta = host(beta).astype(np.float64).reshape(tree.ndec, 3, 3)
    q = host(q).astype(np.float64).reshape(tree.ndec, 3, 3)
    reach = host(reach).astype(np.float64).reshape(tree.ndec, 3)
    head = host(head).astype(np.float64).reshape(tree.ndec, 3, 3)
    if not isinstance(td, MemoryTable):
        td = MemoryTable(tree, native.MEM_TD, td)
    mine = (tree.seat == seat)[:, None]
    legal = np.ones((tree.ndec, 3, 3), bool)
    legal[~tree.legal, :, 2] = False
    legal &= mine[:, :, None]
    reached = mine & (reach > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        qx = np.where(reached[:, :, None], q / reach[:, :, None], np.nan)
    tot = float(reach[reached].sum())
    w = np.where(reached, reach / tot, 0.0) if tot > 0 else np.zeros_like(reach)
    pair = legal & reached[:, :, None]
    err = np.where(pair, head - np.where(pair, qx, 0.0), 0.0)
    with np.errstate(invalid="ignore"):
        greedy = np.argmax(head, axis=2)                           # first maximum, a NaN is the maximum
    greedy = np.where((greedy == 2) & ~tree.legal[:, None], 1, greedy)
    best = np.argmax(beta, axis=2)
    qbest = np.take_along_axis(np.where(reached[:, :, None], qx, 0.0), best[:, :, None], axis=2)[:, :, 0]
    cnt = np.where(legal, td.counts, 0).astype(np.float64)
    has = cnt > 0
    with np.errstate(invalid="ignore"):
        mv = np.where(has, td.mean_v, 0.0)
    both = has & pair
    f1 = td.raw[..., 1][legal].astype(np.float64)
    f2 = td.raw[..., 2][legal].astype(np.float64)
    mass = float(np.abs(f1).sum())
    out = {
        "q_rmse_exact": _rms(err, w[:, :, None] * pair),
        "greedy_mismatch_share": float((w * (greedy != best))[reached].sum()),
        "neg_value_actions": int((pair & (np.where(pair, qx, 0.0) < 0)).sum()),
        "relu_blind_share": float((w * ((best != 0) & (qbest <= 0)))[reached].sum()),
        "td_pairs": int(has.sum()),
        "td_empty_actions": int((legal & ~has).sum()),
        "td_rmse_exact": _rms(np.where(both, mv - np.where(both, qx, 0.0), 0.0), cnt * both),
        "fit_rmse_td": _rms(np.where(has, head - mv, 0.0), cnt),
        "mean_bootstrap_share": float(f2.sum()) * float(gamma) / mass if mass > 0 else float("nan"),
        "linear": bool(linear)}
    if info is not None:
        out["info"] = info
    return out


class _Solver(native.Handle):
    """What the solvers share: the tree, a device table read to the host, the handle's release."""
    DESTROY = None

    def __init__(self, ctx):
        self.ctx = ctx
        self.tree = GameTree.of(ctx.game)

    def _host_table(self, policy: Policy) -> np.ndarray:
        import torch
        t = native.wrap_device(policy.ptr, self.tree.ndec * 9, torch.float64,
                               torch.device("cuda", torch.cuda.current_device()), self)
        return t.cpu().numpy().reshape(self.tree.ndec, 3, 3).copy()

    def _destroy(self):
        getattr(self.ctx.L, self.DESTROY)(self.h)


class XfpSolver(_Solver):
    """Full-width extensive-form fictitious play on the evaluator's tree (``nfsp_xfp_*``): the
    ideal curve of the algorithm NFSP approximates.  ``cfgs`` is one ``(eta, weight)`` per
    independent run (weight: ``native.XFP_WEIGHT_UNIFORM`` / ``_LINEAR`` or "uniform" /
    "linear"); all runs advance together, one workgroup each.  ``run(n)`` continues them by n
    iterations (with ``gaps=True`` it returns the ``[runs, n]`` array of br0 + br1 of the
    strategy each iteration responded to: at eta = 0 the exploitability of the average so far),
    ``average(k)`` is run k's average strategy as a ``Policy``."""

    WEIGHTS = {"uniform": native.XFP_WEIGHT_UNIFORM, "linear": native.XFP_WEIGHT_LINEAR}
    DESTROY = "nfsp_xfp_destroy"

    def __init__(self, ctx, cfgs=((0.0, native.XFP_WEIGHT_UNIFORM),)):
        super().__init__(ctx)
        self.cfgs = [(float(eta), int(self.WEIGHTS.get(w, w))) for eta, w in cfgs]
        self.n = len(self.cfgs)
        arr = (native.XfpCfg * max(self.n, 1))(*[native.XfpCfg(eta, w, 0) for eta, w in self.cfgs])
        h = native.P()
        native.check(ctx.L.nfsp_xfp_create(ctx.h, arr, self.n, C.byref(h)), "nfsp_xfp_create")
        self.h = h

    def run(self, iters: int, gaps: bool = False):
        out = np.zeros((self.n, max(int(iters), 0))) if gaps else None    # iters < 0: the library refuses
        native.check(self.ctx.L.nfsp_xfp_run(self.h, int(iters), out.ctypes.data_as(native.P) if gaps else None),
                     "nfsp_xfp_run")
        return out if gaps else self

    @property
    def iterations(self) -> int:
        n = native.I64(0)
        native.check(self.ctx.L.nfsp_xfp_iterations(self.h, C.byref(n)), "nfsp_xfp_iterations")
        return n.value

    def average(self, run: int = 0) -> Policy:
        p = native.P()
        native.check(self.ctx.L.nfsp_xfp_average(self.h, int(run), C.byref(p)), "nfsp_xfp_average")
        return Policy(native.POL_TABLE, None, p.value, self)

    def average_table(self, run: int = 0) -> np.ndarray:
        return self._host_table(self.average(run))

    def state(self, run: int = 0) -> tuple:
        """(S, B, W) of a run: the weighted sum of the best responses' realisation plans and
        the last one's, ``[ndec, 3, 3]`` each, and the sum of the weights."""
        S = np.zeros((self.tree.ndec, 3, 3))
        B = np.zeros((self.tree.ndec, 3, 3))
        W = native.F64(0.0)
        native.check(self.ctx.L.nfsp_xfp_state(self.h, int(run), S.ctypes.data_as(native.P),
                                               B.ctypes.data_as(native.P), C.byref(W)), "nfsp_xfp_state")
        return S, B, W.value


class MccfrSolver(_Solver):
    """External-sampling MCCFR on the evaluator's tree (``nfsp_mccfr_*``): the sampled tabular
    yardstick, counted in traversals and terminals visited.  ``cfgs`` is one ``(seed, walkers)``
    per independent run; all runs advance together.  ``run(n)`` continues them by n iterations
    (each one half-iteration of ``walkers`` traversals per seat), ``counts(k)`` is run k's
    (traversals, terminals visited), ``average(k)`` its average strategy as a ``Policy`` and
    ``state(k)`` its int64 fixed-point tables (``native.MCCFR_Q`` per chip / per unit)."""

    DESTROY = "nfsp_mccfr_destroy"

    def __init__(self, ctx, cfgs=((1, 1024),)):
        super().__init__(ctx)
        self.cfgs = [(int(seed) & (2**64 - 1), int(w)) for seed, w in cfgs]
        self.n = len(self.cfgs)
        arr = (native.MccfrCfg * max(self.n, 1))(*[native.MccfrCfg(seed, w, 0) for seed, w in self.cfgs])
        h = native.P()
        native.check(ctx.L.nfsp_mccfr_create(ctx.h, arr, self.n, C.byref(h)), "nfsp_mccfr_create")
        self.h = h

    def run(self, iters: int) -> "MccfrSolver":
        native.check(self.ctx.L.nfsp_mccfr_run(self.h, int(iters)), "nfsp_mccfr_run")
        return self

    @property
    def iterations(self) -> int:
        n = native.I64(0)
        native.check(self.ctx.L.nfsp_mccfr_iterations(self.h, C.byref(n)), "nfsp_mccfr_iterations")
        return n.value

    def counts(self, run: int = 0) -> tuple:
        """(traversals, terminals visited) of a run."""
        out = (native.I64 * 2)()
        native.check(self.ctx.L.nfsp_mccfr_counts(self.h, int(run), out), "nfsp_mccfr_counts")
        return int(out[0]), int(out[1])

    def average(self, run: int = 0) -> Policy:
        p = native.P()
        native.check(self.ctx.L.nfsp_mccfr_average(self.h, int(run), C.byref(p)), "nfsp_mccfr_average")
        return Policy(native.POL_TABLE, None, p.value, self)

    def average_table(self, run: int = 0) -> np.ndarray:
        return self._host_table(self.average(run))

    def state(self, run: int = 0) -> tuple:
        """(R, S) of a run: the regrets and the strategy sums, int64 ``[ndec, 3, 3]`` each."""
        R = np.zeros((self.tree.ndec, 3, 3), np.int64)
        S = np.zeros((self.tree.ndec, 3, 3), np.int64)
        native.check(self.ctx.L.nfsp_mccfr_state(self.h, int(run), R.ctypes.data_as(native.P),
                                                 S.ctypes.data_as(native.P)), "nfsp_mccfr_state")
        return R, S

    @property
    def sampling(self) -> int:
        """0 external sampling, 1 outcome sampling (``nfsp_mccfr_sampling``)."""
        k = native.I32(-1)
        native.check(self.ctx.L.nfsp_mccfr_sampling(self.h, C.byref(k)), "nfsp_mccfr_sampling")
        return k.value


class MccfrOsSolver(MccfrSolver):
    """Outcome-sampling MCCFR on the same handle (``nfsp_mccfr_os_create``): a traversal is one
    sampled hand and one terminal, so ``counts(k)`` is (hands, hands) -- the sampled tabular
    learner counted in the engine's own unit.  ``cfgs`` is one ``(seed, walkers, epsilon)`` per
    independent run, epsilon the exploration rate of the updating seat's own actions
    (``native.MCCFR_OS_EPS_MIN`` .. 1).  Everything else is ``MccfrSolver``'s."""

    def __init__(self, ctx, cfgs=((1, 1024, 0.6),)):
        _Solver.__init__(self, ctx)
        self.cfgs = [(int(seed) & (2**64 - 1), int(w), float(eps)) for seed, w, eps in cfgs]
        self.n = len(self.cfgs)
        arr = (native.MccfrOsCfg * max(self.n, 1))(*[native.MccfrOsCfg(seed, w, 0, eps) for seed, w, eps in self.cfgs])
        h = native.P()
        native.check(ctx.L.nfsp_mccfr_os_create(ctx.h, arr, self.n, C.byref(h)), "nfsp_mccfr_os_create")
        self.h = h


class MccfrVrSolver(MccfrOsSolver):
    """Baseline-corrected outcome sampling, VR-MCCFR, on the same handle (``nfsp_mccfr_vr_create``):
    outcome sampling's paths, hands and ``cfgs``, with the values on the way back up corrected by a
    learned baseline at every decision.  ``baseline(k)`` is run k's (Bs, Bn), the int64 sums
    (``native.MCCFR_Q`` per chip) and counts ``[ndec, 3, 3]`` in the acting seat's perspective,
    ``set_baseline(k, Bs, Bn)`` replaces them, and ``baseline_table(k)`` is the clamped f64 table
    the next half-iteration uses.  Everything else is ``MccfrOsSolver``'s."""

    def __init__(self, ctx, cfgs=((1, 1024, 0.6),)):
        _Solver.__init__(self, ctx)
        self.cfgs = [(int(seed) & (2**64 - 1), int(w), float(eps)) for seed, w, eps in cfgs]
        self.n = len(self.cfgs)
        arr = (native.MccfrVrCfg * max(self.n, 1))(*[native.MccfrVrCfg(seed, w, 0, eps) for seed, w, eps in self.cfgs])
        h = native.P()
        native.check(ctx.L.nfsp_mccfr_vr_create(ctx.h, arr, self.n, C.byref(h)), "nfsp_mccfr_vr_create")
        self.h = h

    def baseline(self, run: int = 0) -> tuple:
        Bs = np.zeros((self.tree.ndec, 3, 3), np.int64)
        Bn = np.zeros((self.tree.ndec, 3, 3), np.int64)
        native.check(self.ctx.L.nfsp_mccfr_baseline(self.h, int(run), Bs.ctypes.data_as(native.P),
                                                    Bn.ctypes.data_as(native.P)), "nfsp_mccfr_baseline")
        return Bs, Bn

    def set_baseline(self, run: int, Bs, Bn) -> "MccfrVrSolver":
        shape = (self.tree.ndec, 3, 3)
        Bs, Bn = (np.ascontiguousarray(x, np.int64) for x in (Bs, Bn))
        if Bs.shape != shape or Bn.shape != shape:
            raise ValueError("Bs and Bn must be [ndec, 3, 3]")
        native.check(self.ctx.L.nfsp_mccfr_set_baseline(self.h, int(run), Bs.ctypes.data_as(native.P),
                                                        Bn.ctypes.data_as(native.P)), "nfsp_mccfr_set_baseline")
        return self

    def baseline_table(self, run: int = 0) -> np.ndarray:
        """B = clamp(Bs / (Bn Q), -P, P), 0 where Bn is 0, P the game's max|pay| (include/nfsp.h)."""
        Bs, Bn = self.baseline(run)
        P = float(np.abs(self.tree.pay).max())
        den = np.where(Bn > 0, Bn, 1).astype(np.float64) * float(native.MCCFR_Q)
        return np.where(Bn > 0, np.clip(Bs.astype(np.float64) / den, -P, P), 0.0)


class MccfrXSolver(MccfrVrSolver):
    """Regret matching+ and linear averaging on any of the three sampling kinds
    (``nfsp_mccfr_x_create``).  ``sampling`` (0 external, 1 outcome, 2 outcome with baselines, or
    "es" / "os" / "vr") is the handle's; ``cfgs`` is one ``(seed, walkers, epsilon, regret,
    average)`` per run, epsilon 0.0 under external sampling, regret ``native.MCCFR_REGRET_*`` or
    "plain" / "plus", average ``native.MCCFR_AVG_*`` or "uniform" / "linear".  ``rule(k)`` is run
    k's (regret, average); ``average(k)`` the average its cfg names and ``average(k, which)``
    either, both kept on the same sample paths; ``weighted(k)`` the f64 linear sum Sw.  The
    baseline methods serve sampling 2 and are refused otherwise.  Everything else is
    ``MccfrSolver``'s."""

    SAMPLINGS = {"es": 0, "os": 1, "vr": 2}
    REGRETS = {"plain": native.MCCFR_REGRET_PLAIN, "plus": native.MCCFR_REGRET_PLUS}
    AVERAGES = {"uniform": native.MCCFR_AVG_UNIFORM, "linear": native.MCCFR_AVG_LINEAR}

    def __init__(self, ctx, cfgs=((1, 1024, 0.6, "plus", "linear"),), sampling=2):
        _Solver.__init__(self, ctx)
        samp = int(self.SAMPLINGS.get(sampling, sampling))
        self.cfgs = [(int(seed) & (2**64 - 1), int(w), float(eps), int(self.REGRETS.get(reg, reg)),
                      int(self.AVERAGES.get(avg, avg))) for seed, w, eps, reg, avg in cfgs]
        self.n = len(self.cfgs)
        arr = (native.MccfrXCfg * max(self.n, 1))(*[native.MccfrXCfg(seed, w, samp, eps, reg, avg)
                                                    for seed, w, eps, reg, avg in self.cfgs])
        h = native.P()
        native.check(ctx.L.nfsp_mccfr_x_create(ctx.h, arr, self.n, C.byref(h)), "nfsp_mccfr_x_create")
        self.h = h

    def rule(self, run: int = 0) -> tuple:
        """(regret, average) of a run."""
        out = (native.I32 * 2)()
        native.check(self.ctx.L.nfsp_mccfr_rule(self.h, int(run), out), "nfsp_mccfr_rule")
        return int(out[0]), int(out[1])

    def average(self, run: int = 0, which=None) -> Policy:
        if which is None:
            return MccfrSolver.average(self, run)
        p = native.P()
        native.check(self.ctx.L.nfsp_mccfr_average_of(self.h, int(run), int(self.AVERAGES.get(which, which)),
                                                      C.byref(p)), "nfsp_mccfr_average_of")
        return Policy(native.POL_TABLE, None, p.value, self)

    def average_table(self, run: int = 0, which=None) -> np.ndarray:
        return self._host_table(self.average(run, which))

    def weighted(self, run: int = 0) -> np.ndarray:
        """Sw of a run: the linearly weighted strategy sum, f64 ``[ndec, 3, 3]``."""
        Sw = np.zeros((self.tree.ndec, 3, 3))
        native.check(self.ctx.L.nfsp_mccfr_weighted(self.h, int(run), Sw.ctypes.data_as(native.P)),
                     "nfsp_mccfr_weighted")
        return Sw


class MccfrNetSolver(MccfrXSolver):
    """Regret nets on the MCCFR handle (``nfsp_mccfr_net_create``): sampled regression CFR whose
    walkers read the sigma of two 30-64-3 nets per run, each fitted to its seat's rows of R after the
    seat's half-iteration.  ``sampling`` is ``MccfrXSolver``'s; ``cfgs`` is one ``(seed, walkers,
    epsilon, regret, average, target, fit_steps, loss, lr, momentum)`` per run -- the first five as
    ``MccfrXSolver``'s, target ``native.MCCFR_NET_TARGET_*`` or "avg" / "rowmax", loss "mse" / "huber"
    or ``native.FIT_*``; ``init_seeds`` is one seed per run: the nets are
    ``glorot_net(RandomState(seed), hidden)``, seat 0's first and then seat 1's -- or ``init_nets``,
    two packed nets per run, whose common width (``net_width``) is the handle's
    (``nfsp_mccfr_net_create_h``; one width per handle, 16, 32, 64 or 128, read back as ``.hidden``).  ``sigma_table(k)`` is the
    sigma the walkers read ("net") or regret matching on R ("table"), ``head(k)`` the nets' heads z,
    ``net(k, seat)`` a seat's (w, v), ``set_net`` writes them between runs, ``fit_loss(k)`` the
    ``[seat, before / after]`` losses of the last fits, ``current(k)`` the nets' sigma as a ``Policy``
    and ``sigma_tv(k)`` the per-seat mean total variation between the two sigma tables.  Everything
    else is ``MccfrXSolver``'s."""

    TARGETS = {"avg": native.MCCFR_NET_TARGET_AVG, "rowmax": native.MCCFR_NET_TARGET_ROWMAX}

    def __init__(self, ctx, cfgs=((1, 1024, 0.0, "plain", "uniform", "avg", 32, "mse", 0.5, 0.9),), sampling=0,
                 init_seeds=None, hidden: int = 64, init_nets=None):
        import torch
        _Solver.__init__(self, ctx)
        samp = int(self.SAMPLINGS.get(sampling, sampling))
        self.cfgs = [(int(seed) & (2**64 - 1), int(w), float(eps), int(self.REGRETS.get(reg, reg)),
                      int(self.AVERAGES.get(avg, avg)), int(self.TARGETS.get(tgt, tgt)), int(steps),
                      int(FIT_LOSSES.get(loss, loss)), float(lr), float(mu))
                     for seed, w, eps, reg, avg, tgt, steps, loss, lr, mu in cfgs]
        self.n = len(self.cfgs)
        self.init_seeds = [int(s) for s in (range(1, self.n + 1) if init_seeds is None else init_seeds)]
        if len(self.init_seeds) != self.n:
            raise ValueError("MccfrNetSolver: one init seed per run")
        nets = []
        if init_nets is not None:
            nets = [np.ascontiguousarray(w, np.float32).reshape(-1) for w in init_nets]
            if len(nets) != 2 * self.n:
                raise ValueError("MccfrNetSolver: init_nets holds two nets per run, seat 0's first")
            hidden = _one_width(nets, "MccfrNetSolver")
        else:
            native.net_params(int(hidden))
            for s in self.init_seeds:
                rng = np.random.RandomState(s)
                nets += [glorot_net(rng, int(hidden)), glorot_net(rng, int(hidden))]
        self._np = native.net_params(int(hidden))
        w0 = torch.as_tensor(np.stack(nets) if nets else np.zeros((0, self._np), np.float32), device="cuda")
        arr = (native.MccfrNetCfg * max(self.n, 1))(*[native.MccfrNetCfg(c[0], c[1], samp, *c[2:], 0) for c in self.cfgs])
        ptrs = (native.P * max(2 * self.n, 1))(*[w0[k].data_ptr() for k in range(2 * self.n)])
        h = native.P()
        if init_nets is None and int(hidden) == 64:
            native.check(ctx.L.nfsp_mccfr_net_create(ctx.h, arr, self.n, ptrs, C.byref(h)), "nfsp_mccfr_net_create")
        else:
            native.check(ctx.L.nfsp_mccfr_net_create_h(ctx.h, int(hidden), arr, self.n, ptrs, C.byref(h)),
                         "nfsp_mccfr_net_create_h")
        self.h = h

    @property
    def hidden(self) -> int:
        """the nets' hidden width (``nfsp_mccfr_net_hidden``)"""
        out = native.I32()
        native.check(self.ctx.L.nfsp_mccfr_net_hidden(self.h, C.byref(out)), "nfsp_mccfr_net_hidden")
        return int(out.value)

    def _tables(self, run):
        sg, tab, z = native.P(), native.P(), native.P()
        native.check(self.ctx.L.nfsp_mccfr_net_tables(self.h, int(run), C.byref(sg), C.byref(tab), C.byref(z)),
                     "nfsp_mccfr_net_tables")
        return sg.value, tab.value, z.value

    def _view(self, addr, numel, dtype):
        import torch
        return native.wrap_device(addr, numel, dtype, torch.device("cuda", torch.cuda.current_device()), self)

    def sigma_table(self, run: int = 0, which: str = "net") -> np.ndarray:
        """f64 ``[ndec, 3, 3]``: the nets' sigma ("net", what the walkers read) or regret matching on R ("table")."""
        import torch
        if which not in ("net", "table"):
            raise ValueError('which must be "net" or "table"')
        addr = self._tables(run)[which == "table"]
        return self._view(addr, self.tree.ndec * 9, torch.float64).cpu().numpy().reshape(self.tree.ndec, 3, 3).copy()

    def head(self, run: int = 0) -> np.ndarray:
        """f32 ``[ndec, 3, 3]``: the heads z of the acting seat's net at every row."""
        import torch
        return self._view(self._tables(run)[2], self.tree.ndec * 9, torch.float32).cpu().numpy().reshape(
            self.tree.ndec, 3, 3).copy()

    def _net(self, run, seat):
        import torch
        w, v = native.P(), native.P()
        native.check(self.ctx.L.nfsp_mccfr_net_weights(self.h, int(run), int(seat), C.byref(w), C.byref(v)),
                     "nfsp_mccfr_net_weights")
        return self._view(w.value, self._np, torch.float32), self._view(v.value, self._np, torch.float32)

    def net(self, run: int = 0, seat: int = 0) -> tuple:
        """(w, v) of a seat's net, f32 ``[NP]`` each, copied to the host."""
        w, v = self._net(run, seat)
        return w.cpu().numpy().copy(), v.cpu().numpy().copy()

    def set_net(self, run: int, seat: int, w, v=None) -> "MccfrNetSolver":
        """Writes a seat's net (and with ``v`` its momentum state) between runs; z and sigma follow at
        the handle's next apply."""
        import torch
        dw, dv = self._net(run, seat)
        for dst, src in ((dw, w), (dv, v)):
            if src is None:
                continue
            src = np.ascontiguousarray(src, np.float32)
            if src.shape != (self._np,):
                raise ValueError(f"a net of this handle has {self._np} float32 values")
            if not np.isfinite(src).all():
                raise ValueError("set_net: values that are not finite")
            dst.copy_(torch.as_tensor(src, device=dst.device))
        torch.cuda.current_stream().synchronize()
        return self

    def fit_loss(self, run: int = 0) -> np.ndarray:
        """``[seat, 2]``: the loss of the seat's last fit before its first step and at its final weights."""
        out = np.zeros((2, 2))
        native.check(self.ctx.L.nfsp_mccfr_net_loss(self.h, int(run), out.ctypes.data_as(C.POINTER(native.F64))),
                     "nfsp_mccfr_net_loss")
        return out

    def current(self, run: int = 0) -> Policy:
        return Policy(native.POL_TABLE, None, self._tables(run)[0], self)

    def sigma_tv(self, run: int = 0) -> np.ndarray:
        """Per seat, the mean over the seat's (d, r) rows of half the L1 distance between the nets' sigma and
        regret matching on R."""
        tv = 0.5 * np.abs(self.sigma_table(run, "net") - self.sigma_table(run, "table")).sum(axis=2)
        return np.array([tv[self.tree.seat == s].mean() for s in (0, 1)])


def mccfr_timings(solver, enable=None):
    """``nfsp_mccfr_set_timing`` / ``_get_timings`` of any MCCFR solver: with ``enable`` given turns the
    handle's event timing on or off (and zeroes its sums); returns (ms in walks, ms in applies, iterations)."""
    if enable is not None:
        native.check(solver.ctx.L.nfsp_mccfr_set_timing(solver.h, int(bool(enable))), "nfsp_mccfr_set_timing")
    ms, it = (native.F64 * 2)(), native.I64(0)
    native.check(solver.ctx.L.nfsp_mccfr_get_timings(solver.h, ms, C.byref(it)), "nfsp_mccfr_get_timings")
    return float(ms[0]), float(ms[1]), int(it.value)


class CfrSolver(_Solver):
    """CFR+ on the evaluator's tree (``nfsp_cfr_*``): ``run(n)`` continues the run by n
    iterations, ``average()`` is the linearly weighted average strategy as a ``Policy``."""

    DESTROY = "nfsp_cfr_destroy"

    def __init__(self, ctx):
        super().__init__(ctx)
        h = native.P()
        native.check(ctx.L.nfsp_cfr_create(ctx.h, C.byref(h)), "nfsp_cfr_create")
        self.h = h

    def run(self, iters: int) -> "CfrSolver":
        native.check(self.ctx.L.nfsp_cfr_run(self.h, int(iters)), "nfsp_cfr_run")
        return self

    @property
    def iterations(self) -> int:
        n = native.I64(0)
        native.check(self.ctx.L.nfsp_cfr_iterations(self.h, C.byref(n)), "nfsp_cfr_iterations")
        return n.value

    def average(self) -> Policy:
        p = native.P()
        native.check(self.ctx.L.nfsp_cfr_average(self.h, C.byref(p)), "nfsp_cfr_average")
        return Policy(native.POL_TABLE, None, p.value, self)

    def average_table(self) -> np.ndarray:
        return self._host_table(self.average())

    def state(self) -> tuple:
        """(R, S): the regrets and the strategy sums, ``[ndec, 3, 3]`` each."""
        R = np.zeros((self.tree.ndec, 3, 3))
        S = np.zeros((self.tree.ndec, 3, 3))
        native.check(self.ctx.L.nfsp_cfr_state(self.h, R.ctypes.data_as(native.P), S.ctypes.data_as(native.P)),
                     "nfsp_cfr_state")
        return R, S

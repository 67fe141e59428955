"""Batched self-play: the fused hot path (``nfsp_engine_*`` / ``nfsp_rollout``).

``SelfPlayEngine`` owns one ``nfsp_engine`` (n_lanes hands in flight, both agents'
networks and memories in HBM).  ``step()`` = one hand per lane through the fused
rollout kernel + the deterministic insert + the learner at the reference cadence
(one update_strategy per ``inserts_per_update`` RL inserts of an agent,
agent/agent.py:153).  Configuration keys mirror config.ini:

    reference (config C1)   n_lanes=1,   rl_capacity=40_000,  sl_capacity=40_000
    C2                      n_lanes=65_536
    C3                      n_lanes=1_048_576, rl_capacity=200_000, sl_capacity=2_000_000
                            (slices=16: the 1M lanes advance in 16 slices of 65,536, the
                            learner consuming each slice before the next acts)
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import checkpoint, diagnostics, evaluation, native
from .evaluation import exploitability, exploitability_batch, glorot_net  # noqa: F401  (engine.exploitability is public API)
from .native import NET_AR, NET_BR, NET_TARGET, NP

PRESETS = {
    "reference": dict(n_lanes=1, rl_capacity=40_000, sl_capacity=40_000),
    "c2": dict(n_lanes=65_536, rl_capacity=40_000, sl_capacity=40_000),
    "c3": dict(n_lanes=1_048_576, rl_capacity=200_000, sl_capacity=2_000_000),
}


def make_cfg(L, **cfg) -> native.EngineCfg:
    c = native.EngineCfg()
    native.check(L.nfsp_engine_default_cfg(C.byref(c)), "nfsp_engine_default_cfg")
    for k, v in cfg.items():
        if not hasattr(c, k):
            raise KeyError(k)
        setattr(c, k, v)
    return c


def _timings(obj, fn) -> dict:
    ms = (native.F64 * len(obj.KERNELS))()
    n = (native.I64 * len(obj.KERNELS))()
    native.check(getattr(obj.L, fn)(obj.h, ms, n), "get_timings")
    return {k: (ms[i], n[i]) for i, k in enumerate(obj.KERNELS)}


def _count_tables(obj, dev, fn, R, kind, *head) -> list:
    """``[(evaluation.MemoryTable of ``kind``, [info of agent 0, of agent 1])]`` of R engines: one
    launch of ``fn`` (nfsp_{engine,group}_{memory,td}_table[s]), ``head`` its arguments before the output."""
    tree = evaluation.GameTree.of(obj.ctx.game)
    out = torch.empty((R, tree.ndec, 3, 3, 3), dtype=torch.int64, device=dev)
    info = (native.MemtabInfo * (2 * R))()
    native.check(getattr(obj.L, fn)(obj.h, *head, native.P(out.data_ptr()), info), fn)
    raw = out.cpu().numpy()
    return [(evaluation.MemoryTable(tree, kind, raw[r]), [info[2 * r].to_dict(), info[2 * r + 1].to_dict()])
            for r in range(R)]


class SelfPlayEngine(native.Handle):
    def __init__(self, ctx: native.Context | None = None, init_seed: int = 0, game: int = native.GAME_LEDUC,
                 _borrow=None, **cfg):
        self.ctx = ctx if ctx is not None else native.Context(1, game=game)
        L = self.ctx.L
        self.L = L
        self.dev = torch.device("cuda", torch.cuda.current_device())
        if _borrow is not None:            # a replica of an EngineGroup: (group, handle, cfg)
            self._owner, self.h, self.cfg = _borrow
            self._init_weights(init_seed)
            return
        self._owner = None
        c = make_cfg(L, **cfg)
        self.cfg = c
        h = native.P()
        native.check(L.nfsp_engine_create(self.ctx.h, C.byref(c), C.byref(h)), "nfsp_engine_create")
        self.h = h
        self._init_weights(init_seed)

    def _init_weights(self, init_seed):
        # initial weights in the reference's construction order: per agent AR, BR, target
        # (the target is drawn, then overwritten with BR: agent/agent.py:67-72)
        rng = np.random.RandomState(init_seed)
        for a in (0, 1):
            ar = glorot_net(rng)
            br = glorot_net(rng)
            glorot_net(rng)
            self.set_weights(a, NET_AR, ar)
            self.set_weights(a, NET_BR, br)
            self.set_weights(a, NET_TARGET, br)

    # -- weights ------------------------------------------------------------------
    def _wptr(self, agent, net):
        p = native.P()
        native.check(self.L.nfsp_engine_weights(self.h, agent, net, C.byref(p)), "weights")
        return p.value

    def weights_tensor(self, agent, net) -> torch.Tensor:
        """A torch view (no copy) of the device weights of (agent, net)."""
        return native.wrap_device(self._wptr(agent, net), NP, torch.float32, self.dev, self)

    def get_weights(self, agent, net) -> np.ndarray:
        return self.weights_tensor(agent, net).cpu().numpy().copy()

    def set_weights(self, agent, net, flat):
        self.weights_tensor(agent, net).copy_(torch.as_tensor(np.asarray(flat, np.float32)))

    # -- hot path -----------------------------------------------------------------
    def rollout(self):
        native.check(self.L.nfsp_rollout(self.h), "nfsp_rollout")

    def rollout_with(self, w_flat: np.ndarray, eps):
        """Test hook (nfsp_rollout_with): the next slice's rollout acting with the given nets
        ([2][3][NP] flat, as weights_tensor packs them) and epsilons."""
        w = torch.as_tensor(np.asarray(w_flat, np.float32).reshape(-1), device=self.dev)
        assert w.numel() == 6 * NP
        e = (C.c_double * 2)(float(eps[0]), float(eps[1]))
        native.check(self.L.nfsp_rollout_with(self.h, C.c_void_p(w.data_ptr()), e), "nfsp_rollout_with")
        torch.cuda.synchronize(self.dev)       # w is a temporary

    def update(self):
        native.check(self.L.nfsp_engine_update(self.h), "nfsp_engine_update")

    def step(self):
        """One hand on every lane: ``cfg.slices`` x (rollout of the next slice + update)."""
        native.check(self.L.nfsp_engine_step(self.h), "nfsp_engine_step")

    def stats(self) -> dict:
        s = native.EngineStats()
        native.check(self.L.nfsp_engine_get_stats(self.h, C.byref(s)), "nfsp_engine_get_stats")
        return s.to_dict()

    KERNELS = ("k_rollout", "k_scan", "k_commit", "learner", "learner_prep", "k_br_targets",
               "k_chain3_br", "k_chain3_ar", "br_stream_a0", "br_stream_a1", "ar_exchange")

    def set_timing(self, on=True):
        native.check(self.L.nfsp_engine_set_timing(self.h, int(bool(on))), "set_timing")

    def timings(self) -> dict:
        """{kernel: (total ms, launches)} since the last call (HIP events, ctx stream)."""
        return _timings(self, "nfsp_engine_get_timings")

    # -- inspection (tests) -------------------------------------------------------
    def memories(self, agent):
        rl, sl = native.Records(), native.Records()
        cap = native.I64()
        px, pa, pp = native.P(), native.P(), native.P()
        native.check(self.L.nfsp_engine_memories(self.h, agent, C.byref(rl), C.byref(cap),
                                                  C.byref(sl), C.byref(px), C.byref(pa),
                                                  C.byref(pp)), "nfsp_engine_memories")
        n = cap.value
        d = self.dev
        out = dict(
            log_cap=n,
            rl_s=native.wrap_device(rl.s, n * 30, torch.float32, d, self).view(n, 30),
            rl_a=native.wrap_device(rl.a, n * 3, torch.float32, d, self).view(n, 3),
            rl_r=native.wrap_device(rl.r, n, torch.float32, d, self),
            rl_s2=native.wrap_device(rl.s2, n * 30, torch.float32, d, self).view(n, 30),
            rl_t=native.wrap_device(rl.t, n, torch.uint8, d, self),
            sl_s=native.wrap_device(sl.s, sl.cap * 30, torch.float32, d, self).view(sl.cap, 30),
            sl_a=native.wrap_device(sl.a, sl.cap * 3, torch.float32, d, self).view(sl.cap, 3),
        )
        pc = 4 * self.slice_lanes
        out["pend_x"] = native.wrap_device(px.value, pc, torch.int32, d, self)
        out["pend_a"] = native.wrap_device(pa.value, pc * 3, torch.float32, d, self).view(pc, 3)
        out["pend_pos"] = native.wrap_device(pp.value, pc, torch.int64, d, self)
        return out

    def last_update(self, agent, role):
        rows, perms = native.P(), native.P()
        native.check(self.L.nfsp_engine_last_update(self.h, agent, role, C.byref(rows),
                                                     C.byref(perms)), "last_update")
        B, E = self.cfg.batch, self.cfg.epochs
        return (native.wrap_device(rows.value, B, torch.int64, self.dev).cpu().numpy(),
                native.wrap_device(perms.value, E * B, torch.int32, self.dev).view(E, B).cpu().numpy())

    @property
    def slice_lanes(self) -> int:
        """Lanes per rollout (cfg.slices: n_lanes / slices)."""
        return self.cfg.n_lanes // self.cfg.slices

    def last_slice(self) -> tuple:
        """(global id of the first lane, hand index g) of the last rollout: rollout k plays
        slice k % slices with the lanes' hand index k // slices (include/nfsp.h cfg.slices)."""
        k = self.stats()["rollouts"] - 1
        return (k % self.cfg.slices) * self.slice_lanes, k // self.cfg.slices

    def lane_counts(self) -> np.ndarray:
        """[n_lanes / slices, 4] (RL agent 0, RL agent 1, SL agent 0, SL agent 1) records of each
        lane's hand in the last rollout (its slice's lanes; nfsp_engine_lane_counts;
        synchronises)."""
        p = native.P()
        native.check(self.L.nfsp_engine_lane_counts(self.h, C.byref(p)), "lane_counts")
        torch.cuda.synchronize(self.dev)
        c = native.wrap_device(p.value, self.slice_lanes, torch.int32, self.dev).cpu().numpy()
        c = c.astype(np.int64) & 0xFFFF
        return np.stack([(c >> (4 * k)) & 15 for k in range(4)], axis=1)

    def snapshot(self, parity: int):
        """(acting nets [2][3][NP] flat, (eps0, eps1)) of snapshot `parity` (cfg.slice_lag 2,
        nfsp_engine_snapshot): after a pipelined step of K slices, parity (K - 1) & 1 is what
        the last slice acted with."""
        p = native.P()
        eps = (C.c_double * 2)()
        native.check(self.L.nfsp_engine_snapshot(self.h, int(parity), C.byref(p), eps), "snapshot")
        torch.cuda.synchronize(self.dev)
        w = native.wrap_device(p.value, 6 * NP, torch.float32, self.dev, self).cpu().numpy().copy()
        return w, (eps[0], eps[1])

    def set_exchange(self, every: int, scale: float, comm=None, fn=None):
        """The cross-shard exchange of the AR nets (nfsp_engine_set_exchange): after every
        ``every``-th learner call (slice), W_AR = W0 + (sum over shards of W_AR - W0) * scale on
        the AR chain stream, by the RCCL communicator ``comm`` or the host callback ``fn``
        (a ``native.EXCHANGE_FN``; kept alive here).  W0 = the AR nets now.  every 0: off."""
        self._xchg_fn = fn
        native.check(self.L.nfsp_engine_set_exchange(self.h, int(every), float(scale), comm, fn, None),
                     "nfsp_engine_set_exchange")

    def exchanges(self) -> int:
        n = native.I64()
        native.check(self.L.nfsp_engine_exchanges(self.h, C.byref(n)), "nfsp_engine_exchanges")
        return n.value

    def set_update_limit(self, max_updates: int):
        """Test hook (nfsp_engine_set_update_limit): the chains run only a prefix of each
        learner call's updates."""
        native.check(self.L.nfsp_engine_set_update_limit(self.h, int(max_updates)), "set_update_limit")

    loss_log = False

    def set_loss_log(self, on=True):
        native.check(self.L.nfsp_engine_set_loss_log(self.h, int(bool(on))), "set_loss_log")
        self.loss_log = bool(on)

    def losses(self) -> dict:
        """Keras epoch losses of the last learner call (nfsp_engine_losses), keyed like the
        reference's TensorBoard log dirs (agent/agent.py:84-88): Player{a}rl = BR, Player{a}sl = AR."""
        out = (C.c_double * 8)()
        native.check(self.L.nfsp_engine_losses(self.h, out), "nfsp_engine_losses")
        d = {}
        for a in (0, 1):
            for n, tag in ((0, "sl"), (1, "rl")):
                d[f"Player{a}{tag}/loss_mean"] = out[(2 * a + n) * 2]
                d[f"Player{a}{tag}/loss_last"] = out[(2 * a + n) * 2 + 1]
        return d

    def exploitability(self, mode: int = 0) -> dict:
        """Exact exploitability of the two agents' current AR nets (nfsp_exploitability):
        mode 0 = softmax mixed strategies, 1 = the argmax the env executes."""
        return exploitability(self.ctx, self._wptr(0, NET_AR), self._wptr(1, NET_AR), mode)

    def policy(self, agent: int, net: int = NET_AR, mode: int = 0):
        """An ``evaluation.Policy`` reading this engine's weights in place: the AR net as its
        softmax / argmax, or the BR net played greedily (the head kind from ``cfg.quirks``)."""
        if net == NET_AR:
            return evaluation.Policy.ar(self._wptr(agent, NET_AR), mode, owner=self)
        return evaluation.Policy.br(self._wptr(agent, net), bool(self.cfg.quirks & native.EXT_LINEAR_Q), owner=self)

    def br_gap(self, ar_mode: int = 0, eta: float | None = None) -> list:
        """How far each agent's learned best response is from a true one (kuhn_diag's br_gap,
        exact and on the device).  Per agent i (= seat i): ``br_exact``, the best-response value
        against the other seat's AR policy; ``br_learned``, the value of i's greedy BR net
        against it; ``gap`` = their difference (>= 0).  With ``eta`` the opponent is the per-hand
        mixture eta x greedy BR + (1 - eta) x AR it plays in self-play (``evaluation.mix``):
        kuhn_diag's ``anticip``."""
        return diagnostics.br_gaps(self.ctx, [self], ar_mode, eta)[0]

    def best_response_table(self, eta: float | None = None, values: bool = False):
        """The exact best responses behind ``br_gap``'s ``br_exact``, as a strategy
        (``evaluation.best_response``): one joint one-hot table ``[ndec, 3, 3]`` (a float64
        device tensor) whose rows where seat i acts are seat i's best response against the other
        agent's AR policy -- with ``eta`` against its per-hand mixture, built as ``br_gap(eta=)``
        builds it.  Compare it row by row with the greedy BR net's table
        (``evaluation.policy_table(ctx, engine.policy(i, NET_BR))``) to see where the learned
        best response deviates; with ``values`` returns ``(beta, q, reach)``, the exact action
        values there."""
        return diagnostics.best_response_table(self, eta, values)

    # -- tables that act ---------------------------------------------------
    def set_act_table(self, agent: int, role: int, rows):
        """Slot (agent, role) -- role ``NET_AR`` or ``NET_BR`` -- acts with the table ``rows``
        (float32 ``[ndec, 3, 3]`` over ``GameTree``'s rows, ``evaluation.act_rows`` of a policy
        table; array or tensor) instead of its net, ``None``: the net acts again
        (nfsp_engine_set_act_table; step boundaries only).  A row is the vector the net would have
        output: everything downstream of the forward is unchanged.  The engine keeps a copy."""
        if self._owner is not None:
            raise native.NativeError("set_act_table: a replica of an EngineGroup (EngineGroup.set_act_table)")
        t = _act_rows_dev(self, rows)
        native.check(self.L.nfsp_engine_set_act_table(self.h, int(agent), int(role), native.ptr(t)),
                     "nfsp_engine_set_act_table")

    def act_table(self, agent: int, role: int):
        """``(rows, misses)`` of slot (agent, role) (nfsp_engine_get_act_table): a float32 device
        copy ``[ndec, 3, 3]`` of the installed table, ``None`` when the net acts, and the lookups
        that found no information set since it was installed (0 with a complete table)."""
        p, m = native.P(), native.I64()
        native.check(self.L.nfsp_engine_get_act_table(self.h, int(agent), int(role), C.byref(p), C.byref(m)),
                     "nfsp_engine_get_act_table")
        if not p.value:
            return None, m.value
        n = evaluation.GameTree.of(self.ctx.game).ndec * 9
        return native.wrap_device(p.value, n, torch.float32, self.dev, self).view(-1, 3, 3).clone(), m.value

    def clear_act_tables(self):
        """Every slot acts with its net again."""
        for a in (0, 1):
            for role in (NET_AR, NET_BR):
                self._set_act_table(a, role, None)

    def _set_act_table(self, agent, role, rows):
        if self._owner is not None:
            self._owner.set_act_table(self._owner.replicas.index(self), agent, role, rows)
        else:
            self.set_act_table(agent, role, rows)

    def acting_policy(self, agent: int, role: int, ar_mode: int | None = None, tree=None) -> np.ndarray:
        """What slot (agent, role) executes when it acts, a float64 table ``[ndec, 3, 3]``: its
        installed table if it has one, else its net.  The AR role under ``ar_mode`` 0 is sampled
        (``EXT_SAMPLE_AR``: action 0 with probability y0, 1 with y1, else 2, so a table's rows
        are taken as they stand, clipped to [0, 1]), under 1 its argmax; the BR role is greedy.
        ``ar_mode`` defaults to what the rollout does under ``cfg.quirks``."""
        return diagnostics.acting_policy(self, agent, role, ar_mode, tree)

    def install_oracle_br(self, eta: float | None = None, ar_mode: int | None = None):
        """Oracle-BR self-play (sampled FSP): both agents' BR role acts with the exact best
        response (``evaluation.best_response``, one-hot rows) to the other seat's acting average
        policy as it is now -- ``acting_policy`` of its AR role, ``ar_mode`` defaulting to the
        executed one.  With ``eta`` the opponent is its per-hand mixture eta x BR + (1 - eta) x AR
        (``evaluation.mix``), the BR part being its installed BR table if it has one, else its
        greedy BR net.  Call it before every step to refresh; ``clear_act_tables`` undoes it.
        The BR chains still train on M_RL.  Returns the installed joint table (float64, device)."""
        beta = diagnostics.oracle_br(self, eta, ar_mode)
        rows = evaluation.act_rows(beta)
        for a in (0, 1):
            self._set_act_table(a, NET_BR, rows)
        return beta

    # -- the memories as tables ------------------------------------------
    def memory_table(self, kind: int):
        """``(evaluation.MemoryTable, [info of agent 0, of agent 1])`` of M_SL
        (``native.MEM_SL``) or M_RL (``native.MEM_RL``), both agents in one launch on the packed
        records where they lie (nfsp_engine_memory_table; step boundaries only)."""
        return _count_tables(self, self.dev, "nfsp_engine_memory_table", 1, kind, int(kind))[0]

    def memory_report(self) -> dict:
        """What the memories hold against what the nets make of them, all exact:
        ``exploitability_ar`` (the AR nets, as ``exploitability()``), ``exploitability_sl_argmax``
        / ``_sl_mass`` (M_SL's two tables, ``MemoryTable.policy``: sampling and BR quality without
        function approximation), ``fit_gap_*`` = the nets' minus the tables' (what the 64-unit net
        costs), ``sl_empty_sets`` (information sets without an M_SL record), ``rl_empty_actions``
        ((information set, legal action) pairs without an M_RL record), ``ar_mass_l1`` (the mean
        L1 distance between the AR nets' executed policy and the "mass" table, weighted by the
        records per set) and both calls' infos per agent."""
        sl, si = self.memory_table(native.MEM_SL)
        rl, ri = self.memory_table(native.MEM_RL)
        return diagnostics.memory_reports(self.ctx, [self], [sl], [rl], [(si, ri)])[0]

    def td_table(self):
        """``(evaluation.MemoryTable of kind native.MEM_TD, [info of agent 0, of agent 1])``: the TD
        values r + gamma max Q_target(s2) the BR nets are fitted to, per (information set, stored
        action) over the live M_RL records where they lie, each agent against its own target net
        with ``cfg.gamma`` and ``cfg.quirks`` (nfsp_engine_td_table; step boundaries only).  Under
        ``QUIRK_ALIAS_RL`` a record's key is its hand's LAST s."""
        return _count_tables(self, self.dev, "nfsp_engine_td_table", 1, native.MEM_TD)[0]

    def q_report(self, eta: float | None = None) -> list:
        """The BR half of ``memory_report``, per agent i (``evaluation.q_report_from`` has the keys):
        the Q values the BR net holds (``evaluation.head_tables``) and the TD values M_RL holds for
        it (``td_table``) against the exact action values q / reach of ``best_response_table(eta,
        values=True)`` -- the opponent is the other seat's AR policy, or with ``eta`` its per-hand
        mixture, as ``br_gap(eta=)`` builds it.  ``td_rmse_exact`` is the data against the truth,
        ``fit_rmse_td`` the net against its data.  Under ``QUIRK_ALIAS_RL`` a record's key is its
        hand's LAST s, and under ``QUIRK_ROW0_TARGET`` the net is fitted to one TD value per 128
        sampled rows: the report states what is stored and what the net holds."""
        td, info = self.td_table()
        return diagnostics.q_reports(self.ctx, [self], [td], [info], eta)[0]

    # -- tabular NFSP ----------------------------------------------------
    def tabular_q(self, sweeps: int | None = None, fill=None):
        """``(q, MemoryTable, [info of agent 0, of agent 1], changed)``: a Q table fitted to the live
        M_RL records by ``sweeps`` Jacobi sweeps Q <- mean over the records of (set, action) of
        r + gamma max_a Q(s2, a), each agent on its own rows with ``cfg.gamma`` and ``cfg.quirks``
        (nfsp_engine_tabular_q; step boundaries only; include/nfsp.h has the arithmetic).  ``q`` is
        a float32 device tensor ``[ndec, 3, 3]``, the table the last sweep's sums, ``changed`` the
        entries the last sweep changed.  A (set, action) without a record is ``fill``'s value
        (float32 ``[ndec, 3, 3]``, None: 0) through every sweep.  ``sweeps`` None: the tree's
        ``nlev``, which without ``QUIRK_ALIAS_RL`` is the fixed point; under it a record's key is
        its hand's LAST s and the result is just that many sweeps."""
        return diagnostics.tabular_q([self], sweeps, fill)[0]

    def tabular_q_report(self, sweeps: int | None = None, fill=None, eta: float | None = None) -> list:
        """``q_report`` of the tabular Q (``diagnostics.tabular_q_report``): per agent what a learner
        without function approximation makes of M_RL, against the exact action values."""
        q, td, info, _ = self.tabular_q(sweeps, fill)
        return diagnostics.tabular_q_report(self, q, td, info, eta)

    def install_tabular_br(self, sweeps: int | None = None, fill=None):
        """Tabular-BR self-play: both agents' BR role acts with ``tabular_q(sweeps, fill)``'s rows,
        greedily and with the epsilon draw as the net would.  Installed at a step boundary, the
        table acts in every slice of the step; call it before every step to refresh;
        ``clear_act_tables`` undoes it.  The BR chains still train on M_RL.  Tables are session
        settings, in neither the checkpoint nor the digest.  Returns what ``tabular_q`` returns."""
        res = self.tabular_q(sweeps, fill)
        for a in (0, 1):
            self._set_act_table(a, NET_BR, res[0])
        return res

    def install_tabular_ar(self, stat: str = "mass", fill=None):
        """Tabular-AR self-play: both agents' AR role acts with M_SL's own table, "mass" (the summed
        action vectors, the exact minimiser of the AR net's cross-entropy) or "argmax" (the counts),
        normalised per information set on the device (``evaluation.table_rows``).  A set M_SL never
        saw, or without positive mass, takes ``fill``'s row (float32 ``[ndec, 3, 3]``); ``fill``
        None: the AR net's own softmax row there.  Under the reference quirks the slot executes the
        row's first maximum, under ``EXT_SAMPLE_AR`` it samples it.  Declared as
        ``install_tabular_br``; the AR chains still train on M_SL.  Returns the installed rows."""
        rows = diagnostics.tabular_ar_rows([self], stat, fill)[0]
        for a in (0, 1):
            self._set_act_table(a, NET_AR, rows)
        return rows

    # -- nets fitted to tables ---------------------------------------------
    def warm_start(self, policy, q="exact", steps: int = 2000, lr=(0.5, 0.05), momentum: float = 0.9,
                   weights="visit") -> dict:
        """Self-play started from a solved table, at a step boundary only: the two AR nets are
        fitted to ``policy`` (an ``evaluation.Policy`` or ``[ndec, 3, 3]``, e.g. a ``CfrSolver``
        average) with cross-entropy under ``weights`` ("visit", "uniform" or ``[ndec, 3]``), from
        the nets as they are; with ``q`` "exact" the BR nets to the exact action values against
        ``policy`` (q / reach of ``evaluation.best_response``, weight reach, the legal actions), or
        to the array ``q``; ``q`` None leaves the BR and target nets alone.  The BR head and loss
        are the ones ``cfg.quirks`` trains: linear with ``EXT_LINEAR_Q``, else ReLU; MSE with
        ``EXT_MSE_Q``, else Huber.  The target nets become copies of the BR nets.  ``lr``: one rate,
        or (AR, BR).  All jobs run in one ``evaluation.fit_tables`` call (deterministic).  Memories,
        counters and schedules are untouched; the nets are in the state blob, so save and resume
        need nothing new.  Returns ``{"losses_ar", "losses_br" ([seat][before, after]),
        "exploitability_before", "exploitability_after"}``."""
        return diagnostics.warm_start([self], policy, q, steps, lr, momentum, weights)[0]

    # -- checkpoints (checkpoint.py) ----------------------------------
    def save(self, path):
        """Save the engine at a step boundary (nfsp_engine_save_state); returns the bytes written."""
        return checkpoint.save(self, path)

    def load(self, path):
        """Load a checkpoint into this engine (nfsp_engine_load_state): the continued run is
        bit-identical to the uninterrupted one.  Re-issue ``set_exchange`` afterwards."""
        checkpoint.load(self, path)

    def state_digest(self) -> tuple:
        """(D0, D1) a save would put in its header now, computed on the device state in place
        (nfsp_engine_state_digest): equal iff the training state is, whatever the slicing."""
        d = (native.U64 * 2)()
        native.check(self.L.nfsp_engine_state_digest(self.h, d), "nfsp_engine_state_digest")
        return int(d[0]), int(d[1])

    def state_digest_timed(self) -> tuple:
        """((D0, D1), the digest kernels' ms, the bytes they read) -- nfsp_engine_state_digest_timed."""
        d, ms, nb = (native.U64 * 2)(), native.F64(), native.I64()
        native.check(self.L.nfsp_engine_state_digest_timed(self.h, d, C.byref(ms), C.byref(nb)),
                     "nfsp_engine_state_digest_timed")
        return (int(d[0]), int(d[1])), ms.value, nb.value

    @classmethod
    def from_checkpoint(cls, path, ctx: native.Context | None = None, init_seed: int = 0, **overrides):
        """An engine built from the file's cfg and game, then loaded from it.  ``overrides``:
        slices, slice_lag and sched only (the state does not depend on them).  The initial nets
        (``init_seed``) are overwritten by the load."""
        data = np.fromfile(path, dtype=np.uint8)
        info = checkpoint.check(data)
        if info.kind != checkpoint.KIND_ENGINE:
            raise native.NativeError("from_checkpoint: the file holds an engine group (EngineGroup.from_checkpoint)")
        cfg, game = checkpoint.stored_cfg(data)
        kw = checkpoint.apply_overrides(cfg, overrides)
        eng = cls(ctx if ctx is not None else native.Context(1, game=game), init_seed=init_seed, **kw)
        try:
            checkpoint.load_bytes(eng, data)
        except Exception:
            eng.close()
            raise
        return eng

    def _destroy(self):
        if self._owner is None:                # a replica's handle is its group's
            self.L.nfsp_engine_destroy(self.h)


class EngineGroup(native.Handle):
    """R replicas of the engine stepped together (``nfsp_group_*``, include/nfsp.h): each an
    independent main.train over ``n_lanes`` lanes with its own memories and nets (seed + r,
    initial nets from ``init_seed + r`` -- replica r is bit-identical to
    ``SelfPlayEngine(seed=seed + r, init_seed=init_seed + r)``), their SGD chains in shared
    launches.  ``avg_ar``: the AR nets are averaged over the replicas after every step (C4's
    exchange on device, shards.AvgPolicyAllReduce); ``set_exchange`` for other cadences (e.g.
    after every slice, shards.AvgPolicyExchange's).  ``slice_lag=2``: every replica's slice j
    acts with the nets slice j - 2 left (a pipelined engine's arithmetic; executed pipelined --
    slice j + 1's rollout, plan and prep overlap slice j's chains -- unless the BR nets are
    exchanged or ``set_sched(serial=1)``).

    ``cfgs=[dict, ...]`` instead of ``replicas`` and cfg keywords: a heterogeneous group
    (``nfsp_group_create_v``), one sweep point per replica.  Each dict goes through ``make_cfg``
    and replica r runs it exactly as given (its seed is not offset) -- bit-identical to
    ``SelfPlayEngine(init_seed=init_seeds[r], **cfgs[r])``.  The replicas may differ in seed,
    eta, lr_br, lr_ar, gamma, epsilon, target_every and the quirks outside
    EXT_LINEAR_Q | EXT_MSE_Q; such a group has no exchange.  ``init_seeds[r]`` seeds replica r's
    initial nets (default ``init_seed + r``); equal entries give paired initial nets.
    ``self.cfgs``: every replica's cfg as the group runs it (``nfsp_group_replica_cfg``)."""

    def __init__(self, replicas: int | None = None, ctx: native.Context | None = None, init_seed: int = 0,
                 game: int = native.GAME_LEDUC, avg_ar: bool = False, cfgs=None, init_seeds=None, **cfg):
        if cfgs is not None and (replicas is not None or cfg):
            raise TypeError("EngineGroup: cfgs excludes replicas and cfg keywords (put them in each dict)")
        if cfgs is None and replicas is None:
            raise TypeError("EngineGroup: replicas or cfgs")
        self.ctx = ctx if ctx is not None else native.Context(1, game=game)
        self.L = self.ctx.L
        flags = native.GROUP_AVG_AR if avg_ar else 0
        h = native.P()
        if cfgs is not None:
            made = [make_cfg(self.L, **dict(c)) for c in cfgs]
            self.R = len(made)
            arr = (native.EngineCfg * max(self.R, 1))(*made)
            self.cfg = made[0] if made else make_cfg(self.L)
            native.check(self.L.nfsp_group_create_v(self.ctx.h, arr, self.R, flags, C.byref(h)),
                         "nfsp_group_create_v")
        else:
            self.R = int(replicas)
            self.cfg = make_cfg(self.L, **cfg)
            native.check(self.L.nfsp_group_create(self.ctx.h, C.byref(self.cfg), self.R, flags, C.byref(h)),
                         "nfsp_group_create")
        self.h = h
        self.cfgs = []
        self.replicas = []
        if init_seeds is None:
            init_seeds = [init_seed + r for r in range(self.R)]
        if len(init_seeds) != self.R:
            self.close()
            raise ValueError(f"EngineGroup: {len(init_seeds)} init_seeds for {self.R} replicas")
        for r in range(self.R):
            e = native.P()
            native.check(self.L.nfsp_group_engine(self.h, r, C.byref(e)), "nfsp_group_engine")
            c = native.EngineCfg()
            native.check(self.L.nfsp_group_replica_cfg(self.h, r, C.byref(c)), "nfsp_group_replica_cfg")
            self.cfgs.append(c)
            self.replicas.append(SelfPlayEngine(self.ctx, init_seed=int(init_seeds[r]), _borrow=(self, e, c)))

    def step(self):
        native.check(self.L.nfsp_group_step(self.h), "nfsp_group_step")

    def average_ar(self):
        native.check(self.L.nfsp_group_average_ar(self.h), "nfsp_group_average_ar")

    def set_exchange(self, nets: int = native.XCHG_AR, every: int = 1, scale: float | None = None):
        """nfsp_group_set_exchange: after every ``every``-th slice, the ``nets``
        (native.XCHG_AR | XCHG_BR) of all replicas <- W0 + (sum_r W_r - W0) * scale (default
        1 / R, the mean); every 0: off.  The next exchange of a net not exchanged before copies
        replica 0's instead."""
        scale = 1.0 / self.R if scale is None else float(scale)
        native.check(self.L.nfsp_group_set_exchange(self.h, int(nets), int(every), scale),
                     "nfsp_group_set_exchange")

    def sched(self) -> dict:
        """The group's BR-round / slice schedule (nfsp_group_get_sched)."""
        sc = native.GroupSched()
        native.check(self.L.nfsp_group_get_sched(self.h, C.byref(sc)), "nfsp_group_get_sched")
        return {k: int(getattr(sc, k)) for k, _ in sc._fields_}

    def set_sched(self, **kw):
        """nfsp_group_set_sched: change br_cap / br_pace / br_streams / serial / br_persist
        from the next learner call (the rest stay as they are).  No SGD step changes."""
        cur = self.sched()
        for k in kw:
            if k not in cur:
                raise KeyError(k)
        cur.update(kw)
        native.check(self.L.nfsp_group_set_sched(self.h, C.byref(native.GroupSched(**cur))),
                     "nfsp_group_set_sched")

    def check(self):
        """nfsp_group_check: synchronise the group's streams; raises if a k_br_persist wait
        expired (sched br_persist)."""
        native.check(self.L.nfsp_group_check(self.h), "nfsp_group_check")

    def rounds(self) -> int:
        n = native.I64()
        native.check(self.L.nfsp_group_rounds(self.h, C.byref(n)), "nfsp_group_rounds")
        return n.value

    def set_trace(self, on=True):
        """Start (and clear) / stop the learner-plan trace (nfsp_group_set_trace)."""
        native.check(self.L.nfsp_group_set_trace(self.h, int(bool(on))), "nfsp_group_set_trace")

    def trace(self) -> np.ndarray:
        """The traced learner calls' update counts, [call][replica][agent][AR, BR]."""
        n = native.I64()
        native.check(self.L.nfsp_group_trace(self.h, None, 0, C.byref(n)), "nfsp_group_trace")
        buf = (native.I32 * max(n.value, 1))()
        native.check(self.L.nfsp_group_trace(self.h, buf, n.value, C.byref(n)), "nfsp_group_trace")
        return np.frombuffer(buf, np.int32, count=n.value).reshape(-1, self.R, 2, 2).copy()

    def stats(self) -> dict:
        """Per-replica stats summed (counters) and listed (``replicas``)."""
        per = [e.stats() for e in self.replicas]
        out = {"replicas": per}
        for k in ("hands", "rollouts"):
            out[k] = sum(p[k] for p in per)
        for k in ("rl_total", "sl_total", "br_updates", "ar_updates", "last_rl", "last_sl"):
            out[k] = [sum(p[k][a] for p in per) for a in (0, 1)]
        out["exploitability"] = [float(np.mean([p["exploitability"][a] for p in per])) for a in (0, 1)]
        return out

    KERNELS = SelfPlayEngine.KERNELS

    def set_timing(self, on=True):
        native.check(self.L.nfsp_group_set_timing(self.h, int(bool(on))), "set_timing")

    def timings(self) -> dict:
        return _timings(self, "nfsp_group_get_timings")

    def exploitability(self, mode: int = 0, replica: int = 0) -> dict:
        return self.replicas[replica].exploitability(mode)

    def exploitability_all(self, mode: int = 0) -> list:
        """Exact exploitability of every replica's AR pair in one launch
        (nfsp_exploitability_batch, one workgroup per replica)."""
        w0 = [e._wptr(0, NET_AR) for e in self.replicas]
        w1 = [e._wptr(1, NET_AR) for e in self.replicas]
        return exploitability_batch(self.ctx, w0, w1, mode)

    def br_gap_all(self, ar_mode: int = 0, eta: float | None = None) -> list:
        """``SelfPlayEngine.br_gap`` of every replica, in one batch call (two pairs per replica)."""
        return diagnostics.br_gaps(self.ctx, self.replicas, ar_mode, eta)

    def crossplay(self, mode: int = 0) -> np.ndarray:
        """[R, R]: seat 0's value when replica i's AR net at seat 0 plays replica j's AR net at
        seat 1, all R x R pairs in one batch call (nfsp_evaluate_batch)."""
        p0 = [e.policy(0, NET_AR, mode) for e in self.replicas]
        p1 = [e.policy(1, NET_AR, mode) for e in self.replicas]
        res = evaluation.evaluate_batch(self.ctx, [(a, b) for a in p0 for b in p1])
        return np.array([r["value0"] for r in res]).reshape(self.R, self.R)

    def set_act_table(self, replica: int, agent: int, role: int, rows):
        """``SelfPlayEngine.set_act_table`` for replica ``replica`` (nfsp_group_set_act_table;
        step boundaries of the group only).  The other replicas act as before."""
        t = _act_rows_dev(self.replicas[replica], rows)
        native.check(self.L.nfsp_group_set_act_table(self.h, int(replica), int(agent), int(role), native.ptr(t)),
                     "nfsp_group_set_act_table")

    def memory_tables(self, kind: int) -> list:
        """Every replica's ``SelfPlayEngine.memory_table(kind)`` in one launch
        (nfsp_group_memory_tables): ``[(MemoryTable, [info 0, info 1])]`` by replica."""
        return _count_tables(self, self.replicas[0].dev, "nfsp_group_memory_tables", self.R, kind, int(kind))

    def memory_report_all(self) -> list:
        """``SelfPlayEngine.memory_report`` of every replica: one table launch per memory, and
        one ``evaluate_batch`` per 64 replicas."""
        sl, rl = self.memory_tables(native.MEM_SL), self.memory_tables(native.MEM_RL)
        out = []
        for r0 in range(0, self.R, 64):
            rs = range(r0, min(r0 + 64, self.R))
            out += diagnostics.memory_reports(self.ctx, [self.replicas[r] for r in rs], [sl[r][0] for r in rs],
                                              [rl[r][0] for r in rs], [(sl[r][1], rl[r][1]) for r in rs])
        return out

    def td_tables(self) -> list:
        """Every replica's ``SelfPlayEngine.td_table()`` in one launch (nfsp_group_td_tables), each
        with its own gamma, quirks and target nets: ``[(MemoryTable, [info 0, info 1])]``."""
        return _count_tables(self, self.replicas[0].dev, "nfsp_group_td_tables", self.R, native.MEM_TD)

    def q_report_all(self, eta: float | None = None) -> list:
        """``SelfPlayEngine.q_report`` of every replica: one TD launch and one head launch (per 32
        replicas) for all of them."""
        tds = self.td_tables()
        return diagnostics.q_reports(self.ctx, self.replicas, [t for t, _ in tds], [i for _, i in tds], eta)

    def tabular_q_all(self, sweeps: int | None = None, fill=None) -> list:
        """Every replica's ``SelfPlayEngine.tabular_q`` (nfsp_group_tabular_q): three launches per
        sweep for all of them, each replica with its own gamma and quirks.  ``fill``: one table for
        all, or ``[R, ndec, 3, 3]``."""
        return diagnostics.tabular_q(self.replicas, sweeps, fill)

    def install_tabular_br_all(self, sweeps: int | None = None, fill=None) -> list:
        """``SelfPlayEngine.install_tabular_br`` for every replica, from one ``tabular_q_all``."""
        res = self.tabular_q_all(sweeps, fill)
        for r in range(self.R):
            for a in (0, 1):
                self.set_act_table(r, a, NET_BR, res[r][0])
        return res

    def install_tabular_ar_all(self, stat: str = "mass", fill=None):
        """``SelfPlayEngine.install_tabular_ar`` for every replica: one M_SL table launch, one head
        launch (without ``fill``) and one rows launch for all of them.  Returns the rows
        ``[R, ndec, 3, 3]``."""
        rows = diagnostics.tabular_ar_rows(self.replicas, stat, fill)
        for r in range(self.R):
            for a in (0, 1):
                self.set_act_table(r, a, NET_AR, rows[r])
        return rows

    def warm_start_all(self, policy, q="exact", steps: int = 2000, lr=(0.5, 0.05), momentum: float = 0.9,
                       weights="visit") -> list:
        """``SelfPlayEngine.warm_start`` for every replica, all of their jobs (4R with ``q``) in
        one ``evaluation.fit_tables`` call of 64-job launches; a replica's nets are the bits a
        standalone engine's warm start gives.  Returns the replicas' dicts."""
        return diagnostics.warm_start(self.replicas, policy, q, steps, lr, momentum, weights)

    # -- checkpoints (checkpoint.py) ----------------------------------
    def save(self, path):
        """Save the group at a step boundary (nfsp_group_save_state): every replica, and the
        exchange's W0 with its "already broadcast" flags; returns the bytes written."""
        return checkpoint.save(self, path)

    def load(self, path):
        checkpoint.load(self, path)

    def state_digest(self) -> list:
        """Every replica's ``SelfPlayEngine.state_digest()``."""
        return [e.state_digest() for e in self.replicas]

    @classmethod
    def from_checkpoint(cls, path, ctx: native.Context | None = None, init_seed: int = 0, **overrides):
        """A group built from the file's replica count, flags, every replica's own cfg and the
        game, then loaded from it (``overrides``: slices, slice_lag and sched only, applied to
        every replica)."""
        data = np.fromfile(path, dtype=np.uint8)
        info = checkpoint.check(data)
        if info.kind != checkpoint.KIND_GROUP:
            raise native.NativeError("from_checkpoint: the file holds a single engine (SelfPlayEngine.from_checkpoint)")
        game = checkpoint.stored_cfg(data, 0)[1]
        kws = [checkpoint.apply_overrides(checkpoint.stored_cfg(data, r)[0], overrides) for r in range(info.replicas)]
        grp = cls(ctx=ctx if ctx is not None else native.Context(1, game=game), init_seed=init_seed,
                  avg_ar=bool(info.group_flags & native.GROUP_AVG_AR), cfgs=kws)
        try:
            checkpoint.load_bytes(grp, data)
        except Exception:
            grp.close()
            raise
        return grp

    def _destroy(self):
        for e in self.replicas:
            e.h = None
        self.L.nfsp_group_destroy(self.h)


def _act_rows_dev(e, rows):
    """``rows`` of a set_act_table call as a float32 device tensor of the game's size, or None."""
    if rows is None:
        return None
    t = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(rows))
    if t.dtype != torch.float32:
        raise TypeError("set_act_table: float32 rows (evaluation.act_rows converts a policy table)")
    ndec = evaluation.GameTree.of(e.ctx.game).ndec
    if t.numel() != ndec * 9:
        raise ValueError(f"set_act_table: expected [{ndec}, 3, 3] rows, got {tuple(t.shape)}")
    return t.to(e.dev).contiguous()

"""Diagnostics of an engine: everything that needs both an engine and the exact evaluator.

Functions over anything with a ``SelfPlayEngine``'s ``ctx``, ``cfg``, ``policy``, ``act_table`` and
``_wptr`` (a replica of an ``EngineGroup`` is one); the engine's methods of the same names carry the
documentation and delegate here.  ``opponents`` is the one statement of what seat o plays.
"""
from __future__ import annotations

import numpy as np

from . import evaluation as ev
from . import native
from .native import NET_AR, NET_BR


def _ar_mode(e, ar_mode):
    """``ar_mode``, None being what the rollout executes under ``cfg.quirks``."""
    return ar_mode if ar_mode is not None else 0 if e.cfg.quirks & native.EXT_SAMPLE_AR else 1


def acting_policy(e, agent: int, role: int, ar_mode: int | None = None, tree=None) -> np.ndarray:
    """``SelfPlayEngine.acting_policy``: slot (agent, role)'s installed table as executed, else its net's."""
    tree = tree or ev.GameTree.of(e.ctx.game)
    ar_mode = _ar_mode(e, ar_mode)
    rows, _ = e.act_table(agent, role)
    if rows is None:
        return ev.policy_table(e.ctx, e.policy(agent, role, ar_mode), tree).cpu().numpy()
    y = rows.cpu().numpy().astype(np.float64)
    if role == NET_AR and ar_mode == 0:
        c0 = np.clip(y[..., 0], 0.0, 1.0)
        c1 = np.clip(y[..., 0] + y[..., 1], c0, 1.0)
        t = np.stack([c0, c1 - c0, 1.0 - c1], axis=-1)
    else:
        t = np.eye(3)[np.argmax(y, axis=-1)]            # the first maximum, as the env's argmax
    return tree.remap(t)


def opponents(e, ar_mode, eta, tree=None, tables: bool = False) -> list:
    """[the policy agent 1 - o faces at seat o, o = 0, 1]: engine e's AR part there,
    ``acting_policy(e, o, NET_AR, ar_mode)``, or with ``eta`` the per-hand mixture eta x BR part
    (``acting_policy(e, o, NET_BR)``) + (1 - eta) x AR part it plays in self-play.  An AR slot
    whose net acts is passed as the net itself (no launch) unless ``tables``."""
    tree = tree or ev.GameTree.of(e.ctx.game)
    opp = []
    for o in (0, 1):
        if eta is not None:
            br, ar = acting_policy(e, o, NET_BR, None, tree), acting_policy(e, o, NET_AR, ar_mode, tree)
            opp.append(ev.Policy.table(ev.mix(tree, [(eta, br), (1.0 - eta, ar)])))
        elif tables or e.act_table(o, NET_AR)[0] is not None:
            opp.append(ev.Policy.table(acting_policy(e, o, NET_AR, ar_mode, tree)))
        else:
            opp.append(e.policy(o, NET_AR, _ar_mode(e, ar_mode)))
    return opp


def br_gaps(ctx, engines, ar_mode, eta) -> list:
    """``br_gap`` of each engine: per agent {br_exact, br_learned, gap}; one nfsp_evaluate_batch."""
    pairs = []
    for e in engines:
        opp = opponents(e, ar_mode, eta)
        pairs += [(e.policy(0, NET_BR), opp[1]), (opp[0], e.policy(1, NET_BR))]
    res = ev.evaluate_batch(ctx, pairs)
    out = []
    for k in range(len(engines)):
        r0, r1 = res[2 * k], res[2 * k + 1]
        out.append([{"br_exact": r0["br0"], "br_learned": r0["value0"], "gap": r0["br0"] - r0["value0"]},
                    {"br_exact": r1["br1"], "br_learned": -r1["value0"], "gap": r1["br1"] + r1["value0"]}])
    return out


def best_response_table(e, eta=None, values: bool = False):
    """``SelfPlayEngine.best_response_table``: the exact best responses to ``opponents`` at AR mode 0."""
    opp = opponents(e, 0, eta)
    return ev.best_response(e.ctx, opp[0], opp[1], values)


def oracle_br(e, eta=None, ar_mode=None):
    """The table ``SelfPlayEngine.install_oracle_br`` installs: the exact best responses to what
    the seats execute, ``ar_mode`` None being the rollout's under ``cfg.quirks``."""
    opp = opponents(e, ar_mode, eta, tables=True)
    return ev.best_response(e.ctx, opp[0], opp[1])


def q_reports(ctx, engines, td_tables, infos, eta=None, tree=None) -> list:
    """``SelfPlayEngine.q_report`` of every engine from its TD table: one ``head_tables`` launch for
    all of their BR nets (per 64), one ``best_response`` per engine."""
    tree = tree or ev.GameTree.of(ctx.game)
    lin = [bool(e.cfg.quirks & native.EXT_LINEAR_Q) for e in engines]
    head = ev.head_tables(ctx, [e._wptr(a, NET_BR) for e in engines for a in (0, 1)],
                          [native.ACT_LINEAR if l else native.ACT_RELU for l in lin for _ in (0, 1)], tree).cpu().numpy()
    out = []
    for k, e in enumerate(engines):
        beta, q, reach = (t.cpu().numpy() for t in best_response_table(e, eta, True))
        out.append([ev.q_report_from(tree, a, beta, q, reach, head[2 * k + a], td_tables[k], lin[k],
                                     float(e.cfg.gamma), infos[k][a]) for a in (0, 1)])
    return out


def memory_reports(ctx, engines, sl_tables, rl_tables, infos, tree=None) -> list:
    """``SelfPlayEngine.memory_report`` of every engine from its tables: the AR pair and the two
    M_SL tables of all of them scored in one ``evaluate_batch`` call.  The nets are scored, also
    where a table acts for one."""
    tree = tree or ev.GameTree.of(ctx.game)
    tabs = [(sl.policy("argmax"), sl.policy("mass")) for sl in sl_tables]
    pairs = []
    for e, (am, ms) in zip(engines, tabs):
        pa, pm = ev.Policy.table(am), ev.Policy.table(ms)
        pairs += [(e.policy(0, NET_AR), e.policy(1, NET_AR)), (pa, pa), (pm, pm)]
    res = ev.evaluate_batch(ctx, pairs)
    legal = np.ones((tree.ndec, 3, 3), bool)
    legal[~tree.legal, :, 2] = False
    out = []
    for k, e in enumerate(engines):
        sl, rl = sl_tables[k], rl_tables[k]
        ar, am, ms = (res[3 * k + j]["exploitability"] for j in range(3))
        mass = tree.remap(tabs[k][1])
        num = den = 0.0
        for seat in (0, 1):
            net = ev.policy_table(ctx, e.policy(seat, NET_AR), tree).cpu().numpy()
            rows = tree.seat == seat
            w = sl.n[rows].astype(np.float64)
            num += float((w * np.abs(net[rows] - mass[rows]).sum(axis=2)).sum())
            den += float(w.sum())
        out.append({
            "exploitability_ar": ar, "exploitability_sl_argmax": am, "exploitability_sl_mass": ms,
            # what the net adds to the strategy it is a fit of (> 0: the net is more exploitable)
            "fit_gap_argmax": ar - am, "fit_gap_mass": ar - ms,
            "sl_empty_sets": int((sl.n == 0).sum()),
            "rl_empty_actions": int(((rl.counts == 0) & legal).sum()),
            "ar_mass_l1": num / den if den > 0 else float("nan"),
            "sl_info": infos[k][0], "rl_info": infos[k][1]})
    return out


# -- tabular NFSP: the nets' roles played by tables of exactly the nets' data ----------
def _group_of(engines):
    """The ``EngineGroup`` whose replicas ``engines`` are, in order; None for anything else."""
    g = getattr(engines[0], "_owner", None)
    return g if g is not None and len(engines) == len(g.replicas) and all(a is b for a, b in zip(engines, g.replicas)) else None


def _fill_dev(fill, R, tree, dev):
    """``fill`` of a tabular call as a float32 device tensor ``[R, ndec, 3, 3]`` (one table serves
    every engine), or None."""
    import torch
    if fill is None:
        return None
    t = fill if isinstance(fill, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(fill))
    if t.dtype != torch.float32 or t.numel() not in (tree.ndec * 9, R * tree.ndec * 9):
        raise ValueError(f"fill: float32 [{tree.ndec}, 3, 3], or one such table per engine")
    t = t.to(dev).reshape(-1, tree.ndec, 3, 3)
    return (t.expand(R, -1, -1, -1) if t.shape[0] != R else t).contiguous()


def tabular_q(engines, sweeps=None, fill=None) -> list:
    """``SelfPlayEngine.tabular_q`` of every engine: ``[(q, MemoryTable, info, changed)]``.  The
    replicas of an ``EngineGroup``, all and in order, go through nfsp_group_tabular_q (three
    launches per sweep for all of them); other engines through one nfsp_engine_tabular_q each."""
    import ctypes as C
    import torch
    e0 = engines[0]
    tree = ev.GameTree.of(e0.ctx.game)
    sweeps = tree.nlev if sweeps is None else int(sweeps)
    grp = _group_of(engines)
    calls = [(grp, "nfsp_group_tabular_q", len(engines))] if grp is not None else [(e, "nfsp_engine_tabular_q", 1) for e in engines]
    fill = _fill_dev(fill, len(engines), tree, e0.dev)
    out, r0 = [], 0
    for obj, fn, R in calls:
        q = torch.empty((R, tree.ndec, 3, 3), dtype=torch.float32, device=e0.dev)
        tab = torch.empty((R, tree.ndec, 3, 3, 3), dtype=torch.int64, device=e0.dev)
        info = (native.MemtabInfo * (2 * R))()
        changed = (C.c_int32 * R)()
        native.check(getattr(obj.L, fn)(obj.h, sweeps, native.ptr(None if fill is None else fill[r0:r0 + R]), native.ptr(q),
                                        native.ptr(tab), info, changed), fn)
        raw = tab.cpu().numpy()
        out += [(q[r], ev.MemoryTable(tree, native.MEM_TDQ, raw[r]), [info[2 * r].to_dict(), info[2 * r + 1].to_dict()],
                 int(changed[r])) for r in range(R)]
        r0 += R
    return out


def tabular_ar_rows(engines, stat="mass", fill=None, sl_tables=None):
    """The rows ``SelfPlayEngine.install_tabular_ar`` installs, float32 device ``[R, ndec, 3, 3]``:
    every engine's M_SL table (``sl_tables``: their ``MemoryTable``s when already counted) through
    one ``table_rows`` launch.  ``fill`` None: each agent's AR net's own softmax head row
    (one ``head_tables`` launch for all of them)."""
    import torch
    e0 = engines[0]
    tree = ev.GameTree.of(e0.ctx.game)
    if stat not in ("mass", "argmax"):
        raise ValueError('stat must be "mass" or "argmax"')
    R = len(engines)
    if fill is None:
        heads = ev.head_tables(e0.ctx, [e._wptr(a, NET_AR) for e in engines for a in (0, 1)], [native.ACT_SOFTMAX] * (2 * R), tree)
        mine = torch.as_tensor(tree.seat.astype(np.int64), device=heads.device)          # row -> the agent that acts there
        heads = heads.view(R, 2, tree.ndec, 3, 3)
        fill = torch.where((mine == 0)[None, :, None, None], heads[:, 0], heads[:, 1]).contiguous()
    else:
        fill = _fill_dev(fill, R, tree, e0.dev)
    if sl_tables is None:
        grp = _group_of(engines)
        sl_tables = [t for t, _ in grp.memory_tables(native.MEM_SL)] if grp is not None else \
            [e.memory_table(native.MEM_SL)[0] for e in engines]
    raw = np.stack([t.raw for t in sl_tables])
    rows, _ = ev.table_rows(e0.ctx, native.ROWS_SL_MASS if stat == "mass" else native.ROWS_SL_ARGMAX, raw, fill, tree=tree)
    return rows


def tabular_q_report(e, q, td, info, eta=None, tree=None) -> list:
    """``SelfPlayEngine.q_report`` with the Q table ``q`` of ``tabular_q`` in the BR heads' place and
    its last sweep's table ``td`` as the data, per agent (``evaluation.q_report_from`` has the keys,
    ``linear`` True: a table has no ReLU).  ``q_rmse_exact`` and ``greedy_mismatch_share`` are the
    tabular learner's; at the sweeps' fixed point ``fit_rmse_td`` is 0 by construction."""
    tree = tree or ev.GameTree.of(e.ctx.game)
    beta, qx, reach = (t.cpu().numpy() for t in best_response_table(e, eta, True))
    return [ev.q_report_from(tree, a, beta, qx, reach, q, td, True, float(e.cfg.gamma), info[a]) for a in (0, 1)]


# -- nets fitted to tables: distillation and warm starts -------------------------------
def _as_policy(ctx, table, tree):
    """``table`` (a ``Policy`` or an array ``[ndec, 3, 3]``) as (``Policy``, its executed host table)."""
    if isinstance(table, ev.Policy):
        return table, ev.policy_table(ctx, table, tree).cpu().numpy()
    t = tree.remap(table)
    return ev.Policy.table(t), t


def _fit_weights(ctx, pol, weights, tree):
    """``weights`` of a distillation as float64 ``[ndec, 3]``, None for "uniform"."""
    if isinstance(weights, str):
        if weights == "uniform":
            return None
        if weights == "visit":
            return ev.visit_weights(ctx, pol, pol, tree)
        raise ValueError('weights must be "visit", "uniform" or an array [ndec, 3]')
    return np.asarray(weights, np.float64).reshape(tree.ndec, 3)


def _init_pairs(init, n, hidden=64):
    """``init`` of a distillation as n pairs of packed nets: a seed (seat 0's net, then seat 1's,
    Glorot of width ``hidden``, from one stream), a pair of nets of that width, or a list of either."""
    items = list(init) if isinstance(init, (list, tuple)) and not (len(init) == 2 and np.ndim(init[0]) == 1) else [init]
    if len(items) == 1:
        items = items * n
    if len(items) != n:
        raise ValueError(f"{len(items)} inits for {n} variants")
    out = []
    for it in items:
        if np.ndim(it) == 0:
            rng = np.random.RandomState(int(it))
            out.append((ev.glorot_net(rng, hidden), ev.glorot_net(rng, hidden)))
        else:
            out.append((np.asarray(it[0], np.float32), np.asarray(it[1], np.float32)))
            for w in out[-1]:
                if ev.net_width(w) != hidden:
                    raise ValueError(f"an init net of width {ev.net_width(w)} where hidden is {hidden}")
    return out


def _variants(lr, momentum, init, hidden=64):
    ls = list(lr) if isinstance(lr, (list, tuple)) else [lr]
    ms = list(momentum) if isinstance(momentum, (list, tuple)) else [momentum]
    n = max(len(ls), len(ms), len(init) if isinstance(init, list) else 1)
    ls, ms = (x * n if len(x) == 1 else x for x in (ls, ms))
    if len(ls) != n or len(ms) != n:
        raise ValueError("lr, momentum and init lists must have one length")
    many = any(isinstance(x, (list, tuple)) for x in (lr, momentum)) or isinstance(init, list)
    return ls, ms, _init_pairs(init, n, hidden), many


def q_targets(ctx, policy, tree=None):
    """What a Q net is to hold against ``policy`` at both seats: ``(qx, reach, (beta, q, reach))``
    with qx = q / reach of ``best_response(values=True)`` (0 where the information set is not
    reached: its weight ``reach`` is 0 there)."""
    tree = tree or ev.GameTree.of(ctx.game)
    pol, _ = _as_policy(ctx, policy, tree)
    beta, q, reach = (t.cpu().numpy() for t in ev.best_response(ctx, pol, pol, values=True, tree=tree))
    with np.errstate(invalid="ignore", divide="ignore"):
        qx = np.where(reach[:, :, None] > 0, q / reach[:, :, None], 0.0)
    return qx, reach, (beta, q, reach)


def distill_policy(ctx, table, weights="visit", steps: int = 2000, lr=0.5, momentum=0.9, init=0, tree=None,
                   hidden: int = 64):
    """The approximation floor of the AR net: two 30-H-3 softmax nets (``hidden``: 16, 32, 64 or
    128; scored through ``evaluation.net_policy`` where it is not 64), one per seat, fitted to
    ``table`` (a ``Policy`` or ``[ndec, 3, 3]``; as executed) by ``evaluation.fit_tables`` with
    cross-entropy.  ``weights``: "visit" (``evaluation.visit_weights`` of the table against itself:
    fitted where it is played), "uniform", or ``[ndec, 3]``.  ``init``: a seed for Glorot nets, or
    the pair of packed nets to start from.  Returns ``{"nets": [w0, w1] (float32 device tensors),
    "losses": [2, 2] (seat; before, after), "entropy": [2] (the targets' own weighted entropy: the
    loss's floor), "scores": {"table", "softmax", "argmax"}}``, the scores being the exact
    exploitability of the table and of the nets in both modes, from one ``evaluate_batch``.

    ``lr``, ``momentum`` and ``init`` may be lists of one length (``init`` a list of seeds or
    pairs): that many variants in ONE ``fit_tables`` call and one ``evaluate_batch``; the result is
    then the list of the variants' dicts."""
    tree = tree or ev.GameTree.of(ctx.game)
    pol, tab = _as_policy(ctx, table, tree)
    wt = _fit_weights(ctx, pol, weights, tree)
    native.net_params(hidden)
    ls, ms, inits, many = _variants(lr, momentum, init, hidden)
    jobs = [ev.FitJob(inits[k][s], tab, s, native.ACT_SOFTMAX, "ce", ls[k], ms[k], wt)
            for k in range(len(ls)) for s in (0, 1)]
    losses = ev.fit_tables(ctx, jobs, steps, tree)
    pairs = [(pol, pol)]
    for k in range(len(ls)):
        for mode in (0, 1):
            if hidden == 64:
                pairs.append((ev.Policy.ar(jobs[2 * k].w, mode), ev.Policy.ar(jobs[2 * k + 1].w, mode)))
            else:
                kind = native.POL_AR_ARGMAX if mode else native.POL_AR_SOFTMAX
                pairs.append((ev.net_policy(ctx, jobs[2 * k].w, kind, tree), ev.net_policy(ctx, jobs[2 * k + 1].w, kind, tree)))
    res = ev.evaluate_batch(ctx, pairs)
    w = np.ones((tree.ndec, 3)) if wt is None else wt
    ent = []
    for s in (0, 1):
        rows = tree.seat == s
        ws = w[rows] / w[rows].sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            ent.append(float((ws * -np.where(tab[rows] > 0, tab[rows] * np.log(tab[rows]), 0.0).sum(axis=2)).sum()))
    out = [{"nets": [jobs[2 * k].w, jobs[2 * k + 1].w], "losses": losses[2 * k:2 * k + 2], "entropy": ent,
            "scores": {"table": res[0]["exploitability"], "softmax": res[1 + 2 * k]["exploitability"],
                       "argmax": res[2 + 2 * k]["exploitability"]}} for k in range(len(ls))]
    return out if many else out[0]


def distill_q(ctx, policy, linear: bool = False, loss: str = "mse", steps: int = 2000, lr=0.05, momentum=0.9,
              init=0, tree=None, hidden: int = 64):
    """The approximation floor of the Q net: two 30-H-3 nets (``hidden`` as ``distill_policy``'s), one
    per seat, with the ReLU head
    (the reference's) or the ``linear`` one, fitted to the exact action values against ``policy``
    -- qx = q / reach of ``best_response(values=True)`` -- with weight ``reach`` and the legal
    actions as the mask, by "mse" or "huber".  Returns ``{"nets", "losses" [2, 2], "reports":
    [per seat ``evaluation.q_report_from``'s q_rmse_exact, greedy_mismatch_share and
    relu_blind_share], "br_gap": [per seat br_exact, br_learned, gap of the fitted net played
    greedily against ``policy``]}``; lists of ``lr`` / ``momentum`` / ``init`` as ``distill_policy``."""
    tree = tree or ev.GameTree.of(ctx.game)
    pol, _ = _as_policy(ctx, policy, tree)
    qx, reach, (beta, q, _) = q_targets(ctx, pol, tree)
    head = native.ACT_LINEAR if linear else native.ACT_RELU
    native.net_params(hidden)
    ls, ms, inits, many = _variants(lr, momentum, init, hidden)
    jobs = [ev.FitJob(inits[k][s], qx, s, head, loss, ls[k], ms[k], reach) for k in range(len(ls)) for s in (0, 1)]
    losses = ev.fit_tables(ctx, jobs, steps, tree)
    heads = ev.head_tables(ctx, [j.w for j in jobs], [head] * len(jobs), tree).cpu().numpy()
    pairs = []
    kind = native.POL_BR_GREEDY_LINEAR if linear else native.POL_BR_GREEDY

    def greedy(w):
        return ev.Policy.br(w, linear) if hidden == 64 else ev.net_policy(ctx, w, kind, tree)
    for k in range(len(ls)):
        pairs += [(greedy(jobs[2 * k].w), pol), (pol, greedy(jobs[2 * k + 1].w))]
    res = ev.evaluate_batch(ctx, pairs)
    none = np.zeros((tree.ndec, 3, 3, 3), np.int64)
    out = []
    for k in range(len(ls)):
        rep = []
        for s in (0, 1):
            r = ev.q_report_from(tree, s, beta, q, reach, heads[2 * k + s], none, linear)
            rep.append({key: r[key] for key in ("q_rmse_exact", "greedy_mismatch_share", "relu_blind_share")})
        r0, r1 = res[2 * k], res[2 * k + 1]
        out.append({"nets": [jobs[2 * k].w, jobs[2 * k + 1].w], "losses": losses[2 * k:2 * k + 2], "reports": rep,
                    "br_gap": [{"br_exact": r0["br0"], "br_learned": r0["value0"], "gap": r0["br0"] - r0["value0"]},
                               {"br_exact": r1["br1"], "br_learned": -r1["value0"], "gap": r1["br1"] + r1["value0"]}]})
    return out if many else out[0]


def warm_start(engines, policy, q="exact", steps: int = 2000, lr=(0.5, 0.05), momentum=0.9, weights="visit",
               hidden: int = 64) -> list:
    """``SelfPlayEngine.warm_start`` of every engine (one ctx, one game), all of their jobs -- up to
    four per engine -- in ONE ``fit_tables`` call: the AR nets fitted in place to ``policy`` as
    ``distill_policy`` fits them, from the nets as they are; with ``q`` the BR nets to the action
    values (``q_targets`` against ``policy`` for "exact", or an array ``[ndec, 3, 3]``) with weight
    ``reach``, the head and loss the engine's quirks train, then copied to the target nets.
    ``lr``: one rate or (AR, BR).  ``hidden`` must be 64: the engine's nets are 64 wide."""
    import torch
    if int(hidden) != 64:
        raise ValueError(f"warm_start: hidden is {hidden}, but the engine is 64 wide: its nets, chains and rollout "
                         "are built for 30-64-3 only")
    e0 = engines[0]
    ctx = e0.ctx
    tree = ev.GameTree.of(ctx.game)
    for e in engines:
        e.state_digest()                       # refused off a step boundary
    pol, tab = _as_policy(ctx, policy, tree)
    wt = _fit_weights(ctx, pol, weights, tree)
    lr_ar, lr_br = (lr if isinstance(lr, (list, tuple)) else (lr, lr))
    before = ev.evaluate_batch(ctx, [(e.policy(0, NET_AR), e.policy(1, NET_AR)) for e in engines])
    if q is not None:
        qx, reach, _ = q_targets(ctx, pol, tree)
        if not isinstance(q, str):
            qx = np.asarray(q, np.float64).reshape(tree.ndec, 3, 3)
        elif q != "exact":
            raise ValueError('q must be "exact", None or an array [ndec, 3, 3]')
        qd, rd = torch.as_tensor(qx, device=e0.dev), torch.as_tensor(reach, device=e0.dev)
    td = torch.as_tensor(tab, device=e0.dev)
    wd = None if wt is None else torch.as_tensor(wt, device=e0.dev)
    jobs = []
    for e in engines:
        for s in (0, 1):
            jobs.append(ev.FitJob(e._wptr(s, NET_AR), td, s, native.ACT_SOFTMAX, "ce", lr_ar, momentum, wd))
        if q is not None:
            head = native.ACT_LINEAR if e.cfg.quirks & native.EXT_LINEAR_Q else native.ACT_RELU
            loss = "mse" if e.cfg.quirks & native.EXT_MSE_Q else "huber"
            for s in (0, 1):
                jobs.append(ev.FitJob(e._wptr(s, NET_BR), qd, s, head, loss, lr_br, momentum, rd))
    losses = ev.fit_tables(ctx, jobs, steps, tree)
    if q is not None:
        for e in engines:
            for s in (0, 1):
                e.weights_tensor(s, native.NET_TARGET).copy_(e.weights_tensor(s, NET_BR))
        torch.cuda.synchronize(e0.dev)
    after = ev.evaluate_batch(ctx, [(e.policy(0, NET_AR), e.policy(1, NET_AR)) for e in engines])
    per = 2 if q is None else 4
    return [{"losses_ar": losses[per * k:per * k + 2], "losses_br": None if q is None else losses[per * k + 2:per * k + 4],
             "exploitability_before": before[k]["exploitability"], "exploitability_after": after[k]["exploitability"]}
            for k in range(len(engines))]

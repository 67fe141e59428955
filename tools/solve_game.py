#!/usr/bin/env python3
"""A tabular equilibrium of the game as the engine plays it: CFR+ on the evaluator's tree
(evaluation.CfrSolver, csrc/cfr.hip), scored by the evaluator itself (nfsp_evaluate_batch) --
or, with --solver xfp, the curve of full-width fictitious play on it (evaluation.XfpSolver,
csrc/xfp.hip): the algorithm NFSP approximates, with an exact best response and averaging.

    python tools/solve_game.py --game leduc --iters 4096 --out eq.npz
    python tools/solve_game.py --game leduc --solver xfp --weight linear --eta 0.1 --iters 4096
    python tools/solve_game.py --game leduc --solver xfp --eta 0.5 --runs 64 --every 1024
    python tools/solve_game.py --game leduc --solver mccfr --walkers 1024 --seeds 4 --iters 32768
    python tools/solve_game.py --solver mccfr --time
    python tools/solve_game.py --game leduc --solver mccfr-os --epsilon 0.6 --walkers 1024 --seeds 4 --iters 32768
    python tools/solve_game.py --solver mccfr-os --time
    python tools/solve_game.py --game leduc --solver mccfr-vr --epsilon 0.6 --walkers 1024 --seeds 4 --iters 16384
    python tools/solve_game.py --solver mccfr-vr --time
    python tools/solve_game.py --game leduc --solver mccfr-vr --regret plus --average both --walkers 1024 --seeds 4
    python tools/solve_game.py --solver mccfr-vr --regret plus --average linear --time --time-walkers 1024 --time-runs 4
    python tools/solve_game.py --game leduc --solver mccfr --regret-net --net-steps 32 --net-target rowmax --seeds 4
    python tools/solve_game.py --solver mccfr --regret-net --net-steps 200 --time

eq.npz holds ``table`` [ndec, 3 ranks, 3 actions] (rows as evaluation.GameTree's; usable as
evaluation.Policy.table), ``game``, and per checkpoint (--every, doubling by default)
``iterations``, ``exploitability``, ``br0`` / ``br1``, ``value0`` and ``value0_dealer`` [k, 2]:
what seat 0 wins per hand when it deals / when seat 1 deals.  The game value per dealer lies
within the exploitability of that row.  One JSON line per checkpoint goes to stdout, with the
solver's milliseconds per iteration.

--solver xfp: --eta is the anticipatory parameter (the best response is to (1 - eta) x average
+ eta x last best response), --weight the averaging (uniform: 1/t; linear: t).  --runs N > 1
runs N independent runs in the one launch, eta evenly spaced over [0, --eta]; the fields above
are then the last run's (eta = --eta), ``eta_runs`` / ``exploitability_runs`` list every run's,
and eq.npz also holds ``tables`` [N, ndec, 3, 3].  The milliseconds are the whole handle's.

--solver mccfr: external-sampling MCCFR (evaluation.MccfrSolver, csrc/mccfr.hip), the sampled
tabular yardstick.  --walkers W traversals per seat and iteration, --seeds K independent runs
(seeds 1 .. K) in the one handle.  Its cost is counted in ``traversals`` and ``terminals``
visited, which each checkpoint's line carries beside ``exploitability_runs``; the fields above
are the first seed's.  --time instead reports traversals/s and terminals/s for Leduc at
W = 2^20: one iteration timed with HIP events on the solver's stream, best of 5 after a warm-up.

--solver mccfr-os: outcome-sampling MCCFR (evaluation.MccfrOsSolver, k_mccfr_os_walk) on the same
handle, --epsilon the exploration rate of the updating seat's own actions.  A traversal is one
sampled hand and one terminal, so its lines carry ``hands`` (= traversals) and ``epsilon`` beside
what mccfr's carry, and --time adds ``hands_per_s``.  W x iterations is bounded by the int64
fixed point (include/nfsp.h): 197,912,092 on Leduc at --epsilon 0.6.

--solver mccfr-vr: baseline-corrected outcome sampling, VR-MCCFR (evaluation.MccfrVrSolver,
k_mccfr_vr_walk), with mccfr-os's options and output columns, --time included: the same sampled
hands, the values on the way back up corrected by a learned baseline at every decision.  Its
corrected values are larger than one pay, so its budget is smaller: W x iterations up to
29,142,433 on Leduc at --epsilon 0.6.

--regret-net, for the three mccfr solvers: the regrets are held in two 30-H-3 nets per run (--net-hidden 16, 32,
64 or 128; 64 without it), fitted to R after
every half-iteration, and the walkers read the nets' sigma (evaluation.MccfrNetSolver, k_mccfr_net_apply):
sampled regression CFR.  --net-steps K, --net-lr, --net-momentum, --net-target avg|rowmax, --net-loss mse|huber
and --net-init SEED set the fit; --regret / --average apply as below (left out: plain / uniform).  The lines add
``exploitability_current`` (the nets' sigma scored), ``sigma_tv`` (per seat, the mean total variation between
the nets' sigma and regret matching on R) and ``fit_loss`` ([seat][before, after] of the last fits), each with
a ``_runs`` list over the seeds.  --time then times one iteration at --time-walkers and splits it
into ``ms_walk`` and ``ms_applies`` with HIP events.  Without the flag every output is as it was.

--regret plain|plus and --average uniform|linear|both, for the three mccfr solvers: regret matching+
and the linearly weighted average on the same walks (evaluation.MccfrXSolver, k_mccfr_x_apply; a flag
left out is plain / uniform).  Given either, the handle is nfsp_mccfr_x_create's and the lines carry
``regret`` and ``average``; without both flags the handles are the old ones and the output is as it
was.  ``both`` keeps the linear average as the handle's own and scores the two averages of every run
at every checkpoint, on identical sample paths: ``exploitability_runs_uniform`` and
``exploitability_runs_linear``; the other fields are then the linear average's.  --time takes the
flags too, and --time-walkers W / --time-runs K time K runs of W walkers in the one handle.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def time_mccfr(ev, nat, epsilon=None, walkers=1 << 20, repeats=5, baselines=False, rule=None, runs=1):
    """Best of ``repeats`` single iterations (2 W traversals each) after a warm-up; outcome
    sampling where ``epsilon`` is given, baseline-corrected with ``baselines``; ``rule`` =
    (regret, average) times the handle of nfsp_mccfr_x_create; ``runs`` seeds 1 .. runs in the one
    handle (the counts are the first's)."""
    import torch
    ctx = nat.Context(1, game=nat.GAME_LEDUC)
    seeds = range(1, runs + 1)
    if rule is not None:
        sampling = 0 if epsilon is None else 2 if baselines else 1
        solver = ev.MccfrXSolver(ctx, [(seed, walkers, epsilon or 0.0) + tuple(rule) for seed in seeds], sampling).run(1)
    elif epsilon is None:
        solver = ev.MccfrSolver(ctx, [(seed, walkers) for seed in seeds]).run(1)
    elif baselines:
        solver = ev.MccfrVrSolver(ctx, [(seed, walkers, epsilon) for seed in seeds]).run(1)
    else:
        solver = ev.MccfrOsSolver(ctx, [(seed, walkers, epsilon) for seed in seeds]).run(1)
    best = None
    for _ in range(repeats):
        before = solver.counts(0)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        solver.run(1)
        t1.record()
        t1.synchronize()
        ms = t0.elapsed_time(t1)
        after = solver.counts(0)
        rec = {"ms": ms, "traversals": after[0] - before[0], "terminals": after[1] - before[1]}
        if best is None or ms < best["ms"]:
            best = rec
    name = "mccfr" if epsilon is None else "mccfr-vr" if baselines else "mccfr-os"
    best.update(game="leduc", solver=name, walkers=walkers, repeats=repeats,
                traversals_per_s=best["traversals"] / (best["ms"] * 1e-3),
                terminals_per_s=best["terminals"] / (best["ms"] * 1e-3))
    if epsilon is not None:
        best.update(epsilon=epsilon, hands=best["traversals"], hands_per_s=best["traversals_per_s"])
    if rule is not None:
        best.update(regret=rule[0], average=rule[1])
    if runs != 1:
        best.update(runs=runs)
    print(json.dumps(best), flush=True)
    solver.close()


def time_mccfr_net(ev, nat, sampling, cfg, init_seed, repeats=5, runs=1, hidden=64):
    """Regret nets (--regret-net --time): best of ``repeats`` single iterations of ``runs`` runs of ``cfg``
    (seeds cfg's .. + runs - 1) after a warm-up, and of the same iteration split by the handle's own HIP
    events (nfsp_mccfr_set_timing) into its two walks and its applies (k_mccfr_x_apply and k_mccfr_net_apply,
    twice each)."""
    import torch
    ctx = nat.Context(1, game=nat.GAME_LEDUC)
    cfgs = [(cfg[0] + k,) + tuple(cfg[1:]) for k in range(runs)]
    solver = ev.MccfrNetSolver(ctx, cfgs, sampling, [init_seed + k for k in range(runs)], hidden=hidden).run(1)
    best = None
    for _ in range(repeats):
        before = solver.counts(0)
        ev.mccfr_timings(solver, True)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        solver.run(1)
        t1.record()
        t1.synchronize()
        walk, applies, _ = ev.mccfr_timings(solver)
        after = solver.counts(0)
        rec = {"ms": t0.elapsed_time(t1), "ms_walk": walk, "ms_applies": applies,
               "traversals": after[0] - before[0], "terminals": after[1] - before[1]}
        if best is None or rec["ms"] < best["ms"]:
            best = rec
    best.update(game="leduc", solver=("mccfr", "mccfr-os", "mccfr-vr")[sampling], regret_net=True, walkers=cfg[1],
                repeats=repeats, regret=cfg[3], average=cfg[4], net_target=cfg[5], net_steps=cfg[6], net_loss=cfg[7],
                net_lr=cfg[8], net_momentum=cfg[9], net_init=init_seed, net_hidden=hidden,
                us_per_fit_step_upper=(1e3 * best["ms_applies"] / (2 * cfg[6]) if cfg[6] else None))
    if sampling:
        best.update(epsilon=cfg[2])
    if runs != 1:
        best.update(runs=runs)
    print(json.dumps(best), flush=True)
    solver.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="leduc", choices=["leduc", "kuhn"])
    ap.add_argument("--solver", default="cfr", choices=["cfr", "xfp", "mccfr", "mccfr-os", "mccfr-vr"])
    ap.add_argument("--iters", type=int, default=1024)
    ap.add_argument("--every", type=int, default=0, help="checkpoint every K iterations (default: 1, 2, 4, ...)")
    ap.add_argument("--eta", type=float, default=0.0, help="xfp: anticipatory parameter, in [0, 1)")
    ap.add_argument("--weight", default="uniform", choices=["uniform", "linear"], help="xfp: averaging weights")
    ap.add_argument("--runs", type=int, default=1, help="xfp: runs in one launch, eta spaced over [0, --eta]")
    ap.add_argument("--walkers", type=int, default=1024, help="mccfr: traversals per seat and iteration (even)")
    ap.add_argument("--seeds", type=int, default=1, help="mccfr: independent runs, seeds 1 .. K")
    ap.add_argument("--epsilon", type=float, default=0.6, help="mccfr-os, mccfr-vr: exploration rate, in [0.0625, 1]")
    ap.add_argument("--time", action="store_true",
                    help="mccfr, mccfr-os, mccfr-vr: traversals/s and terminals/s, Leduc at W = 2^20")
    ap.add_argument("--regret", default=None, choices=["plain", "plus"],
                    help="mccfr, mccfr-os, mccfr-vr: regret matching (plain) or regret matching+ (plus)")
    ap.add_argument("--average", default=None, choices=["uniform", "linear", "both"],
                    help="mccfr, mccfr-os, mccfr-vr: the average scored; both scores the two of every run")
    ap.add_argument("--time-walkers", type=int, default=1 << 20, help="--time: walkers of a run")
    ap.add_argument("--time-runs", type=int, default=1, help="--time: runs in the one handle")
    ap.add_argument("--regret-net", action="store_true",
                    help="mccfr, mccfr-os, mccfr-vr: hold the regrets in two 30-64-3 nets per run (sampled regression CFR)")
    ap.add_argument("--net-steps", type=int, default=32, help="--regret-net: full-batch steps per fit, 0 .. 4096")
    ap.add_argument("--net-lr", type=float, default=0.5, help="--regret-net: learning rate")
    ap.add_argument("--net-momentum", type=float, default=0.9, help="--regret-net: momentum, in [0, 1)")
    ap.add_argument("--net-target", default="avg", choices=["avg", "rowmax"], help="--regret-net: how R is scaled into targets")
    ap.add_argument("--net-loss", default="mse", choices=["mse", "huber"], help="--regret-net: the fit's loss")
    ap.add_argument("--net-init", type=int, default=1, metavar="SEED",
                    help="--regret-net: run k's nets are glorot_net(RandomState(SEED + k)), seat 0's then seat 1's")
    ap.add_argument("--net-hidden", type=int, default=64, choices=[16, 32, 64, 128],
                    help="--regret-net: the nets' hidden width, one per handle")
    ap.add_argument("--out", default=None, metavar="PATH")
    args = ap.parse_args()
    import __graft_entry__
    pkg = __graft_entry__.load_package()
    ev, nat = pkg.evaluation, pkg.native
    game = nat.GAME_KUHN if args.game == "kuhn" else nat.GAME_LEDUC
    rule = None                                         # (regret, average of the handle): nfsp_mccfr_x_create
    if args.regret is not None or args.average is not None:
        if args.solver not in ("mccfr", "mccfr-os", "mccfr-vr"):
            ap.error("--regret and --average are for --solver mccfr, mccfr-os and mccfr-vr")
        rule = (args.regret or "plain", "linear" if args.average == "both" else args.average or "uniform")
    both = args.average == "both"
    net = None                                          # the fit's part of a cfg: nfsp_mccfr_net_create
    if args.regret_net:
        if args.solver not in ("mccfr", "mccfr-os", "mccfr-vr"):
            ap.error("--regret-net is for --solver mccfr, mccfr-os and mccfr-vr")
        rule = rule or ("plain", "uniform")
        net = (args.net_target, args.net_steps, args.net_loss, args.net_lr, args.net_momentum)
    sampling = {"mccfr": 0, "mccfr-os": 1, "mccfr-vr": 2}.get(args.solver)
    if args.time and net is not None:
        eps = args.epsilon if sampling else 0.0
        return time_mccfr_net(ev, nat, sampling, (1, args.time_walkers, eps) + rule + net, args.net_init,
                              runs=args.time_runs, hidden=args.net_hidden)
    if args.time:
        if args.solver not in ("mccfr", "mccfr-os", "mccfr-vr"):
            ap.error("--time is for --solver mccfr, mccfr-os and mccfr-vr")
        return time_mccfr(ev, nat, None if args.solver == "mccfr" else args.epsilon, baselines=args.solver == "mccfr-vr",
                          rule=rule, walkers=args.time_walkers, runs=args.time_runs)
    ctx = nat.Context(1, game=game)
    xfp = args.solver == "xfp"
    outcome = args.solver in ("mccfr-os", "mccfr-vr")
    mccfr = args.solver == "mccfr" or outcome
    if net is not None:
        solver = ev.MccfrNetSolver(ctx, [(seed, args.walkers, args.epsilon if outcome else 0.0) + rule + net
                                         for seed in range(1, args.seeds + 1)], sampling,
                                   [args.net_init + k for k in range(args.seeds)], hidden=args.net_hidden)
    elif rule is not None:
        solver = ev.MccfrXSolver(ctx, [(seed, args.walkers, args.epsilon if outcome else 0.0) + rule
                                       for seed in range(1, args.seeds + 1)],
                                 {"mccfr": "es", "mccfr-os": "os", "mccfr-vr": "vr"}[args.solver])
    elif outcome:
        solver = (ev.MccfrVrSolver if args.solver == "mccfr-vr" else ev.MccfrOsSolver)(
            ctx, [(seed, args.walkers, args.epsilon) for seed in range(1, args.seeds + 1)])
    elif mccfr:
        solver = ev.MccfrSolver(ctx, [(seed, args.walkers) for seed in range(1, args.seeds + 1)])
    elif xfp:
        etas = [args.eta] if args.runs == 1 else [float(e) for e in np.linspace(0.0, args.eta, args.runs)]
        solver = ev.XfpSolver(ctx, [(e, args.weight) for e in etas])
    else:
        solver = ev.CfrSolver(ctx)
    rows = []
    done = 0
    while done < args.iters:
        nxt = min(args.iters, done + args.every if args.every else max(1, 2 * done))
        t0 = time.perf_counter()
        solver.run(nxt - done)
        ms = (time.perf_counter() - t0) * 1e3 / (nxt - done)
        done = nxt
        if mccfr:
            avgs = [solver.average(k) for k in range(solver.n)]
            res = ev.evaluate_batch(ctx, [(a, a) for a in avgs])
            r = res[0]
        elif xfp:
            avgs = [solver.average(k) for k in range(len(etas))]
            res = ev.evaluate_batch(ctx, [(a, a) for a in avgs])
            r = res[-1]
        else:
            eq = solver.average()
            r = ev.evaluate(ctx, eq, eq)
        rec = {"game": args.game, "iterations": done, "exploitability": r["exploitability"], "br0": r["br0"],
               "br1": r["br1"], "value0": r["value0"],
               "value0_dealer": [r["value0_dealer0"], r["value0_dealer1"]], "ms_per_iteration": ms}
        if mccfr:
            counts = [solver.counts(k) for k in range(solver.n)]
            rec.update(solver=args.solver, walkers=args.walkers, traversals=counts[0][0],
                       terminals=[c[1] for c in counts], exploitability_runs=[x["exploitability"] for x in res])
        if outcome:
            rec.update(hands=counts[0][0], epsilon=args.epsilon)
        if rule is not None:
            rec.update(regret=rule[0], average=args.average or "uniform")
        if net is not None:
            cur = ev.evaluate_batch(ctx, [(c, c) for c in (solver.current(k) for k in range(solver.n))])
            tv = [solver.sigma_tv(k).tolist() for k in range(solver.n)]
            rec.update(regret_net=True, net_target=net[0], net_steps=net[1], net_loss=net[2], net_lr=net[3],
                       net_momentum=net[4], net_init=args.net_init, net_hidden=solver.hidden, exploitability_current=cur[0]["exploitability"],
                       exploitability_current_runs=[x["exploitability"] for x in cur], sigma_tv=tv[0], sigma_tv_runs=tv,
                       fit_loss=solver.fit_loss(0).tolist(),
                       fit_loss_runs=[solver.fit_loss(k).tolist() for k in range(solver.n)])
        if both:
            uni = ev.evaluate_batch(ctx, [(a, a) for a in (solver.average(k, "uniform") for k in range(solver.n))])
            rec.update(exploitability_runs_uniform=[x["exploitability"] for x in uni],
                       exploitability_runs_linear=rec["exploitability_runs"])
        if xfp:
            rec.update(solver="xfp", weight=args.weight, eta=etas[-1])
            if len(etas) > 1:
                rec.update(eta_runs=etas, exploitability_runs=[x["exploitability"] for x in res])
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        extra = {}
        if mccfr:
            extra = {"tables": np.stack([solver.average_table(k) for k in range(solver.n)]),
                     "traversals": np.array([r["traversals"] for r in rows]),
                     "terminals": np.array([r["terminals"] for r in rows])}
        if xfp:
            extra = {"tables": np.stack([solver.average_table(k) for k in range(len(etas))]), "eta": np.array(etas),
                     "weight": args.weight}
        np.savez(args.out, table=solver.average_table(len(etas) - 1) if xfp else solver.average_table(),
                 game=args.game,
                 iterations=np.array([r["iterations"] for r in rows]),
                 exploitability=np.array([r["exploitability"] for r in rows]),
                 br0=np.array([r["br0"] for r in rows]), br1=np.array([r["br1"] for r in rows]),
                 value0=np.array([r["value0"] for r in rows]),
                 value0_dealer=np.array([r["value0_dealer"] for r in rows]), **extra)
    solver.close()


if __name__ == "__main__":
    main()

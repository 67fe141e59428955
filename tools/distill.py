#!/usr/bin/env python3
"""The capacity table of the 30-H-3 nets ("Nets fitted to tables"; H = 64 unless
--hidden says otherwise): what the AR
net and the Q heads reach when they are fitted to exact tables with exact weights, full batch, on
the device (nfsp_fit_tables) -- the approximation floors under NFSP's sampled, minibatch fits.

    python tools/distill.py --game leduc --iters 2000 --steps 500,2000,8000,32000 --lr 0.5,1.0 --inits 4

* policy: two softmax nets fitted to the CFR+ average of --iters iterations with visit weights
  (diagnostics.distill_policy); per step count, rate and init seed the exact exploitability of the
  nets (softmax and argmax) beside the table's.  Every (rate, seed) of a step count is one batch.
* --q: the ReLU and the linear Q head fitted to the exact action values against that average
  (diagnostics.distill_q, --q-loss, --q-lr): q_rmse_exact, greedy_mismatch_share and the greedy
  policy's br_gap.
* --checkpoint PATH: the target is M_SL's own mass table of that engine checkpoint with its counts
  as weights -- the full-batch limit of what the AR chain approaches -- beside the checkpoint's AR
  nets and the table itself.
* --time: microseconds per step of k_fit_tables for 1 and 64 jobs (HIP events, best of 5 after a
  warm-up, the difference of a long and a short call so that the call's fixed cost drops out), and
  the same rows through nfsp_mlp_fit in <= 64-row minibatches (unweighted: a time comparison only).

* --hidden 16,32,64,128: every table above once per hidden width (nfsp_fit_tables_h; the nets of a
  width other than 64 are scored through evaluation.net_policy), a "hidden" column in every row;
  with --time the step times per width too.

JSON goes to profiles/distill/ (--out).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def floats(s):
    return [float(x) for x in s.split(",")]


def event_ms(torch, fn, reps=5):
    fn()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def fit_step_times(pkg, torch, ctx, tree, hidden=64, short=1000, long=5000):
    """us per step of the fit kernel of that width for 1 and 64 jobs: the difference of two calls"""
    import numpy as np
    ev, nat = pkg.evaluation, pkg.native
    rng = np.random.RandomState(0)
    table = tree.remap(rng.dirichlet(np.ones(3), size=(tree.ndec, 3)))
    out = {}
    for n in (1, 64):
        def call(steps, n=n):
            jobs = [ev.FitJob(ev.glorot_net(np.random.RandomState(k), hidden), table, k & 1, nat.ACT_SOFTMAX, "ce", 0.1,
                              0.9) for k in range(n)]
            return lambda: ev.fit_tables(ctx, jobs, steps, tree)
        t0, t1 = event_ms(torch, call(short)), event_ms(torch, call(long))
        out[f"fit_tables_us_per_step_{n}"] = 1e3 * (t1 - t0) / (long - short)
        out[f"fit_tables_call_ms_{n}_jobs_{short}_steps"] = t0
    out["ratio_64_over_1"] = out["fit_tables_us_per_step_64"] / out["fit_tables_us_per_step_1"]
    return out


def step_times(pkg, torch, ctx, tree, short=1000, long=5000):
    import numpy as np
    ev, nat = pkg.evaluation, pkg.native
    rng = np.random.RandomState(0)
    table = tree.remap(rng.dirichlet(np.ones(3), size=(tree.ndec, 3)))
    out = fit_step_times(pkg, torch, ctx, tree, 64, short, long)
    # the parent's own path: one net through nfsp_mlp_fit, the seat's rows in <= 64-row minibatches
    d = np.nonzero(tree.seat == 0)[0]
    rows = len(d) * 3
    x = ((tree.obs[d].reshape(-1)[:, None] >> np.arange(30, dtype=np.uint32)) & 1).astype(np.float32)
    t = table[d].reshape(-1, 3).astype(np.float32)
    xd, tdv = torch.as_tensor(x, device="cuda"), torch.as_tensor(t, device="cuda")
    w = torch.as_tensor(ev.glorot_net(np.random.RandomState(0)), device="cuda")

    def mlp(epochs):
        perm = torch.as_tensor(np.tile(np.arange(rows, dtype=np.int32), epochs), device="cuda")

        def go():
            nat.check(ctx.L.nfsp_mlp_fit(ctx.h, nat.ptr(w), 64, nat.ACT_SOFTMAX, nat.ptr(xd), nat.ptr(tdv), rows,
                                         nat.ptr(perm), epochs, min(64, rows), 0.01), "nfsp_mlp_fit")
            ctx.call("nfsp_synchronize")
        return go
    e0, e1 = 50, 250
    m0, m1 = event_ms(torch, mlp(e0)), event_ms(torch, mlp(e1))
    out["mlp_fit_us_per_pass"] = 1e3 * (m1 - m0) / (e1 - e0)
    out["mlp_fit_minibatches_per_pass"] = -(-rows // 64)
    out["rows"] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="leduc", choices=["leduc", "kuhn"])
    ap.add_argument("--iters", type=int, default=2000, help="CFR+ iterations of the target")
    ap.add_argument("--steps", default="500,2000,8000,32000")
    ap.add_argument("--lr", default="0.5,1.0")
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--inits", type=int, default=4, help="Glorot seeds 1..N")
    ap.add_argument("--weights", default="visit", choices=["visit", "uniform"])
    ap.add_argument("--q", action="store_true")
    ap.add_argument("--q-lr", default="0.02,0.05")
    ap.add_argument("--q-loss", default="mse", choices=["mse", "huber"])
    ap.add_argument("--checkpoint", default=None, metavar="PATH")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--hidden", default="64", help="hidden widths, comma separated: 16, 32, 64, 128")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__
    pkg = __graft_entry__.load_package()
    nat, ev, dg = pkg.native, pkg.evaluation, pkg.diagnostics
    game = nat.GAME_KUHN if args.game == "kuhn" else nat.GAME_LEDUC
    steps = [int(x) for x in args.steps.split(",")]
    widths = [int(x) for x in args.hidden.split(",")]
    for h in widths:
        nat.net_params(h)
    seeds = list(range(1, args.inits + 1))
    out = {"game": args.game, "momentum": args.momentum, "weights": args.weights, "hidden": widths, "policy": [], "q": []}

    def grid(lrs):
        return [lr for lr in lrs for _ in seeds], [s for _ in lrs for s in seeds]

    if args.checkpoint:
        eng = pkg.engine.SelfPlayEngine.from_checkpoint(args.checkpoint)
        ctx, tree = eng.ctx, ev.GameTree.of(eng.ctx.game)
        sl, _ = eng.memory_table(nat.MEM_SL)
        target, weights = sl.policy("mass"), sl.n.astype(np.float64)
        out.update({"target": "M_SL mass table of " + os.path.basename(args.checkpoint),
                    "ar_nets_exploitability": eng.exploitability()["exploitability"],
                    "sl_empty_sets": int((sl.n == 0).sum())})
    else:
        ctx = nat.Context(1, game=game)
        tree = ev.GameTree.of(game)
        solver = ev.CfrSolver(ctx).run(args.iters)
        target, weights = solver.average(), args.weights
        out["target"] = f"CFR+ average, {args.iters} iterations"
    lrs, sd = grid(floats(args.lr))
    for hidden, n in [(h, n) for h in widths for n in steps]:
        res = dg.distill_policy(ctx, target, weights, n, lrs, args.momentum, sd, tree, hidden)
        out["table_exploitability"] = res[0]["scores"]["table"]
        for lr, seed, r in zip(lrs, sd, res):
            row = {"hidden": hidden, "steps": n, "lr": lr, "seed": seed, "softmax": r["scores"]["softmax"], "argmax": r["scores"]["argmax"],
                   "loss_minus_entropy": [float(r["losses"][s, 1] - r["entropy"][s]) for s in (0, 1)]}
            out["policy"].append(row)
            print(json.dumps(row), flush=True)
    if args.q and not args.checkpoint:
        lrs, sd = grid(floats(args.q_lr))
        for hidden, linear in [(h, lin) for h in widths for lin in (False, True)]:
            for n in steps:
                res = dg.distill_q(ctx, target, linear, args.q_loss, n, lrs, args.momentum, sd, tree, hidden)
                for lr, seed, r in zip(lrs, sd, res):
                    row = {"hidden": hidden, "head": "linear" if linear else "relu", "loss": args.q_loss, "steps": n, "lr": lr, "seed": seed,
                           "q_rmse_exact": [x["q_rmse_exact"] for x in r["reports"]],
                           "greedy_mismatch_share": [x["greedy_mismatch_share"] for x in r["reports"]],
                           "relu_blind_share": [x["relu_blind_share"] for x in r["reports"]],
                           "br_gap": [x["gap"] for x in r["br_gap"]], "fit_loss": r["losses"][:, 1].tolist()}
                    out["q"].append(row)
                    print(json.dumps(row), flush=True)
    if args.time:
        out["time"] = step_times(pkg, torch, ctx, tree)
        print(json.dumps(out["time"]), flush=True)
        for h in widths:
            if h != 64:
                out[f"time_hidden_{h}"] = fit_step_times(pkg, torch, ctx, tree, h)
                print(json.dumps({"hidden": h, **out[f"time_hidden_{h}"]}), flush=True)
    path = args.out or os.path.join(REPO, "profiles", "distill", f"capacity_{args.game}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path, file=sys.stderr)


if __name__ == "__main__":
    main()

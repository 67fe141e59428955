#!/usr/bin/env python3
"""A tabular equilibrium of the game as the engine plays it: CFR+ on the evaluator's tree
(evaluation.CfrSolver, csrc/cfr.hip), scored by the evaluator itself (nfsp_evaluate_batch).

    python tools/solve_game.py --game leduc --iters 4096 --out eq.npz

eq.npz holds ``table`` [ndec, 3 ranks, 3 actions] (rows as evaluation.GameTree's; usable as
evaluation.Policy.table), ``game``, and per checkpoint (--every, doubling by default)
``iterations``, ``exploitability``, ``br0`` / ``br1``, ``value0`` and ``value0_dealer`` [k, 2]:
what seat 0 wins per hand when it deals / when seat 1 deals.  The game value per dealer lies
within the exploitability of that row.  One JSON line per checkpoint goes to stdout, with the
solver's milliseconds per iteration.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="leduc", choices=["leduc", "kuhn"])
    ap.add_argument("--iters", type=int, default=1024)
    ap.add_argument("--every", type=int, default=0, help="checkpoint every K iterations (default: 1, 2, 4, ...)")
    ap.add_argument("--out", default=None, metavar="PATH")
    args = ap.parse_args()
    import __graft_entry__
    pkg = __graft_entry__.load_package()
    ev, nat = pkg.evaluation, pkg.native
    game = nat.GAME_KUHN if args.game == "kuhn" else nat.GAME_LEDUC
    ctx = nat.Context(1, game=game)
    solver = ev.CfrSolver(ctx)
    rows = []
    done = 0
    while done < args.iters:
        nxt = min(args.iters, done + args.every if args.every else max(1, 2 * done))
        t0 = time.perf_counter()
        solver.run(nxt - done)
        ms = (time.perf_counter() - t0) * 1e3 / (nxt - done)
        done = nxt
        eq = solver.average()
        r = ev.evaluate(ctx, eq, eq)
        rec = {"game": args.game, "iterations": done, "exploitability": r["exploitability"], "br0": r["br0"],
               "br1": r["br1"], "value0": r["value0"],
               "value0_dealer": [r["value0_dealer0"], r["value0_dealer1"]], "ms_per_iteration": ms}
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        np.savez(args.out, table=solver.average_table(), game=args.game,
                 iterations=np.array([r["iterations"] for r in rows]),
                 exploitability=np.array([r["exploitability"] for r in rows]),
                 br0=np.array([r["br0"] for r in rows]), br1=np.array([r["br1"] for r in rows]),
                 value0=np.array([r["value0"] for r in rows]),
                 value0_dealer=np.array([r["value0_dealer"] for r in rows]))
    solver.close()


if __name__ == "__main__":
    main()

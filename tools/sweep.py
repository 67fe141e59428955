#!/usr/bin/env python3
"""A hyperparameter sweep in one launch: every grid point x seed is a replica of ONE
heterogeneous engine group (EngineGroup(cfgs=...), nfsp_group_create_v), each
replica bit-identical to a standalone engine with its cfg.  Every K steps all replicas are
scored with the exact exploitability (one launch, exploitability_all); one JSON line per
checkpoint: hands per replica, the per-replica exploitability (the package's sweep.expand_grid
order: grid-major, seed-minor) and per grid point its mean and standard deviation over seeds.

    python tools/sweep.py --grid lr_ar=0.1,0.02 lr_br=0.05,0.01 --seeds 4 --steps 64 --every 8 \\
        --paired-init > sweep.jsonl

--set gives the fields every replica shares (the group's shape), e.g. C3's memories at 16
replicas of 65,536 lanes: --set n_lanes=65536 --set rl_capacity=200000 --set sl_capacity=2000000.
--time adds the wall ms per step of the steps since the previous line (each bracketed by device
syncs, evaluations outside); --save F writes the group's checkpoint after the last step.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def number(v: str):
    return float(v) if any(c in v for c in ".eE") and not v.lower().startswith("0x") else int(v, 0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", nargs="+", required=True, metavar="KEY=V1,V2,..",
                    help="swept cfg fields (seed, eta, lr_br, lr_ar, gamma, epsilon, target_every, quirks)")
    ap.add_argument("--seeds", type=int, default=1, help="seeds per grid point (seed = base seed + s)")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--paired-init", action="store_true",
                    help="seed s of every grid point starts from the same initial nets")
    ap.add_argument("--set", action="append", default=[], metavar="KEY=VALUE",
                    help="a cfg field shared by every replica (default: n_lanes=4096, M_RL / M_SL 40000)")
    ap.add_argument("--game", default="leduc", choices=["leduc", "kuhn"])
    ap.add_argument("--save", default=None, metavar="F", help="checkpoint the group after the last step")
    ap.add_argument("--time", action="store_true", help="add wall ms per step to every line")
    args = ap.parse_args()
    base = dict(n_lanes=4096, rl_capacity=40_000, sl_capacity=40_000)
    for kv in args.set:
        k, v = kv.split("=", 1)
        base[k] = number(v)
    grid = {}
    for kv in args.grid:
        k, v = kv.split("=", 1)
        grid[k] = [number(x) for x in v.split(",") if x]
    import torch
    import __graft_entry__
    pkg = __graft_entry__.load_package()
    try:
        cfgs, init_seeds, labels = pkg.sweep.expand_grid(grid, args.seeds, base, args.paired_init)
    except ValueError as ex:
        ap.error(str(ex))
    game = pkg.native.GAME_KUHN if args.game == "kuhn" else pkg.native.GAME_LEDUC
    g = pkg.engine.EngineGroup(cfgs=cfgs, init_seeds=init_seeds, game=game)
    points = [{k: v for k, v in lab.items() if k not in ("point", "seed_index")} for lab in labels[::args.seeds]]
    print(json.dumps({"sweep": {"grid": grid, "seeds": args.seeds, "paired_init": args.paired_init, "base": base,
                                "replicas": g.R, "points": points, "labels": labels, "init_seeds": init_seeds}}),
          flush=True)
    timed = {"s": 0.0, "n": 0}

    def report(step):
        torch.cuda.synchronize()
        ex = [e["exploitability"] for e in g.exploitability_all(0)]
        stats = pkg.sweep.point_stats(ex, args.seeds)
        rec = {"step": step, "hands": int(g.replicas[0].stats()["hands"]), "exploitability": ex,
               "points": [dict(p, mean=m, std=sd) for p, (m, sd) in zip(points, stats)]}
        if args.time and timed["n"]:
            rec["ms_per_step"] = timed["s"] / timed["n"] * 1e3
            timed["s"], timed["n"] = 0.0, 0
        print(json.dumps(rec), flush=True)

    report(0)
    for k in range(1, args.steps + 1):
        if args.time:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.step()
            torch.cuda.synchronize()
            timed["s"] += time.perf_counter() - t0
            timed["n"] += 1
        else:
            g.step()
        if k % args.every == 0 or k == args.steps:
            report(k)
    if args.save:
        g.save(args.save)
    g.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The memory tables' cost (csrc/memtab.hip): records only, nothing is gated.

    python tools/memtab_bench.py --part a --out profiles/memtab/c3.json
    python tools/memtab_bench.py --part c --out profiles/memtab/c3_r16.json

Every table time is the two kernels' (k_memtab + k_memtab_sum) under HIP events recorded around
them (nfsp_memtab_last_ms): one warm-up launch, then the best of --repeats.  The states are tens
of MB, under the 256 MiB Infinity Cache, so launches after the first may be served from it and
not from HBM -- as the state digest's beside them (nfsp_engine_state_digest_timed).

  a  a C3 engine stepped until M_SL is full (at most --max-steps): the M_SL and M_RL tables' ms and
     bytes read / time, the state digest on the same engine in the same process (the existing
     read-once pass over the same records), one memory_report() against one step; then
  b  synthetic M_SL records at the same n with keys uniform over a seat's sets and all in one
     set: the two ends of the contention on the LDS bins.  (profiles/memtab/schemes_c3.json is
     this part run while two more aggregation schemes were compiled in)
     With --td (profiles/qreport/): also the TD table (nfsp_engine_td_table: a forward of the target
     net per record inside k_memtab) beside the M_RL table on the same state, and one q_report();
     part b is skipped.  --quirks picks the reference's quirks or NFSP_TEXTBOOK_MSE_DECAY.
     With --tdq (profiles/tabular/): as --td, and beside both the TD pass whose bootstrap reads a
     table (nfsp_engine_tabular_q): one sweep -- k_memtab<TDQ>, k_memtab_sum and k_table_rows under
     the same events -- and the tree's nlev sweeps; then one install_tabular_br() and one
     install_tabular_ar() by the wall clock, against one step.
  c  the c3_r16 group (16 replicas x 65,536 lanes, each M_RL 200k + M_SL 2M): the group form
     against 16 engine-form calls."""
import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

def last_ms(pkg):
    ms = pkg.native.F64()
    pkg.native.check(pkg.native.load().nfsp_memtab_last_ms(C.byref(ms)), "nfsp_memtab_last_ms")
    return ms.value


def timed(pkg, call, repeats):
    call()                                   # warm-up (the first also loads the code object)
    first = last_ms(pkg)
    runs = []
    for _ in range(repeats):
        call()
        runs.append(last_ms(pkg))
    return dict(ms_first=first, ms_runs=runs, ms_best=min(runs))


def rate(t, nbytes):
    t["bytes"] = int(nbytes)
    t["bytes_per_s"] = nbytes / (t["ms_best"] * 1e-3)
    return t


def part_a(pkg, args, torch):
    import numpy as np
    nat, ev = pkg.native, pkg.evaluation
    quirks = nat.QUIRKS_REFERENCE if args.quirks == "reference" else nat.TEXTBOOK_MSE_DECAY
    eng = pkg.engine.SelfPlayEngine(n_lanes=args.lanes, slices=args.slices, slice_lag=2 if args.slices > 1 else 1,
                                    rl_capacity=args.rl_capacity, sl_capacity=args.sl_capacity, quirks=quirks)
    steps, step_ms = 0, None
    while steps < args.max_steps:
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.step()
        torch.cuda.synchronize()
        step_ms = (time.perf_counter() - t) * 1e3
        steps += 1
        if steps >= 2 and min(eng.stats()["sl_size"]) >= args.sl_capacity:
            break
    st = eng.stats()
    out = {"steps": steps, "step_ms": step_ms, "rl_size": st["rl_size"], "sl_size": st["sl_size"], "quirks": args.quirks}
    for kind, name, rec, n in ((nat.MEM_SL, "sl", 16, sum(st["sl_size"])), (nat.MEM_RL, "rl", 32, sum(st["rl_size"]))):
        out[name] = rate(timed(pkg, lambda: eng.memory_table(kind), args.repeats), rec * n)
        # M_RL: the kernel reads the first 16 bytes of each 32-byte record; the bytes are the records'
    if args.td or args.tdq:
        out["td"] = rate(timed(pkg, lambda: eng.td_table(), args.repeats), 32 * sum(st["rl_size"]))
        out["td_over_rl"] = out["td"]["ms_best"] / out["rl"]["ms_best"]
        torch.cuda.synchronize()
        t = time.perf_counter()
        rep = eng.q_report()
        out["q_report_ms"] = (time.perf_counter() - t) * 1e3
        out["q_report_over_step"] = out["q_report_ms"] / step_ms
        out["q_report"] = [{k: v for k, v in r.items() if k != "info"} for r in rep]
        if args.tdq:
            nlev = ev.GameTree.of(eng.ctx.game).nlev
            out["tdq_sweep"] = rate(timed(pkg, lambda: eng.tabular_q(sweeps=1), args.repeats), 32 * sum(st["rl_size"]))
            out["tdq_over_td"] = out["tdq_sweep"]["ms_best"] / out["td"]["ms_best"]
            out["tdq_over_rl"] = out["tdq_sweep"]["ms_best"] / out["rl"]["ms_best"]
            out["tdq_nlev"] = dict(sweeps=nlev, **timed(pkg, lambda: eng.tabular_q(), args.repeats))
            for name, call in (("install_tabular_br", eng.install_tabular_br), ("install_tabular_ar", eng.install_tabular_ar)):
                call()
                wall = []
                for _ in range(args.repeats):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    call()
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t) * 1e3)
                out[name + "_ms"] = min(wall)
                out[name + "_over_step"] = min(wall) / step_ms
            rep = eng.tabular_q_report()
            out["tabular_q_report"] = [{k: v for k, v in r.items() if k != "info"} for r in rep]
            eng.clear_act_tables()
        out["exploitability"] = eng.exploitability()["exploitability"]
        out["br_gap"] = [g["gap"] for g in eng.br_gap()]
        eng.close()
        return out
    d0, first, _ = eng.state_digest_timed()
    runs = []
    for _ in range(args.repeats):
        d, ms, nbytes = eng.state_digest_timed()
        runs.append(ms)
    out["digest"] = rate(dict(ms_first=first, ms_runs=runs, ms_best=min(runs)), nbytes)
    torch.cuda.synchronize()
    t = time.perf_counter()
    rep = eng.memory_report()
    out["report_ms"] = (time.perf_counter() - t) * 1e3
    out["report_over_step"] = out["report_ms"] / step_ms
    out["report"] = {k: v for k, v in rep.items() if not isinstance(v, list)}
    # real M_SL's skew: the share of the records in the most populated sets
    sl, _ = eng.memory_table(nat.MEM_SL)
    share = np.sort(sl.n.reshape(-1))[::-1] / max(1, sl.n.sum())
    out["sl_key_share_top1_top6_top24"] = [float(share[:1].sum()), float(share[:6].sum()), float(share[:24].sum())]

    # b: synthetic M_SL at the same n
    n = int(st["sl_size"][0])
    tree = ev.GameTree(eng.ctx.game)
    keys = np.array(sorted(o for (s, o) in tree._rows if s == 0), np.uint32)
    rng = np.random.RandomState(1)
    words = np.zeros((n, 4), np.uint32)
    hot = np.eye(3, dtype=np.float32)[rng.randint(3, size=n)]
    draw = rng.rand(n, 3).astype(np.float32)
    words[:, 1:] = np.where((rng.rand(n) < 0.5)[:, None], hot, draw).view(np.uint32)
    synth = {}
    for dist in ("uniform", "one_set"):
        words[:, 0] = keys[rng.randint(len(keys), size=n)] if dist == "uniform" else keys[0]
        recs = torch.from_numpy(words.view(np.int32)).cuda()
        got = {}

        def call():
            got["info"] = ev.memory_table(eng.ctx, nat.MEM_SL, 0, recs, tree=tree)[1]
        synth[dist] = rate(timed(pkg, call, args.repeats), 16 * n)
        assert got["info"]["matched"] == n
    out["synthetic_sl"] = dict(n=n, runs=synth)
    eng.close()
    return out


def part_c(pkg, args, torch):
    nat = pkg.native
    R = args.replicas
    grp = pkg.engine.EngineGroup(R, n_lanes=args.lanes // R, rl_capacity=args.rl_capacity,
                                 sl_capacity=args.sl_capacity, avg_ar=True)
    grp.average_ar()
    for _ in range(args.group_steps):
        grp.step()
    torch.cuda.synchronize()
    st = [e.stats() for e in grp.replicas]
    out = {"replicas": R, "steps": args.group_steps, "sl_size_total": sum(sum(s["sl_size"]) for s in st),
           "rl_size_total": sum(sum(s["rl_size"]) for s in st)}
    for kind, name, rec, n in ((nat.MEM_SL, "sl", 16, out["sl_size_total"]), (nat.MEM_RL, "rl", 32, out["rl_size_total"])):
        out[name + "_group"] = rate(timed(pkg, lambda: grp.memory_tables(kind), args.repeats), rec * n)

        def each():
            tot = 0.0
            for e in grp.replicas:
                e.memory_table(kind)
                tot += last_ms(pkg)
            return tot
        each()
        runs, wall = [], []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            runs.append(each())
            wall.append((time.perf_counter() - t) * 1e3)
        out[name + "_engines"] = dict(kernel_ms_runs=runs, kernel_ms_best=min(runs), wall_ms_best=min(wall))
        torch.cuda.synchronize()
        t = time.perf_counter()
        grp.memory_tables(kind)
        out[name + "_group"]["wall_ms"] = (time.perf_counter() - t) * 1e3
    grp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="a", choices=["a", "c"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=1_048_576)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--rl-capacity", type=int, default=200_000)
    ap.add_argument("--sl-capacity", type=int, default=2_000_000)
    ap.add_argument("--max-steps", type=int, default=12)
    ap.add_argument("--replicas", type=int, default=16)
    ap.add_argument("--group-steps", type=int, default=3)
    ap.add_argument("--td", action="store_true", help="part a: the TD table beside the M_RL table, and one q_report()")
    ap.add_argument("--tdq", action="store_true",
                    help="part a: --td, and the table-bootstrapped TD pass, its sweeps and the two installs beside it")
    ap.add_argument("--quirks", default="reference", choices=["reference", "textbook"],
                    help="part a: NFSP_QUIRKS_REFERENCE or NFSP_TEXTBOOK_MSE_DECAY")
    args = ap.parse_args()
    import torch
    import __graft_entry__
    pkg = __graft_entry__.load_package()
    out = {"what": "k_memtab + k_memtab_sum (HIP events around the two kernels), part " + args.part,
           "device": torch.cuda.get_device_name(0),
           "config": dict(n_lanes=args.lanes, slices=args.slices, rl_capacity=args.rl_capacity,
                          sl_capacity=args.sl_capacity),
           "note": "every state here is under the 256 MiB Infinity Cache: launches after the first may be served "
                   "from it rather than from HBM; the first also loads the code object"}
    out.update(part_a(pkg, args, torch) if args.part == "a" else part_c(pkg, args, torch))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

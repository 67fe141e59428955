#!/usr/bin/env python3
"""Checkpoint costs at C3 size: the state digest kernel's time against HBM
bandwidth, and save / load as fractions of one C3 step taken in the same process.

    python tools/ckpt_bench.py --out profiles/ckpt/digest_c3.json

A C3 engine (bench.py's config: 1,048,576 lanes in 16 pipelined slices, M_RL 200k, M_SL 2M)
runs 2 steps; the second is timed (host clock around step + synchronise).  The digest is
launched once to warm up, then --repeats times under HIP events recorded around its two
kernels (nfsp_engine_state_digest_timed); bytes = what the kernels read (EngineDev, the nets,
the live M_RL records, the M_SL rows).  Save = nfsp_engine_save_state into host memory, and
separately the file write; load = nfsp_engine_load_state from host memory, including its
digest check.  Not gated: these are records."""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12         # bytes/s, MI355X HBM3E spec
HBM_ACHIEVABLE = 6.3e12   # float4 copy, measured


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=1_048_576)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--rl-capacity", type=int, default=200_000)
    ap.add_argument("--sl-capacity", type=int, default=2_000_000)
    args = ap.parse_args()
    import torch
    import __graft_entry__
    pkg = __graft_entry__.load_package()
    ck = pkg.checkpoint
    eng = pkg.engine.SelfPlayEngine(n_lanes=args.lanes, slices=args.slices, slice_lag=2 if args.slices > 1 else 1,
                                    rl_capacity=args.rl_capacity, sl_capacity=args.sl_capacity)
    eng.step()
    torch.cuda.synchronize()
    t = time.perf_counter()
    eng.step()
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t) * 1e3
    st = eng.stats()

    d0, first_ms, _ = eng.state_digest_timed()            # warm-up launch (loads the code object)
    runs = []
    for _ in range(args.repeats):
        d, ms, nbytes = eng.state_digest_timed()
        assert d == d0
        runs.append(ms)
    best = min(runs)

    t = time.perf_counter()
    blob = ck._blob(eng)
    save_ms = (time.perf_counter() - t) * 1e3
    assert tuple(ck.check(blob).digest) == d0
    with tempfile.TemporaryDirectory() as tmp:
        t = time.perf_counter()
        eng.save(os.path.join(tmp, "c3.nfsp"))
        save_file_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    ck.load_bytes(eng, blob)
    load_ms = (time.perf_counter() - t) * 1e3
    assert eng.state_digest() == d0

    out = {
        "what": "k_state_digest + k_state_digest_sum on a C3 engine after 2 steps; save / load of its state",
        "device": torch.cuda.get_device_name(0),
        "config": dict(n_lanes=args.lanes, slices=args.slices, rl_capacity=args.rl_capacity,
                       sl_capacity=args.sl_capacity),
        "rl_size": st["rl_size"], "sl_size": st["sl_size"],
        "digest_bytes": nbytes, "digest_ms_first": first_ms, "digest_ms_runs": runs, "digest_ms_best": best,
        "note": "the state (tens of MB) fits the 256 MiB Infinity Cache, so launches after the first "
                "may be served from it rather than from HBM; the first also loads the code object",
        "digest_bytes_per_s": nbytes / (best * 1e-3),
        "share_of_hbm_peak_8TBps": nbytes / (best * 1e-3) / HBM_PEAK,
        "share_of_hbm_achievable_6p3TBps": nbytes / (best * 1e-3) / HBM_ACHIEVABLE,
        "blob_bytes": int(blob.size),
        "step_ms": step_ms,
        "save_ms": save_ms, "save_to_file_ms": save_file_ms, "load_ms": load_ms,
        "save_over_step": save_ms / step_ms, "save_to_file_over_step": save_file_ms / step_ms,
        "load_over_step": load_ms / step_ms,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

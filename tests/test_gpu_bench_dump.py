"""bench.py --dump-outputs and the plain / --full split.

dump_outputs writes what the timed steps left with their caller (nets, counters, the last
rollout's lane counts, a fixed sample of the memories' rows) as float32 / float64 .npy files;
the engine's seeds are fixed, so the same arguments give the same files, and the files hold what
the engine's own accessors return.  A plain `bench.py` run prints the headline line without any
of the side measurements; they are behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(n_lanes=2048, slices=4, slice_lag=2, rl_capacity=3000, sl_capacity=2000)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _names(tag=""):
    per_agent = [f"{t}_{c}_a{a}" for a in (0, 1)
                 for t, cols in (("rl", ("rows", "s", "a", "r", "s2", "t")), ("sl", ("rows", "s", "a"))) for c in cols]
    return {tag + n for n in ["weights", "stats", "lane_counts", *per_agent]}


def test_dump_is_what_the_engine_holds_and_repeats(pkg, tmp_path):
    import bench
    dirs = []
    for k in range(2):
        eng = pkg.engine.SelfPlayEngine(seed=1234, init_seed=0, **SMALL)
        for _ in range(3):
            eng.step()
        d = str(tmp_path / f"run{k}")
        written = bench.dump_outputs(eng, d)
        dirs.append(d)
        if k == 0:
            got = _load(d)
            assert set(got) == set(written) == _names()
            assert all(a.dtype in (np.float32, np.float64) for a in got.values())
            assert sum(a.nbytes for a in got.values()) <= 64 << 20
            w = np.stack([np.stack([eng.get_weights(a, n) for n in (0, 1, 2)]) for a in (0, 1)])
            assert np.array_equal(got["weights"], w) and got["weights"].dtype == np.float32
            st = eng.stats()
            assert got["stats"][0] == st["hands"] == 3 * 2048
            assert np.array_equal(got["lane_counts"], eng.lane_counts())
            for a in (0, 1):
                mem = eng.memories(a)
                torch.cuda.synchronize()
                rows = got[f"rl_rows_a{a}"].astype(np.int64)
                assert len(rows) == min(mem["log_cap"], st["rl_total"][a], bench.DUMP_ROWS) > 0
                assert np.array_equal(got[f"rl_s2_a{a}"], mem["rl_s2"].cpu().numpy()[rows])
                assert np.array_equal(got[f"rl_t_a{a}"], mem["rl_t"].cpu().numpy()[rows].astype(np.float32))
                rows = got[f"sl_rows_a{a}"].astype(np.int64)
                assert len(rows) == min(st["sl_size"][a], bench.DUMP_ROWS) > 0
                assert np.array_equal(got[f"sl_a_a{a}"], mem["sl_a"].cpu().numpy()[rows])
        eng.close()
    a, b = _load(dirs[0]), _load(dirs[1])
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_dump_of_a_group_names_every_replica(pkg, tmp_path):
    import bench
    g = pkg.engine.EngineGroup(2, seed=1234, init_seed=0, avg_ar=True, **SMALL)
    g.step()
    written = bench.dump_outputs(g, str(tmp_path))
    assert set(written) == _names("r0_") | _names("r1_")
    got = _load(str(tmp_path))
    assert np.array_equal(got["r1_weights"][0, 1], g.replicas[1].get_weights(0, 1))
    assert not np.array_equal(got["r0_weights"][0, 1], got["r1_weights"][0, 1])
    assert len(got["r0_rl_rows_a0"]) <= bench.DUMP_ROWS // 2
    g.close()


def test_plain_run_prints_the_headline_only(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` (here at C2): the line says what the K timed steps
    took and nothing that needs a run of its own; --dump-outputs writes the files it lists."""
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "c2", "--dump-outputs", d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1
    out = lines[0]
    assert out["metric"] == "Leduc self-play hands/sec" and out["unit"] == "hands/s" and out["dtype"] == "fp32"
    assert out["higher_is_better"] is True and out["steps"] == 3 and out["full"] is False
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - 65_536 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    for k in ("kernel_ms", "roofline", "ms_per_step_event_timed", "exploitability_exact", "groups", "cpu_baseline"):
        assert k not in out, k
    got = _load(d)
    assert set(got) == set(out["dumped_outputs"]) == _names()
    assert got["stats"][0] == (1 + 3) * 65_536          # the state after the last timed step

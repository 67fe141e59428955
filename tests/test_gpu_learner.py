"""Whole learner steps (nfsp_engine_update) against the numpy restatement of the learner
(oracle/learner_oracle.py).  Every update of the step is replayed:
* BR: row sampling, target-net forwards, TD targets, the row-0 quirk and the proxy; the Huber
  fits in their permutation order; the lr schedule; target syncs in mid-step;
* AR: the reservoir as of each trigger; the cross-entropy fits;
* the reservoir after the step.

The engine's memories after the rollout are the input.  The rollout itself is checked
against rollout_oracle in test_gpu_engine.py.

Tolerances:
* Sampling, schedules and the reservoir are compared exactly.
* Weights are compared after ~60 updates (~480 SGD steps) per net: max 1e-4, median 1e-7.
  Measured: max 2.4e-7, median 0. The chain sums exact products on bf16 matrix cores;
  numpy sums with BLAS. The max leaves room for a ReLU input near zero to change sign
  between the two.
"""
import numpy as np
import pytest

import learner_oracle as LO
from engine_ref import learner_state, obs_bits, oracle_cfg

CFG = dict(n_lanes=4096, rl_capacity=3000, sl_capacity=2000, target_every=30, seed=4242)
# edge cases: memories barely above the batch (the RL window is always capacity-bound, the
# reservoir replaces from the start), and the Kuhn swap-in
CASES = {
    "leduc": (CFG, "leduc"),
    "tiny_memories": (dict(n_lanes=1024, rl_capacity=200, sl_capacity=150, target_every=7, seed=99), "leduc"),
    "kuhn": (dict(n_lanes=4096, rl_capacity=3000, sl_capacity=2000, target_every=10, seed=7), "kuhn"),
    # the cfg's other fit shapes: minibatch sample of 64 rows, 3 epochs, an update every 96 inserts
    "batch64_e3": (dict(n_lanes=4096, rl_capacity=3000, sl_capacity=2000, target_every=20, seed=11,
                        batch=64, epochs=3, inserts_per_update=96), "leduc"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case,quirks", [("leduc", 7), ("leduc", 0), ("tiny_memories", 7), ("kuhn", 7),
                                         ("batch64_e3", 7),
                                         # textbook-NFSP extensions (NFSP_TEXTBOOK = 248; 120 =
                                         # without sampled AR actions, 112 = also without the
                                         # one-hot SL targets)
                                         ("leduc", 120), ("leduc", 112), ("tiny_memories", 120),
                                         ("kuhn", 120), ("kuhn", 248),
                                         # + NFSP_EXT_MSE_Q (504 = NFSP_TEXTBOOK_MSE)
                                         ("leduc", 504), ("kuhn", 504)])
def test_learner_step_matches_oracle(pkg, case, quirks):
    cfg_e, game = CASES[case]
    g = pkg.native.GAME_KUHN if game == "kuhn" else pkg.native.GAME_LEDUC
    eng = pkg.engine.SelfPlayEngine(init_seed=5, quirks=quirks, game=g, **cfg_e)
    for _ in range(2):
        eng.step()
    eng.rollout()
    st0, state = learner_state(eng)
    eng.update()
    st1 = eng.stats()
    c = eng.cfg
    cfg = oracle_cfg(c)
    want = LO.learner_step(cfg, state, quirks=quirks)
    for a in (0, 1):
        W = want[a]
        assert W["U_br"] > c.target_every and W["U"] >= W["U_br"]     # several target-sync segments
        assert st1["br_updates"][a] == W["br_updates"]
        assert st1["ar_updates"][a] - st0["ar_updates"][a] == W["ar_updates"]
        assert st1["iteration"][a] == W["iteration"]
        assert st1["epsilon"][a] == pytest.approx(W["epsilon"], rel=1e-12)
        assert st1["lr_br"][a] == pytest.approx(W["lr_br"], rel=1e-7)
        assert st1["temp"][a] == pytest.approx(W["temp"], rel=1e-12)
        assert st1["exploitability"][a] == pytest.approx(W["exploitability"], abs=1e-4)
        # Under the textbook extensions (quirks >= 8) the linear Q head moves more hidden units
        # across zero, where a ReLU's derivative follows the summation order (the cause
        # test_gpu_learner_divergence.py measures), and one-hot AR targets saturate the softmax
        # (its clip mask is the other discrete decision): a single flipped decision in ~480 SGD
        # steps leaves a net up to ~2e-4 away (measured 1.2e-4 .. 3.3e-4) while the median
        # stays at ~1e-7.  Bars: 1e-3 / 1e-6 there; 1e-4 / 1e-7 for the reference.
        tol_max, tol_med = (1e-3, 1e-6) if quirks >= 8 else (1e-4, 1e-7)
        for n in (0, 1, 2):
            d = np.abs(eng.get_weights(a, n) - W["w"][n])
            assert d.max() <= tol_max, (a, n, d.max())
            assert np.median(d) <= tol_med, (a, n, np.median(d))
        m = eng.memories(a)
        size = int(st1["sl_size"][a])
        assert np.array_equal(obs_bits(m["sl_s"].cpu().numpy()[:size]), W["res_x"][:size])
        assert np.array_equal(m["sl_a"].cpu().numpy()[:size], W["res_a"][:size])


@pytest.mark.gpu
def test_single_lane_engine_matches_oracle(pkg):
    """The reference's own configuration (C1: one env, one hand per step) through the engine:
    every learner call that triggers updates is replayed by the oracle, with memories small
    enough that M_RL wraps and the reservoir replaces within the run."""
    eng = pkg.engine.SelfPlayEngine(n_lanes=1, rl_capacity=300, sl_capacity=150, target_every=3,
                                    eta=0.5, seed=31337, init_seed=5)
    c = eng.cfg
    cfg = oracle_cfg(c)
    checked = ar_checked = 0
    for _ in range(4000):
        eng.rollout()
        st = eng.stats()
        due = any(st["rl_total"][a] // c.inserts_per_update > (st["rl_total"][a] - st["last_rl"][a]) // c.inserts_per_update
                  for a in (0, 1))
        if not due:
            eng.update()
            continue
        st0, state = learner_state(eng)
        eng.update()
        st1 = eng.stats()
        want = LO.learner_step(cfg, state, quirks=c.quirks)
        for a in (0, 1):
            W = want[a]
            assert st1["br_updates"][a] == W["br_updates"]
            assert st1["ar_updates"][a] - st0["ar_updates"][a] == W["ar_updates"]
            assert st1["iteration"][a] == W["iteration"]
            assert st1["epsilon"][a] == pytest.approx(W["epsilon"], rel=1e-12)
            ar_checked += W["ar_updates"]
            for n in (0, 1, 2):
                d = np.abs(eng.get_weights(a, n) - W["w"][n])
                assert d.max() <= 1e-4, (a, n, d.max())
            size = int(st1["sl_size"][a])
            m = eng.memories(a)
            assert np.array_equal(obs_bits(m["sl_s"].cpu().numpy()[:size]), W["res_x"][:size])
        checked += 1
        if (checked >= 12 and ar_checked >= 4 and min(st1["rl_total"]) > c.rl_capacity
                and max(st1["sl_total"]) > c.sl_capacity):
            break
    assert checked >= 12 and ar_checked >= 4
    assert min(st1["rl_total"]) > c.rl_capacity and max(st1["sl_total"]) > c.sl_capacity

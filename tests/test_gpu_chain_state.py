"""The SGD chain's row-owned W2 / b2 state (csrc/chain3_body.inc): each lane carries the two
values it owns in registers across the steps of a launch, and LDS holds the copy the other rows
and the epilogue read.  The cases below are the ones where that can go wrong, at the smallest
engine shapes that reach them:
* the generic-phase loop (SGD steps per update not a multiple of 4: the ring slot and the
  partial-sum buffer are run-time values, and the loop is not unrolled);
* many short launches (a target sync every 3 updates: the owned state goes through global
  memory at every launch boundary);
* a launch whose loop never runs (the AR chain while M_SL is not above the batch): the epilogue
  must write back what the prologue loaded;
* the loss-log instantiation (LOSS = 1, scalar forms) against the plain one: bit-identical;
* the table instantiation (TABLE = 1, engine groups) against standalone engines: bit-identical.

Parity with oracle/learner_oracle.py follows tests/test_gpu_learner.py: two steps, a rollout,
a snapshot of the memories, one learner call; bars 1e-4 max / 1e-7 median per net (quirks 7)."""
import numpy as np
import pytest
import torch

import learner_oracle as LO
from engine_ref import learner_state, nets, oracle_cfg

pytestmark = pytest.mark.gpu

TINY = dict(n_lanes=1024, rl_capacity=200, sl_capacity=150)
QUIRKS = 7


def _update_against_oracle(eng):
    """One learner call from the engine's present memories; returns the stats before it, the
    weights before it and the oracle's result, after checking counters and weights."""
    st0, state = learner_state(eng)
    eng.update()
    st1 = eng.stats()
    cfg = oracle_cfg(eng.cfg)
    want = LO.learner_step(cfg, state, quirks=QUIRKS)
    for a in (0, 1):
        W = want[a]
        assert st1["br_updates"][a] == W["br_updates"]
        assert st1["ar_updates"][a] - st0["ar_updates"][a] == W["ar_updates"]
        assert st1["iteration"][a] == W["iteration"]
        for n in (0, 1, 2):
            d = np.abs(eng.get_weights(a, n) - W["w"][n])
            print(f"agent {a} net {n}: max {d.max():.3g} median {np.median(d):.3g}")
            assert d.max() <= 1e-4, (a, n, d.max())
            assert np.median(d) <= 1e-7, (a, n, np.median(d))
    return st0, state, want


@pytest.mark.parametrize("batch,epochs,target_every", [
    (96, 1, 7),      # 3 SGD steps per update: the generic-phase loop
    (64, 3, 7),      # 6
    (128, 2, 3),     # 8, the unrolled loop; a BR launch every 3 updates
])
def test_chain_state_matches_oracle(pkg, batch, epochs, target_every):
    eng = pkg.engine.SelfPlayEngine(init_seed=5, quirks=QUIRKS, seed=99, batch=batch, epochs=epochs,
                                    target_every=target_every, **TINY)
    assert eng.cfg.epochs * (eng.cfg.batch // 32) == {96: 3, 64: 6, 128: 8}[batch]   # SGD steps per update
    for _ in range(2):
        eng.step()
    eng.rollout()
    _, _, want = _update_against_oracle(eng)
    for a in (0, 1):
        assert want[a]["U_br"] > target_every          # several launches of the BR chain
        assert want[a]["ar_updates"] > 0


@pytest.mark.parametrize("eta", [0.02, None])
def test_launch_with_an_inactive_prefix(pkg, eta):
    """A fresh engine's first learner call, right after its first rollout.  With eta 0.02 few
    actions come from the best response, M_SL is not above the batch at any trigger, and the AR
    launch is all inactive prefix: its loop never runs and the weights come back as they were,
    bit for bit.  With the default eta one agent's M_SL passes the batch in mid-call: its launch
    skips the inactive updates and runs the rest.  The BR chain runs as usual in both."""
    kw = {} if eta is None else dict(eta=eta)
    eng = pkg.engine.SelfPlayEngine(init_seed=5, quirks=QUIRKS, seed=99, target_every=3, **TINY, **kw)
    eng.rollout()
    ar0 = [eng.get_weights(a, 0) for a in (0, 1)]
    _, _, want = _update_against_oracle(eng)
    if eta is None:      # at least one agent's launch skips a prefix and runs the rest
        assert any(0 < want[a]["ar_updates"] < want[a]["U"] for a in (0, 1))
    for a in (0, 1):
        assert want[a]["U_br"] > 3 and want[a]["U"] > 0
        if eta is not None:
            assert want[a]["ar_updates"] == 0
        assert np.array_equal(eng.get_weights(a, 0), ar0[a]) == (want[a]["ar_updates"] == 0), a


def test_loss_log_changes_no_weight(pkg):
    """The loss-log build of the chain (scalar forms) leaves every net bit-identical to the
    plain build's."""
    out = []
    for log in (False, True):
        eng = pkg.engine.SelfPlayEngine(init_seed=5, quirks=QUIRKS, seed=99, target_every=3, **TINY)
        eng.set_loss_log(log)
        for _ in range(3):
            eng.step()
        st = eng.stats()
        assert min(st["br_updates"]) > 3 and min(st["ar_updates"]) > 0
        out.append(nets(eng))
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def test_table_launch_matches_standalone(pkg):
    """Engine groups launch the chain's table instantiation: 2 replicas against 2 standalone
    engines after one learner call, with a BR launch every 3 updates."""
    kw = dict(quirks=QUIRKS, target_every=3, **TINY)
    g = pkg.engine.EngineGroup(2, seed=99, init_seed=5, **kw)
    solo = [pkg.engine.SelfPlayEngine(seed=99 + r, init_seed=5 + r, **kw) for r in range(2)]
    w0 = nets(solo[0])
    g.step()
    for e in solo:
        e.step()
    torch.cuda.synchronize()
    for r in range(2):
        assert min(solo[r].stats()["br_updates"]) > 3
        for x, y in zip(nets(g.replicas[r]), nets(solo[r])):
            assert np.array_equal(x, y), r
    assert not np.array_equal(nets(solo[0])[1], w0[1])     # the BR net moved

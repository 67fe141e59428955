"""The SGD chain's b2 update is carried across the step boundary (csrc/chain3_body.inc): step t
leaves its loss gradients and lr pending in registers, step t + 1 totals them and updates the b2
copy that every lane holds in registers, and the epilogue applies the last one.  The cases below
are the ones where a deferred update can go wrong, at tests/test_gpu_chain_state.py's TINY engine:
* the fewest SGD steps per update the cfg rules allow (batch 32: 1, 2 and 3 steps): the generic
  loop, where the pending update crosses every update boundary;
* target_every 1, 2, 3: a BR launch boundary every few steps, the epilogue's pending update
  applied and the weights through global memory each time;
* the all-inactive AR launch (its loop never runs): the net comes back bit for bit;
* the loss-log instantiation (LOSS = 1) against the plain one: bit-identical;
* a group of 2 (TABLE = 1) against standalone engines: bit-identical.

Every case is checked against oracle/learner_oracle.py at the bars of tests/test_gpu_learner.py
(1e-4 max / 1e-7 median per net, quirks 7), and its engine digest against
tests/golden/chain_parent_digests.json: the digests of the same runs on the parent commit's
library (b2 row-owned in LDS, updated inside the step), recorded by

    NFSP_LIB=<the parent's libnfsp.so> python tests/test_gpu_chain_b2.py <out.json>

so the deferred update changes no bit of the training state."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TINY = dict(n_lanes=1024, rl_capacity=200, sl_capacity=150)
QUIRKS = 7
GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_parent_digests.json")


def _hex(d):
    return [f"{int(x):016x}" for x in d]


def _update_against_oracle(eng):
    """One learner call from the engine's present memories, checked against the oracle's."""
    import learner_oracle as LO
    from engine_ref import learner_state, oracle_cfg
    st0, state = learner_state(eng)
    eng.update()
    st1 = eng.stats()
    want = LO.learner_step(oracle_cfg(eng.cfg), state, quirks=QUIRKS)
    for a in (0, 1):
        W = want[a]
        assert st1["br_updates"][a] == W["br_updates"]
        assert st1["ar_updates"][a] - st0["ar_updates"][a] == W["ar_updates"]
        for n in (0, 1, 2):
            d = np.abs(eng.get_weights(a, n) - W["w"][n])
            print(f"agent {a} net {n}: max {d.max():.3g} median {np.median(d):.3g}")
            assert d.max() <= 1e-4, (a, n, d.max())
            assert np.median(d) <= 1e-7, (a, n, np.median(d))
    return want


def _engine(pkg, **kw):
    return pkg.engine.SelfPlayEngine(init_seed=5, quirks=QUIRKS, seed=99, **TINY, **kw)


def run_steps(pkg, batch, epochs, target_every):
    """Two steps, a rollout and one learner call against the oracle; the digest after it."""
    eng = _engine(pkg, batch=batch, epochs=epochs, target_every=target_every)
    assert eng.cfg.epochs * (eng.cfg.batch // 32) == epochs * (batch // 32)
    for _ in range(2):
        eng.step()
    eng.rollout()
    want = _update_against_oracle(eng)
    for a in (0, 1):
        assert want[a]["U_br"] > target_every          # several launches of the BR chain
        assert want[a]["ar_updates"] > 0
    return [_hex(eng.state_digest())]


def run_inactive(pkg):
    """A fresh engine's first learner call with eta 0.02: M_SL is not above the batch at any
    trigger, the AR launch is all inactive prefix and its loop never runs."""
    eng = _engine(pkg, target_every=3, eta=0.02)
    eng.rollout()
    ar0 = [eng.get_weights(a, 0) for a in (0, 1)]
    want = _update_against_oracle(eng)
    for a in (0, 1):
        assert want[a]["U_br"] > 3 and want[a]["U"] > 0 and want[a]["ar_updates"] == 0
        assert np.array_equal(eng.get_weights(a, 0), ar0[a]), a      # b2 included, bit for bit
    return [_hex(eng.state_digest())]


def run_loss_log(pkg):
    from engine_ref import nets
    out, dig = [], []
    for log in (False, True):
        eng = _engine(pkg, target_every=3)
        eng.set_loss_log(log)
        for _ in range(2):
            eng.step()
        eng.rollout()
        _update_against_oracle(eng)
        st = eng.stats()
        assert min(st["br_updates"]) > 3 and min(st["ar_updates"]) > 0
        out.append(nets(eng))
        dig.append(_hex(eng.state_digest()))
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    return dig


def run_group(pkg):
    import torch
    from engine_ref import nets
    kw = dict(quirks=QUIRKS, target_every=3, **TINY)
    g = pkg.engine.EngineGroup(2, seed=99, init_seed=5, **kw)
    solo = [pkg.engine.SelfPlayEngine(seed=99 + r, init_seed=5 + r, **kw) for r in range(2)]
    w0 = nets(solo[0])
    g.step()
    for e in solo:           # one step of a one-slice engine, its learner call against the oracle
        e.rollout()
        _update_against_oracle(e)
    torch.cuda.synchronize()
    for r in range(2):
        assert min(solo[r].stats()["br_updates"]) > 3
        for x, y in zip(nets(g.replicas[r]), nets(solo[r])):
            assert np.array_equal(x, y), r
    assert not np.array_equal(nets(solo[0])[1], w0[1])     # the BR net moved
    return [_hex(d) for d in g.state_digest()] + [_hex(e.state_digest()) for e in solo]


CASES = {
    "steps1_b32_e1_te7": lambda pkg: run_steps(pkg, 32, 1, 7),
    "steps2_b32_e2_te7": lambda pkg: run_steps(pkg, 32, 2, 7),
    "steps3_b32_e3_te7": lambda pkg: run_steps(pkg, 32, 3, 7),
    "steps8_b128_e2_te1": lambda pkg: run_steps(pkg, 128, 2, 1),
    "steps8_b128_e2_te2": lambda pkg: run_steps(pkg, 128, 2, 2),
    "steps8_b128_e2_te3": lambda pkg: run_steps(pkg, 128, 2, 3),
    "inactive_ar": run_inactive,
    "loss_log": run_loss_log,
    "group2": run_group,
}


@pytest.fixture(scope="module")
def parent_digests():
    with open(GOLDEN_JSON) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_deferred_b2_matches_oracle_and_parent(pkg, parent_digests, case):
    got = CASES[case](pkg)
    print(case, got)
    assert got == parent_digests[case], case


if __name__ == "__main__":      # record the digests of the library NFSP_LIB names (see above)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import conftest  # noqa: F401  (puts the repository and the oracle on sys.path)
    import __graft_entry__
    package = __graft_entry__.load_package()
    with open(sys.argv[1], "w") as f:
        json.dump({k: CASES[k](package) for k in sorted(CASES)}, f, indent=1, sort_keys=True)
        f.write("\n")

"""The learner and the rollout away from the reference's hyperparameters, against the oracles.

Every other oracle test holds lr_br = 0.05, lr_ar = 0.1, gamma = 0.95, epsilon = 0.06 and
eta = 0.3; test_gpu_group_hetero.py varies them but compares the project with itself.  Here
the same two procedures run at the values a sweep visits:

A. test_learner_step_matches_oracle's procedure (two steps, a rollout, then nfsp_engine_update
   replayed update by update by oracle/learner_oracle.py) on the `tiny_memories` shape, once
   per field and once with all of them changed.
   * Bars: test_gpu_learner.py's own, max 1e-4 / median 1e-7 (1e-3 / 1e-6 for quirks >= 8),
     for every rate at or below its default: an SGD step is linear in its rate, so a lower
     rate cannot widen the ReLU-crossing gap those bars leave room for.  `rates_x2` doubles
     both rates and gets twice the bars, the ratio of the rates.
   * Sensitivity (a condition on the inputs, decided on the CPU): for a case that changes one
     field, the oracle replays the same snapshot with that field at its default.  The net the
     field acts on (BR for lr_br and gamma, AR for lr_ar) must then land more than 100 x the
     case's max bar away, so a kernel that ignored the field could not pass.  Under the
     reference's row-0 quirk no seed gives that at 1e-4: one row in 128 carries TD values, the
     BR net moves by 1e-3 to 5e-3 in the whole call, and over six seeds the replay at the
     default lies 2e-5 to 1.3e-4 (gamma = 1), 1.7e-4 to 1.3e-3 (gamma = 0.5), 3e-4 to 2.8e-3
     (gamma = 0) and 7e-4 to 3.2e-3 (lr_br = 0.01) away.  With a bar of 1e-4 a kernel that ignored
     gamma = 1 would pass.  So the bar gives way, not the condition: on the affected net the
     case's max bar is min(1e-4, distance / 128), and the inputs are refused if that falls below
     MIN_BAR.  Without the quirk (gamma_zero_q0) and for lr_ar the distance is ~1e-1 and the
     bar stays 1e-4.
   * lr_br = 0 and lr_ar = 0 need no oracle: the nets stay bit-identical to their initial values
     while the counters advance.  Those runs act at eta = 1 with a constant epsilon of 1 (every
     action is a Philox draw), so that the hands, and with them every counter and the nets of
     the other kind, are the same as in the run at the default rates they are compared with.
B. test_rollout_matches_oracle's procedure (oracle/rollout_oracle.py) at eta = 0 and 1, at
   epsilon = 0 and 1, and with an epsilon that differs between the agents, on 777 lanes (a
   multiple of neither the wave nor the workgroup).  Bars: test_gpu_engine.py's, everything
   exact but the action vectors (1e-6).

Measured (MI355X): the largest max and median |engine - oracle| over both agents' three nets;
for the single-field cases the distance between the two oracle replays on the affected net
(agent 0, agent 1) and the max bar that net gets.  Updates per agent: 13-21 (cadence: 28-32
triggers, 20-24 of them with a BR update, 9-18 with an AR update).

    case            max      median   distance            bar on that net
    lr_br_low       7.5e-8   0        1.2e-3, 1.0e-3      8.1e-6
    lr_ar_low       4.5e-8   0        8.8e-2, 7.9e-2      1e-4
    gamma_half      6.0e-8   0        6.0e-4, 4.2e-4      3.3e-6
    gamma_one       8.9e-8   0        8.0e-5, 4.8e-5      3.7e-7  (BR net: 4.5e-8)
    gamma_zero      8.9e-8   0        1.4e-3, 9.0e-4      7.0e-6
    gamma_zero_q0   8.9e-8   0        1.1e-1, 1.8e-1      1e-4
    epsilon         8.9e-8   0
    epsilon_const   2.1e-7   0
    sweep_point     6.0e-8   0
    cadence         6.0e-8   0
    rates_x2        1.0e-7   0        (bars 2e-4 / 2e-7)

The whole file takes 14 s, test_gpu_learner.py (the same procedure 12 times at 4 x the lanes) 10 s.
"""
import numpy as np
import pytest

import learner_oracle as LO
import rollout_oracle as R
from engine_ref import check_rollout, learner_state, obs_bits, oracle_cfg, weights_flat

pytestmark = pytest.mark.gpu

SHAPE = dict(n_lanes=1024, rl_capacity=200, sl_capacity=150, target_every=7, seed=99)
NET = {"lr_br": 1, "lr_ar": 0, "gamma": 1}          # the net a field acts on (0 AR, 1 BR)
# The narrowest max bar a case may end up with.  The weights are f32 below 0.5 (ulp 3e-8), and
# the two sides round each of the call's ~150 SGD steps differently: a random walk of half-ulp
# steps ends ~6 ulp away.
MIN_BAR = 2e-7

# name: (cfg fields, quirks, bar factor)
LEARNER_CASES = {
    "lr_br_low": (dict(lr_br=0.01), 7, 1),
    "lr_ar_low": (dict(lr_ar=0.02), 7, 1),
    "gamma_half": (dict(gamma=0.5), 7, 1),
    "gamma_one": (dict(gamma=1.0), 7, 1),
    "gamma_zero": (dict(gamma=0.0), 7, 1),            # targets are the rewards alone
    "gamma_zero_q0": (dict(gamma=0.0), 0, 1),         # ... where terminal rows skip the bootstrap
    "epsilon": (dict(epsilon=0.2), 7, 1),
    "epsilon_const": (dict(epsilon=0.2), 120, 1),
    "sweep_point": (dict(lr_br=0.01, lr_ar=0.02, gamma=0.8, epsilon=0.2), 504, 1),
    # a fresh engine's first learner call: triggers 1..8 have an AR slot but no BR update
    # (m c <= batch), and every BR update is its own target-sync segment.  eta = 0.5 fills M_SL
    # past the batch in mid-call, so the AR chain has skipped slots, then active ones
    "cadence": (dict(inserts_per_update=16, target_every=1, n_lanes=256, eta=0.5), 7, 1),
    "rates_x2": (dict(lr_br=0.1, lr_ar=0.2), 7, 2),
}


def _diffs(eng, W, a):
    d = [np.abs(eng.get_weights(a, n) - W["w"][n]) for n in (0, 1, 2)]
    return [(float(x.max()), float(np.median(x))) for x in d]


@pytest.mark.parametrize("case", list(LEARNER_CASES))
def test_learner_step_off_default(pkg, case):
    fields, quirks, factor = LEARNER_CASES[case]
    eng = pkg.engine.SelfPlayEngine(init_seed=5, quirks=quirks, **dict(SHAPE, **fields))
    c = eng.cfg
    for k, v in fields.items():          # the engine runs the value asked for (f32 for the rates)
        assert getattr(c, k) == (np.float32(v) if k.startswith("lr_") else v), k
    if case != "cadence":
        for _ in range(2):
            eng.step()
    eng.rollout()
    st0, state = learner_state(eng)
    eng.update()
    st1 = eng.stats()
    cfg = oracle_cfg(c)
    want = LO.learner_step(cfg, state, quirks=quirks)
    tol_max, tol_med = (1e-3, 1e-6) if quirks >= 8 else (1e-4, 1e-7)
    tol_max, tol_med = tol_max * factor, tol_med * factor
    tol_net = {n: tol_max for n in (0, 1, 2)}
    if len(fields) == 1 and next(iter(fields)) in NET:
        # sensitivity: the same snapshot at the field's default must land more than 100 bars away
        k = next(iter(fields))
        dflt = pkg.engine.make_cfg(eng.L)
        other = LO.learner_step(dict(cfg, **{k: getattr(dflt, k)}), state, quirks=quirks)
        dist = [float(np.abs(other[a]["w"][NET[k]] - want[a]["w"][NET[k]]).max()) for a in (0, 1)]
        tol_net[NET[k]] = min(tol_max, min(dist) / 128)
        print(f"{case}: oracle at the default {k} is {dist[0]:.1e}, {dist[1]:.1e} away on net {NET[k]}, "
              f"whose max bar is {tol_net[NET[k]]:.1e}")
        assert min(dist) > 100 * tol_net[NET[k]]
        assert tol_net[NET[k]] >= MIN_BAR, "these inputs cannot show the field: pick another seed"
    for a in (0, 1):
        W = want[a]
        if case == "cadence":
            assert st0["br_updates"][a] == 0 and st0["iteration"][a] == 0
            assert W["U"] > W["U_br"] > 8
            assert 0 < W["ar_updates"] < W["U"]
            assert st1["target_syncs"][a] == W["U_br"]
            assert np.array_equal(eng.get_weights(a, 1), eng.get_weights(a, 2))
        else:
            assert W["U_br"] > c.target_every and W["U"] >= W["U_br"]     # several target-sync segments
        assert st1["br_updates"][a] == W["br_updates"]
        assert st1["ar_updates"][a] - st0["ar_updates"][a] == W["ar_updates"]
        assert st1["iteration"][a] == W["iteration"]
        assert st1["epsilon"][a] == pytest.approx(W["epsilon"], rel=1e-12)
        assert st1["lr_br"][a] == pytest.approx(W["lr_br"], rel=1e-7)
        assert st1["temp"][a] == pytest.approx(W["temp"], rel=1e-12)
        assert st1["exploitability"][a] == pytest.approx(W["exploitability"], abs=1e-4)
        if "epsilon" in fields:
            if quirks & LO.EXT_EPS_CONST:           # the extension: epsilon stays the cfg's
                assert st0["epsilon"][a] == st1["epsilon"][a] == 0.2
            else:                                   # the schedule divides the cfg's value
                eps = 0.2
                for k in range(1, st1["br_updates"][a] + 1):
                    if k == st0["br_updates"][a] + 1:
                        assert st0["epsilon"][a] == pytest.approx(eps, rel=1e-12)
                    eps /= 2 * k
                assert 0.0 < eps and st1["epsilon"][a] == pytest.approx(eps, rel=1e-12)
        d = _diffs(eng, W, a)
        print(f"{case} agent {a}: U={W['U']} U_br={W['U_br']} AR={W['ar_updates']} (max, median) per net",
              " ".join(f"{mx:.1e}/{md:.1e}" for mx, md in d))
        for n, (mx, md) in enumerate(d):
            assert mx <= tol_net[n], (a, n, mx)
            assert md <= tol_med, (a, n, md)
        m = eng.memories(a)
        size = int(st1["sl_size"][a])
        assert np.array_equal(obs_bits(m["sl_s"].cpu().numpy()[:size]), W["res_x"][:size])
        assert np.array_equal(m["sl_a"].cpu().numpy()[:size], W["res_a"][:size])


RANDOM_ACTING = dict(n_lanes=1024, rl_capacity=200, sl_capacity=150, target_every=7, seed=99,
                     eta=1.0, epsilon=1.0, quirks=7 | 64)       # 64 = NFSP_EXT_EPS_CONST
COUNTERS = ("rl_total", "sl_total", "br_updates", "ar_updates", "iteration", "target_syncs")


def _three_steps(pkg, **fields):
    eng = pkg.engine.SelfPlayEngine(init_seed=5, **dict(RANDOM_ACTING, **fields))
    w0 = [[eng.get_weights(a, n) for n in (0, 1, 2)] for a in (0, 1)]
    for _ in range(3):
        eng.step()
    st = eng.stats()
    w = [[eng.get_weights(a, n) for n in (0, 1, 2)] for a in (0, 1)]
    return w0, w, {k: st[k] for k in COUNTERS}


@pytest.fixture(scope="module")
def default_rates_run(pkg):
    return _three_steps(pkg)


def _same(x, y):
    return np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("field,frozen,free", [("lr_br", (1, 2), (0,)), ("lr_ar", (0,), (1, 2))])
def test_zero_rate_freezes_its_nets_and_nothing_else(pkg, default_rates_run, field, frozen, free):
    """A rate of zero: the nets it trains keep their initial bits through three steps, the
    counters advance as at the default rates, and the other nets are the default run's."""
    w0_d, w_d, st_d = default_rates_run
    w0, w, st = _three_steps(pkg, **{field: 0.0})
    assert st == st_d
    assert min(st["br_updates"]) > 3 * 7 and min(st["ar_updates"]) > 3 and min(st["target_syncs"]) > 3
    for a in (0, 1):
        assert st["iteration"][a] == 2 * st["br_updates"][a]
        for n in frozen:
            assert _same(w[a][n], w0[a][n]), (a, n)
            assert not _same(w_d[a][n], w0_d[a][n]), (a, n)      # the default run does train them
        for n in free:
            assert _same(w[a][n], w_d[a][n]), (a, n)
            assert not _same(w[a][n], w0[a][n]), (a, n)


# ---------------------------------------------------------------------------------------------
# B. rollouts
# ---------------------------------------------------------------------------------------------
N, SEED = 777, 1234


def _rollout_engine(pkg, **kw):
    return pkg.engine.SelfPlayEngine(n_lanes=N, seed=SEED, quirks=7, init_seed=11, inserts_per_update=1 << 30, **kw)


def _ref(g, w, eps, eta, rl_before=(0, 0)):
    # the device compares an f32 eta with an f32 u01: the oracle gets the f32 value
    return R.rollout_with_positions(N, g, SEED, w, eps, eta=float(np.float32(eta)), alias=True,
                                    rl_before=rl_before, ext=7)


def _rl_actions(eng, p, n):
    return eng.memories(p)["rl_a"].cpu().numpy()[:n]


def test_rollout_eta_zero(pkg):
    """eta = 0: no agent ever plays its best response, so no SL record is made and every stored
    action vector is an AR net's softmax."""
    eng = _rollout_engine(pkg, eta=0.0)
    w = weights_flat(eng)
    eng.rollout()
    ref = _ref(0, w, (0.06, 0.06), 0.0)
    assert [len(ref["sl"][p]) for p in (0, 1)] == [0, 0]
    check_rollout(eng, ref)
    st = eng.stats()
    assert st["last_sl"] == [0, 0] and st["hands"] == N
    assert np.array_equal(np.array(st["actions"]), ref["actions"])
    for p in (0, 1):
        a = _rl_actions(eng, p, st["last_rl"][p])
        assert len(a) > N // 2 and np.abs(a.sum(axis=1) - 1.0).max() <= 1e-6     # softmax rows
    eng.update()
    st = eng.stats()
    assert st["ar_updates"] == [0, 0] and st["sl_total"] == [0, 0]
    before = tuple(st["rl_total"])
    eng.rollout()
    ref2 = _ref(1, w, (0.06, 0.06), 0.0, rl_before=before)
    check_rollout(eng, ref2, rl_before=before)
    assert eng.stats()["last_sl"] == [0, 0]
    # with the learner at its usual cadence the BR nets train and the AR nets have nothing to fit
    eng = pkg.engine.SelfPlayEngine(n_lanes=N, seed=SEED, init_seed=11, eta=0.0, rl_capacity=1000, sl_capacity=1000)
    ar0 = [eng.get_weights(a, 0) for a in (0, 1)]
    eng.step()
    st = eng.stats()
    assert st["ar_updates"] == [0, 0] and st["sl_total"] == [0, 0] and min(st["br_updates"]) > 0
    assert all(np.array_equal(eng.get_weights(a, 0), ar0[a]) for a in (0, 1))


def test_rollout_eta_one_epsilon_one(pkg):
    """eta = 1, epsilon = 1: every decision is a best-response one and every action the random
    draw.  No net is consulted: the oracle replays the rollout with all-zero nets."""
    eng = _rollout_engine(pkg, eta=1.0, epsilon=1.0)
    assert eng.stats()["epsilon"] == [1.0, 1.0]
    blank = np.zeros_like(weights_flat(eng))
    eng.rollout()
    ref = _ref(0, blank, (1.0, 1.0), 1.0)
    check_rollout(eng, ref)
    st = eng.stats()
    assert np.array_equal(np.array(st["actions"]), ref["actions"])
    assert st["last_sl"] == [int(sum(st["actions"][p])) for p in (0, 1)]      # an SL record per decision
    eng.update()
    before = tuple(eng.stats()["rl_total"])
    eng.rollout()
    ref2 = _ref(1, blank, (1.0, 1.0), 1.0, rl_before=before)
    check_rollout(eng, ref2, rl_before=before)
    assert np.array_equal(np.array(eng.stats()["actions"]), ref["actions"] + ref2["actions"])


def test_rollout_eta_one_epsilon_zero(pkg):
    """eta = 1, epsilon = 0: every action is the BR net's output on the observation it stored."""
    eng = _rollout_engine(pkg, eta=1.0)
    w = weights_flat(eng)
    eng.rollout_with(w, (0.0, 0.0))
    ref = _ref(0, w, (0.0, 0.0), 1.0)
    check_rollout(eng, ref)
    st = eng.stats()
    assert np.array_equal(np.array(st["actions"]), ref["actions"])
    nets = R.Nets(w)
    for p in (0, 1):
        k = st["last_sl"][p]
        assert k == int(sum(st["actions"][p])) and k > N // 2
        m = eng.memories(p)
        x = LO.bits_to_x(m["pend_x"][:k].cpu().numpy().astype(np.int64) & 0xFFFFFFFF)
        assert np.abs(m["pend_a"][:k].cpu().numpy() - nets.br[p].predict(x)).max() <= 1e-6


def test_rollout_epsilons_differ_between_agents(pkg):
    """What every run has after its first BR update: the two agents act with different epsilons.
    Agent 0 explores on half of its best-response decisions, agent 1 on none."""
    eng = _rollout_engine(pkg, eta=0.3)
    w = weights_flat(eng)
    eng.rollout_with(w, (0.5, 0.0))
    ref = _ref(0, w, (0.5, 0.0), 0.3)
    check_rollout(eng, ref)
    st = eng.stats()
    assert np.array_equal(np.array(st["actions"]), ref["actions"])
    # the inputs tell the agents apart: swapped epsilons give other records for both
    swapped = _ref(0, w, (0.0, 0.5), 0.3)
    for p in (0, 1):
        assert st["last_sl"][p] > 50
        assert any(not np.array_equal(x[1], y[1]) for x, y in zip(ref["sl"][p], swapped["sl"][p]))

"""The exact rollout model (tests/rollout_dist_ref.py) without a GPU: against the brute-force
oracle (oracle/exploit_oracle.py plays whole histories through the reference-restated Env and
knows nothing of the tree), against closed forms, and against the counts of
``rollout_oracle.rollout_lanes`` at 3,000 lanes -- with wrong models that must break the bound.
The GPU side is tests/test_gpu_rollout_dist.py.

Measured on the oracle's counts (cells with expectation >= 30; z* = 6.36 for the K = 4,836
statistics of the three comparisons and the alias run):
    leduc, quirks 3,   eta 0.3, eps (0.06, 0.06)   62 cells  max |z| 2.57  rms z 1.08
    leduc, quirks 248, eta 0.3, eps (0.3, 0.06)    76 cells  max |z| 2.24  rms z 0.95
    kuhn,  quirks 248, eta 0.2, eps (0.1, 0.1)     73 cells  max |z| 2.38  rms z 0.97
Without rule 4 the first cell alone is off by z = -12.4 (3 records where 144 are expected).
"""
import ctypes as C
import math

import numpy as np
import pytest

import exploit_oracle as eo
import policy_ref as pr
import rollout_dist_ref as rd
import rollout_oracle as R

GAMES = {"leduc": 0, "kuhn": 1}
N_LANES, SEED = 3000, 1234
# (game, quirks, eta, eps, init_seed)
ORACLE_CASES = {
    "leduc3": ("leduc", 3, 0.3, (0.06, 0.06), 11),
    "leduc248": ("leduc", 248, 0.3, (0.3, 0.06), 11),
    "kuhn248": ("kuhn", 248, 0.2, (0.1, 0.1), 11),
}
PARAM_SETS = [(3, 0.3, (0.06, 0.06), 11), (248, 0.3, (0.3, 0.06), 11), (7, 0.1, (0.06, 0.06), 5)]
CUT = 30.0
_TREES = {}
_RUNS = {}


@pytest.fixture(scope="module")
def trees(pkg):
    import __graft_entry__
    __graft_entry__.build()
    for name, g in GAMES.items():
        if name not in _TREES:
            _TREES[name] = pkg.evaluation.GameTree(g)
    return _TREES


def init_weights(pkg, init_seed):
    """The packed [2][3][NP] nets an engine starts from (engine.SelfPlayEngine._init_weights)."""
    rng = np.random.RandomState(init_seed)
    out = []
    for _ in (0, 1):
        ar = pkg.engine.glorot_net(rng)
        br = pkg.engine.glorot_net(rng)
        pkg.engine.glorot_net(rng)
        out += [ar, br, br]
    return np.concatenate(out)


def z_file(trees):
    """z* of this file: the statistics of the three oracle comparisons and of the alias run."""
    k = sum(rd.stats_per_rollout(trees[ORACLE_CASES[c][0]].ndec) for c in ORACLE_CASES)
    k += rd.stats_per_rollout(trees["leduc"].ndec)
    return rd.z_star(k)


def oracle_counts(tree, out, alias):
    """``check_counts``'s observation of a ``rollout_lanes`` result."""
    rl = np.zeros((tree.ndec, 3, 3), np.int64)
    sl = np.zeros((tree.ndec, 3), np.int64)
    n_rl, n_sl = [0, 0], [0, 0]
    for lane in out["lanes"]:
        for p in (0, 1):
            for (s, a, _r, _s2, _t) in lane["rl"][p]:
                if not alias:
                    row, rank = tree.row_of(p, s)
                    rl[row, rank, int(np.argmax(a))] += 1
                n_rl[p] += 1
            for (x, _y, _pos) in lane["sl"][p]:
                row, rank = tree.row_of(p, x)
                sl[row, rank] += 1
                n_sl[p] += 1
    return dict(rl=None if alias else rl, sl=sl, actions=out["actions"], reward0=out["reward"][0], n_rl=n_rl, n_sl=n_sl)


def oracle_run(pkg, trees, case):
    """(model, observation) of one oracle rollout; computed once and shared (teeth included)."""
    if case not in _RUNS:
        game, quirks, eta, eps, init_seed = ORACLE_CASES[case]
        w = init_weights(pkg, init_seed)
        out = R.rollout_lanes(N_LANES, 0, SEED, w, eps, eta=eta, alias=bool(quirks & 4), game=game, ext=quirks)
        _RUNS[case] = (w, oracle_counts(trees[game], out, bool(quirks & 4)))
    return _RUNS[case]


def model_of(trees, case, w, **wrong):
    game, quirks, eta, eps, _ = ORACLE_CASES[case]
    return rd.Model(trees[game], w, eta, eps, quirks, **wrong)


# ---- the model against the brute force ----------------------------------------------------------
@pytest.mark.parametrize("game", ["leduc", "kuhn"])
@pytest.mark.parametrize("params", PARAM_SETS)
def test_model_reward_matches_brute_force(pkg, trees, game, params):
    quirks, eta, eps, init_seed = params
    tree = trees[game]
    m = rd.Model(tree, init_weights(pkg, init_seed), eta, eps, quirks)
    # rule 1: the remapped acting table is evaluation.mix of the two tables
    mix = pkg.evaluation.mix(tree, [(m.p_br, m.t_br), (1.0 - m.p_br, m.t_ar)])
    reached = (m.visit.sum(axis=0) > 0)
    assert np.abs(m.acting - mix)[reached].max() <= 1e-12
    p0, p1 = pr.oracle_policy(tree, m.acting, 0), pr.oracle_policy(tree, m.acting, 1)
    for d in (0, 1):
        want = eo.on_policy_value0(p0, p1, game, dealers=(d,))
        assert abs(m.reward_mean[d] - want) <= 1e-9, (d, m.reward_mean[d], want)


# ---- closed forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", ["leduc", "kuhn"])
@pytest.mark.parametrize("params", PARAM_SETS)
def test_model_closed_forms(pkg, trees, game, params):
    quirks, eta, eps, init_seed = params
    tree = trees[game]
    m = rd.Model(tree, init_weights(pkg, init_seed), eta, eps, quirks)
    for d in (0, 1):
        assert np.abs(m.p_dec[d].sum(axis=2) - m.visit[d]).max() <= 1e-15
        first = int(tree.nodes["row"][tree.root[d]])
        assert tree.seat[first] == d                     # the dealer acts first
        assert np.abs(m.visit[d][first] - 1.0 / 3.0).max() <= 1e-15
        assert np.all(m.p_rec[d] >= 0.0) and np.all(m.p_rec[d] <= m.p_dec[d])
        assert np.all(m.p_sl[d] <= m.visit[d] + 1e-18)
        # rows of the other dealer's tree are never visited
        assert m.visit[d][m.dealer_of_row != d].max() == 0.0
        # the mode walk's means are the behavioural tables' (Kuhn's theorem: rule 1)
        for p in (0, 1):
            own = tree.seat == p
            assert np.abs(m.cnt_mean[d][5 * p:5 * p + 3] - m.p_dec[d][own].sum(axis=(0, 1))).max() <= 1e-12
            assert abs(m.cnt_mean[d][5 * p + 3] - m.p_rec[d][own].sum()) <= 1e-12
            assert abs(m.cnt_mean[d][5 * p + 4] - m.p_sl[d][own].sum()) <= 1e-12
        assert np.all(m.cnt_var[d] >= -1e-15)


def test_draw_probabilities():
    """Rule 6: 24-bit draws, inclusive comparisons."""
    assert rd.p_not_above(0.0) == 2.0 ** -24 and rd.p_not_above(1.0) == 1.0 and rd.p_not_above(-1.0) == 0.0
    assert rd.p_not_above(0.5) == 0.5 + 2.0 ** -24
    assert abs(rd.p_not_above(0.06) - 0.06) <= 2.0 ** -24
    zs = rd.z_star(5000)                    # 6.36
    assert 5000 * math.erfc(zs / math.sqrt(2.0)) <= 1e-6 < 5000 * math.erfc((zs - 1e-6) / math.sqrt(2.0))
    assert [int(v) for v in rd.dealer_lanes(87381, 87381, 0)] == [43690, 43691]
    assert [int(v) for v in rd.dealer_lanes(87381, 87381, 1)] == [43691, 43690]


@pytest.mark.parametrize("game", ["leduc", "kuhn"])
def test_model_uniform_play_is_uniform(pkg, trees, game):
    tree = trees[game]
    m = rd.Model(tree, init_weights(pkg, 11), 1.0, (1.0, 1.0), 3)
    assert m.p_br == 1.0 and np.all(m.p_rand == 1.0)
    for d in (0, 1):
        assert np.abs(m.p_dec[d] - m.visit[d][:, :, None] / 3.0).max() <= 1e-16
        assert np.array_equal(m.p_rec[d], m.p_dec[d])    # a random action is never all zero
        assert np.array_equal(m.p_sl[d], m.visit[d])


def test_model_leduc_joint_deal(pkg, trees):
    """P(r0, r1, public) read off the first decisions of round 2 is count / 120 of the 6-card
    deck.  Under uniform play every deal reaches round 2 with the same probability, so the
    reach there, normalised, is the deal itself."""
    tree = trees["leduc"]
    m = rd.Model(tree, init_weights(pkg, 11), 1.0, (1.0, 1.0), 3)
    deals = eo.rank_deals("leduc")
    N = tree.nodes
    for d in (0, 1):
        joint = np.zeros((3, 3, 3))
        for n in range(tree.nn):
            par = int(N["parent"][n])
            if par >= 0 and N["kind"][par] == pr.CHANCE and m.dealer_of_row[N["row"][n]] == d:
                assert N["kind"][n] == pr.DECISION and tree.seat[N["row"][n]] == d    # the dealer opens round 2
                joint[:, :, int(N["via"][n])] += m.reach[d][n]
        tot = joint.sum()
        assert 0.0 < tot < 1.0
        want = np.zeros((3, 3, 3))
        for k, pv in deals.items():
            want[k] = pv
        assert np.abs(joint / tot - want).max() <= 1e-15
        assert joint[want == 0.0].max() == 0.0           # three cards of one rank


# ---- the model against the oracle's rollout -----------------------------------------------------------
@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_model_matches_oracle_rollout(pkg, trees, case):
    w, obs = oracle_run(pkg, trees, case)
    zs = z_file(trees)
    out = rd.check_counts(model_of(trees, case, w), obs, 0, N_LANES, 0, zs, cut=CUT)
    print(f"{case}: z* {zs:.2f}; {rd.summary(out)}")
    assert not out["failures"], out["failures"]
    if len(out["z_cells"]) >= 200:
        assert 0.7 <= rd.rms(out) <= 1.3


def test_oracle_rollout_under_the_alias_quirk(pkg, trees):
    """Quirks 7: the aggregate statistics and the SL records (rule 5), same lanes as leduc3 --
    the alias changes which (s, a) a row carries, not the hands."""
    w = init_weights(pkg, 11)
    out = R.rollout_lanes(600, 0, SEED, w, (0.06, 0.06), eta=0.3, alias=True, game="leduc", ext=7)
    obs = oracle_counts(trees["leduc"], out, True)
    res = rd.check_counts(rd.Model(trees["leduc"], w, 0.3, (0.06, 0.06), 7), obs, 0, 600, 0, z_file(trees), cut=CUT)
    print(rd.summary(res))
    assert not res["failures"], res["failures"]


# ---- teeth: wrong models break the bound on the same counts ------------------------------------------
def test_teeth_without_rule_4(pkg, trees):
    w, obs = oracle_run(pkg, trees, "leduc3")
    out = rd.check_counts(model_of(trees, "leduc3", w, rule4=False), obs, 0, N_LANES, 0, z_file(trees), cut=CUT)
    print(rd.summary(out), out["failures"][:3])
    assert out["failures"]


@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_teeth_dealer_fixed(pkg, trees, case):
    w, obs = oracle_run(pkg, trees, case)
    out = rd.check_counts(model_of(trees, case, w), obs, 0, N_LANES, 0, z_file(trees), cut=CUT, n_by_dealer=(N_LANES, 0))
    assert out["failures"]


def test_teeth_without_rule_3(pkg, trees):
    """Remapped rows in the action counters and the stored action rows.  (In the counters alone
    the wrong model is off by |z| 6.0 at most at 3,000 lanes -- Kuhn's raises, 720 counted against
    591.6 +- 21.5 -- which is inside z*: test_teeth_remapped_action_counters_alone holds it to
    |z| = 4, and tests/test_gpu_rollout_dist.py to z* at 262,144 lanes.)"""
    for case in ORACLE_CASES:
        w, obs = oracle_run(pkg, trees, case)
        out = rd.check_counts(model_of(trees, case, w, rule3=False), obs, 0, N_LANES, 0, z_file(trees), cut=CUT)
        print(case, out["failures"][:3])
        assert out["failures"]


def test_teeth_remapped_action_counters_alone(pkg, trees):
    """The counters-only wrong model (``remap_counters``; the stored rows stay un-remapped) on
    Kuhn's oracle counts.  It stays inside this file's z* at 3,000 lanes, so it is held to
    |z| = 4 instead: a threshold the right model passes in every statistic with probability
    1 - 111 erfc(4 / sqrt 2) = 0.993 and the wrong one misses on seat 0's and seat 1's raises,
    whose expectation it moves by 137 and 152 at a standard deviation of 22."""
    w, obs = oracle_run(pkg, trees, "kuhn248")
    right = rd.check_counts(model_of(trees, "kuhn248", w), obs, 0, N_LANES, 0, 4.0, cut=CUT)
    wrong = rd.check_counts(model_of(trees, "kuhn248", w, remap_counters=True), obs, 0, N_LANES, 0, 4.0, cut=CUT)
    print(wrong["failures"])
    assert not right["failures"], right["failures"]
    assert any(f.startswith("raises of seat 0") for f in wrong["failures"])
    assert any(f.startswith("raises of seat 1") for f in wrong["failures"])


def test_negative_eta_and_epsilon_are_accepted(pkg):
    """tests/test_gpu_rollout_dist.py's cases e0 and f0 set eta = -1 and epsilon = -1 to make
    ``u > x`` certain (rule 6: the only way to a probability of exactly 0).  The cfg rules
    (csrc/engine_cfg.h engine_cfg_rule, host only) must go on accepting them."""
    L = pkg.native.load()
    for kw in (dict(eta=-1.0), dict(epsilon=-1.0)):
        c = pkg.native.EngineCfg()
        assert L.nfsp_engine_default_cfg(C.byref(c)) == pkg.native.OK
        c.n_lanes, c.sched = 1024, 0
        for k, v in kw.items():
            setattr(c, k, v)
        arr = (pkg.native.EngineCfg * 1)(c)
        assert L.nfsp_group_cfgs_check(arr, 1, 0) == pkg.native.OK, L.nfsp_last_error().decode()
